"""
CPU: step ahead (pcl_step_ahead, include/pyclaw_amd.h).  The library enqueues the next step
with the dt the caller is about to compute, and adopts it only for the same 64 bits: pcl_step_ahead_dt must be Python's
min(dt_max, dt * cfl_desired / cfl) bit for bit.  The source-level rules the scheme rests on are checked as the other
*_cpu tests check theirs: the new entry points invalidate the quiet tiles first, pcl_bc_step still takes the valid flag
once and first, the calls that report on the last launch drop a pending step before anything else, and a step is run
ahead of only for a Courant number strictly below cfl_max.
"""
import os
import re
import struct

import numpy as np

from pyclaw_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pyclaw_amd", "csrc", "pclaw.hip")


def bits(x):
    return struct.pack("<d", x)


def python_dt(dt, cfl, cfl_desired, dt_max):
    """solver.py, evolve_to_time, behind an accepted step with cfl > 0"""
    return min(dt_max, dt * cfl_desired / cfl)


def cases():
    rng = np.random.default_rng(15)
    n = 100000
    dt = 10.0 ** rng.uniform(-12, 2, n)
    cfl = rng.uniform(1e-6, 1.0, n)
    des = rng.uniform(0.05, 1.0, n)
    dtm = np.where(rng.random(n) < 0.3, dt * rng.uniform(0.5, 2.0, n), 1e99)       # dt_max hit about every sixth time
    out = list(zip(dt.tolist(), cfl.tolist(), des.tolist(), dtm.tolist()))
    tiny, big = 5e-324, 1.7976931348623157e308
    cfl_max = 0.5
    near = [np.nextafter(cfl_max, 0.0), cfl_max, np.nextafter(cfl_max, 1.0), np.nextafter(0.45, 0.0), 0.45]
    for d in (tiny, 3 * tiny, 2.2250738585072014e-308, 1e-310, 1e-300, 0.001, 1.0 / 3.0, 1.0, big):
        with np.errstate(over="ignore"):
            around = (float(np.nextafter(d, 0.0)), float(np.nextafter(d, np.inf)))
        for c in near + [tiny, 1e-300, 1e-17, 1.0, 3.0, big]:
            for des_ in (0.45, 0.9, 1.0, tiny):
                for m in (1e99, d) + around + (0.0, tiny, big, float("inf")):
                    out.append((float(d), float(c), des_, float(m)))
    # the quotient equal to dt_max exactly (a tie goes to dt_max: the same value, and the same bits), and unordered
    out += [(0.5, 0.25, 0.5, 1.0), (0.0, 0.3, 0.45, 1.0), (-0.0, 0.3, 0.45, 1.0), (float("inf"), 0.3, 0.0, 1.0),
            (1.0, 0.3, 0.45, float("nan")), (float("nan"), 0.3, 0.45, 2.0)]
    return out


def test_dt_rule_bit_for_bit():
    L = _lib.lib()
    cs = cases()
    assert len(cs) >= 100000
    bad = []
    with np.errstate(all="ignore"):
        for dt, cfl, des, dtm in cs:
            want, got = python_dt(dt, cfl, des, dtm), L.pcl_step_ahead_dt(dt, cfl, des, dtm)
            if bits(want) != bits(got) and not (want != want and got != got):
                bad.append((dt, cfl, des, dtm, want, got))
    assert not bad, bad[:5]
    # some of each kind were in there
    assert sum(1 for c in cs if python_dt(*c) == c[3]) > 1000 and sum(1 for c in cs if python_dt(*c) < c[3]) > 1000


def code():
    return re.sub(r"//[^\n]*", "", open(SRC).read())


def body(src, head):
    b = src[src.index(head):]
    return b[:b.index("\n}\n")]


def test_new_entry_points_invalidate_first():
    src = open(SRC).read()
    for name in ("pcl_step_ahead", "pcl_step_ahead_stats"):
        m = re.search(r"^int %s\(pcl_solver \*s\b[^{;]*\{\n([^\n]*)\n" % name, src, re.M)
        assert m and m.group(1).strip().startswith("if (s) s->qt.invalidate();"), name
    # the dt rule takes no solver and touches no device
    b = body(code(), "double pcl_step_ahead_dt(double dt, double cfl, double cfl_desired, double dt_max)")
    assert "hip" not in b and "->" not in b
    assert re.search(r"dt \* cfl_desired / cfl;", b) and re.search(r"x < dt_max \? x : dt_max", b)


def test_bc_step_takes_the_flag_once_and_first():
    b = body(code(), "int pcl_bc_step(pcl_solver *s")
    uses = [m.group(0) for m in re.finditer(r"\bqt\b[^;]*;", b)]
    assert uses and uses[0].startswith("qt.take_valid()") and sum("take_valid" in u for u in uses) == 1, uses
    # adopt or drop comes before the step's own plans, and behind the flag
    assert b.index("take_valid") < b.index("ahead_matches") < b.index("ahead_drop") < b.index("step_loading_bcs")


def test_reporting_calls_drop_a_pending_step_first():
    src = code()
    for name in ("pcl_undo_step", "pcl_tile_words", "pcl_tile_list_classes", "pcl_tile_ring_stats",
                 "pcl_tile_rowreuse_stats", "pcl_tile_ycol_stats", "pcl_step_ahead"):
        b = body(src, "int %s(pcl_solver *s" % name)
        lines = [ln.strip() for ln in b.split("\n")[1:] if ln.strip()]
        assert lines[0].startswith("if (s) s->qt.invalidate();"), name
        drop = [k for k, ln in enumerate(lines) if "ahead_drop(s)" in ln]
        assert drop and drop[0] <= 2, (name, lines[:4])
    # pcl_tile_skip_stats is read-only for the quiet tiles, but it reports on the last launch: the drop comes before it reads
    b = body(src, "int pcl_tile_skip_stats(pcl_solver *s")
    assert b.index("ahead_drop(s)") < b.index("last_launch()")


def test_run_ahead_only_strictly_below_cfl_max():
    b = body(code(), "static int ahead_enqueue(pcl_solver *s")
    assert re.search(r"if \(!\(c > 0\.0 && c < a\.cfl_max\)\) return PCL_OK;", b)
    assert b.index("c < a.cfl_max") < b.index("do_step2ds")
    # the pre-step buffer is given up before the launch that overwrites it
    assert b.index("undo_slot = nullptr") < b.index("do_step2ds")
