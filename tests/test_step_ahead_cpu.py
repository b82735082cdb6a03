"""
CPU: step ahead (pcl_step_ahead, include/pyclaw_amd.h).  The library enqueues the next step
with the dt the caller is about to compute, and adopts it only for the same 64 bits: pcl_step_ahead_dt must be Python's
min(dt_max, dt * cfl_desired / cfl) bit for bit.  The decisions (csrc/step_ahead.hpp: pcl::StepAhead) are driven
through the pure-host trace entry point pcl_step_ahead_trace: a step is run ahead of only for a Courant number strictly
below cfl_max, the back-off after misses, the long-launch bound, rule 2, and what "the same step" means.  The
source-level rules the scheme rests on are checked as the other *_cpu tests check theirs: the new entry points
invalidate the quiet tiles first, pcl_bc_step still takes the valid flag once and first, the calls that report on the
last launch drop a pending step before anything else, and the pre-step buffer is given up before the launch that
overwrites it.
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
    assert b.index("take_valid") < b.index("ahead.matches(") < b.index("ahead_drop") < b.index("step_loading_bcs")


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


def test_undo_slot_is_given_up_before_the_launch():
    b = body(code(), "static int ahead_enqueue(pcl_solver *s")
    # the type's own checks (the Courant bound among them: below) come before the launch, the solver's before those
    assert b.index("list_behind_last()") < b.index("ahead.wants(") < b.index("do_step2ds") < b.index("ahead.enqueued(")
    # the pre-step buffer is given up before the launch that overwrites it
    assert b.index("undo_slot = nullptr") < b.index("do_step2ds")


# ---- the decisions, through pcl_step_ahead_trace ----
WANTS, NEXT_DT, ENQUEUED, MATCHES, MISSED, ADOPTED, DROPPED = range(7)
CFL_MAX = 0.5
OUTFLOW = [1, 1, 1, 1]


def trace(events, on=1, cfl_desired=0.45, cfl_max=CFL_MAX, dt_max=1e99):
    """events: dicts with ev and any of flag, x, y, ran, ntiles, bc (4 types), cstate (4 x 8); returns (out, out_dt)"""
    n = len(events)

    def g(k, dflt, dtype):
        return np.array([e.get(k, dflt) for e in events], dtype=dtype)

    ev, flag = g("ev", 0, np.int32), g("flag", 1, np.int32)
    x, y = g("x", 0.0, np.float64), g("y", 0.0, np.float64)
    ran, ntiles = g("ran", 100, np.int64), g("ntiles", 100000, np.int64)
    bc = np.array([e.get("bc", OUTFLOW) for e in events], dtype=np.int32).reshape(n, 4)
    cs = np.array([e.get("cstate", np.zeros((4, 8))) for e in events], dtype=np.float64).reshape(n, 32)
    out, out_dt = np.full(n, -99, dtype=np.int32), np.full(n, -99.0)
    lp = _lib.C.POINTER(_lib.C.c_long)
    _lib.check(_lib.lib().pcl_step_ahead_trace(on, cfl_desired, cfl_max, dt_max, n, _lib.i(ev), _lib.i(flag), _lib.d(x),
                                               _lib.d(y), ran.ctypes.data_as(lp), ntiles.ctypes.data_as(lp), _lib.i(bc),
                                               _lib.d(cs), _lib.i(out), _lib.d(out_dt)))
    return out.tolist(), out_dt.tolist()


def wants(c=0.3, **kw):
    return dict(ev=WANTS, x=c, **kw)


def test_run_ahead_only_strictly_below_cfl_max():
    below, above = float(np.nextafter(CFL_MAX, 0.0)), float(np.nextafter(CFL_MAX, 1.0))
    cs = [CFL_MAX, below, above, 0.0, -0.0, -1.0, float("nan"), float("inf"), 5e-324, 0.3]
    out, _ = trace([wants(c) for c in cs])
    assert out == [0, 1, 0, 0, 0, 0, 0, 0, 1, 1]
    # not armed: never
    assert trace([wants(c) for c in cs], on=0)[0] == [0] * len(cs)
    # an unordered bound admits nothing
    assert trace([wants(c) for c in cs], cfl_max=float("nan"))[0] == [0] * len(cs)


def test_back_off_after_misses():
    def miss():
        return [wants(), dict(ev=ENQUEUED, x=0.1), dict(ev=MISSED), dict(ev=DROPPED)]

    # consecutive misses: the next 1, 2, 4 .. 64, 64 steps are not run ahead of
    ev, want = [], []
    for pause in (1, 2, 4, 8, 16, 32, 64, 64, 64):
        ev += miss() + [wants()] * pause
        want += [1, 0, 0, 1] + [0] * pause
    out, _ = trace(ev + [wants()])
    assert out == want + [1]
    # an adoption ends the run of misses, not a pause already running
    ev = miss() + [wants()] + miss() + [wants()] * 2 + miss()                   # three misses: a pause of 4 is running
    ev += [wants(), dict(ev=ENQUEUED, x=0.1), dict(ev=ADOPTED), wants(), wants(), wants(), wants()]
    ev += miss() + [wants(), wants()]                                           # the next miss pauses 1 again
    out, _ = trace(ev)
    assert out == [1, 0, 0, 1, 0] + [1, 0, 0, 1, 0, 0] + [1, 0, 0, 1] + [0, 0, 0, 0, 0, 0, 1] + [1, 0, 0, 1, 0, 1]
    # the countdown does not tick on a call that an earlier check refused: Courant bound, form check
    refused = [wants(CFL_MAX), wants(float("nan")), wants(flag=0), wants(0.0)]
    ev = miss() + [wants()] + miss() + refused * 3 + [wants(), wants(), wants()]
    out, _ = trace(ev)
    assert out == [1, 0, 0, 1, 0] + [1, 0, 0, 1] + [0] * 12 + [0, 0, 1]
    # ... but it does on one that only the long-launch bound would refuse (that check comes behind it)
    ev = miss() + [wants(ran=50000, ntiles=100000), wants(ran=50000, ntiles=100000), wants()]
    assert trace(ev)[0] == [1, 0, 0, 1] + [0, 0, 1]
    # dropped() reports whether a step was pending, and the tile count of the step before it
    out, rep = trace([dict(ev=DROPPED), dict(ev=ENQUEUED, x=0.1, ran=77), dict(ev=DROPPED), dict(ev=DROPPED)])
    assert [out[0], out[2], out[3]] == [0, 1, 0] and rep[0] == -1.0 and rep[2] == 77.0 and rep[3] == 77.0


def test_long_launch_bound():
    # refused iff ran > 4096 and 4 ran > ntiles
    cases = [(4096, 4, 1), (4097, 4 * 4097, 1), (4097, 4 * 4097 - 1, 0), (4096, 4 * 4096 - 1, 1), (4097, 10 ** 9, 1),
             (10 ** 6, 4 * 10 ** 6, 1), (10 ** 6, 4 * 10 ** 6 - 1, 0), (0, 0, 1), (5000, 5000, 0)]
    out, _ = trace([wants(ran=r, ntiles=n) for r, n, _ in cases])
    assert out == [w for _, _, w in cases]


def test_next_dt_rules():
    dts = [0.001, 1.0 / 3.0, 5e-324, -0.0, 0.0, float("inf"), 1.7976931348623157e308]
    # rule 2: the dt's own bits
    _, got = trace([dict(ev=NEXT_DT, x=d, y=0.3) for d in dts] + [dict(ev=NEXT_DT, x=float("nan"), y=0.3)], on=2)
    assert [bits(g) for g in got[:-1]] == [bits(d) for d in dts] and got[-1] != got[-1]
    # rule 1: pcl_step_ahead_dt with the armed constants
    with np.errstate(all="ignore"):
        for des, dtm in ((0.45, 1e99), (0.9, 0.01)):
            _, got = trace([dict(ev=NEXT_DT, x=d, y=0.3) for d in dts], on=1, cfl_desired=des, dt_max=dtm)
            assert [bits(g) for g in got] == [bits(python_dt(d, 0.3, des, dtm)) for d in dts]


def test_matches_means_the_same_bits():
    nan = float("nan")
    cst = np.arange(32, dtype=np.float64).reshape(4, 8) + 0.5
    bc = [0, 1, 0, 3]                                           # sides 0 and 2 custom (PCL_BC_CUSTOM = 0)

    def asked(dt=0.1, bc=bc, cstate=cst, flag=1):
        return dict(ev=MATCHES, x=dt, bc=bc, cstate=cstate, flag=flag)

    def changed(k, m, v):
        c = cst.copy()
        c[k, m] = v
        return c

    ev = [dict(ev=ENQUEUED, x=0.1, bc=bc, cstate=cst),
          asked(), asked(flag=0), asked(dt=float(np.nextafter(0.1, 1.0))),
          asked(bc=[0, 1, 0, 2]), asked(bc=[0, 1, 1, 3]), asked(bc=[0, -1, 0, 3]),
          asked(cstate=changed(0, 0, 0.25)), asked(cstate=changed(2, 7, float(np.nextafter(23.5, 0.0)))),
          asked(cstate=changed(1, 3, 99.0)), asked(cstate=changed(3, 0, nan)),                  # non-custom sides: a match
          dict(ev=ENQUEUED, x=0.0, bc=bc, cstate=changed(0, 1, 0.0)),
          asked(dt=0.0, cstate=changed(0, 1, 0.0)), asked(dt=-0.0, cstate=changed(0, 1, 0.0)),
          asked(dt=0.0, cstate=changed(0, 1, -0.0)),
          dict(ev=ENQUEUED, x=nan, bc=bc, cstate=changed(2, 2, nan)),
          asked(dt=nan, cstate=changed(2, 2, nan)), asked(dt=nan), asked(dt=0.1, cstate=changed(2, 2, nan))]
    out, _ = trace(ev)
    assert out == [0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 0, 0]
    # not armed: nothing matches
    assert trace(ev[:2], on=0)[0] == [0, 0]
