"""
CPU: the bookkeeping of the device gauge log (csrc/gauge_log.hpp: pcl::GaugeLog) through its pure-host trace entry point
pcl_gauge_log_trace, against the rule restated here.

State: armed, capacity, count (records held), last (the last step call wrote record count - 1 and nothing has popped it).
1. arm(capacity): armed, count = 0, last = false.  disarm: not armed, everything zero.
2. a step: refused (-1, nothing changes) when not armed or count == capacity; else it writes slot `count`, then
   count += 1 and last = true.  A slot handed out is always < capacity.
3. undo / restore: if last: count -= 1, last = false, reported 1; else nothing, reported 0.
4. a read returns count records, then count = 0 and last = false.
"""
import os
import random
import re

import numpy as np

from pyclaw_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pyclaw_amd", "csrc", "pclaw.hip")

ARM, STEP, UNDO, RESTORE, READ, DISARM = range(6)


def trace(events):
    """events: (event, a) each; returns (value, count, last, armed) per event"""
    n = len(events)
    ev, a = (np.array([e[k] for e in events], dtype=np.int32) for k in range(2))
    out = np.full(4 * n, -99, dtype=np.int32)
    L.check(L.lib().pcl_gauge_log_trace(n, L.i(ev), L.i(a), L.i(out)))
    return [tuple(r) for r in out.reshape(n, 4).tolist()]


def rule(events):
    armed, cap, count, last, out = False, 0, 0, False, []
    for ev, a in events:
        v = 0
        if ev == ARM:
            armed, cap, count, last = True, a, 0, False
        elif ev == DISARM:
            armed, cap, count, last = False, 0, 0, False
        elif ev == STEP:
            if not armed or count == cap:
                v = -1
            else:
                v, count, last = count, count + 1, True
        elif ev in (UNDO, RESTORE):
            if armed and last:
                v, count, last = 1, count - 1, False
        elif ev == READ:
            v, count, last = count, 0, False
        out.append((v, count, int(last), int(armed)))
    return out


def values(events):
    return [r[0] for r in trace(events)], [r[1] for r in trace(events)]


def test_step_undo_step_keeps_one_record():
    v, count = values([(ARM, 4), (STEP, 0), (UNDO, 0), (STEP, 0)])
    assert v == [0, 0, 1, 0] and count == [0, 1, 0, 1]          # the retake writes the slot of the rejected step
    # the redo of ClawSolver.step at cfl == cfl_max behind an accepted step: the accepted record stays
    v, count = values([(ARM, 4), (STEP, 0), (STEP, 0), (UNDO, 0), (STEP, 0), (READ, 0)])
    assert v == [0, 0, 1, 1, 1, 2] and count == [0, 1, 2, 1, 2, 0]


def test_undo_twice_pops_once():
    v, count = values([(ARM, 4), (STEP, 0), (STEP, 0), (UNDO, 0), (UNDO, 0), (RESTORE, 0)])
    assert v == [0, 0, 1, 1, 0, 0] and count == [0, 1, 2, 1, 1, 1]


def test_restore_without_a_step_pops_nothing():
    v, count = values([(ARM, 4), (RESTORE, 0), (STEP, 0), (READ, 0), (RESTORE, 0), (UNDO, 0)])
    assert v == [0, 0, 0, 1, 0, 0] and count == [0, 0, 1, 0, 0, 0]
    assert values([(RESTORE, 0), (UNDO, 0), (STEP, 0)]) == ([0, 0, -1], [0, 0, 0])       # never armed: nothing recorded


def test_step_past_capacity_is_refused():
    cap = 3
    rows = trace([(ARM, cap)] + [(STEP, 0)] * (cap + 2) + [(UNDO, 0), (STEP, 0), (STEP, 0)])
    assert [r[0] for r in rows[1:cap + 1]] == [0, 1, 2]
    assert rows[cap + 1][:2] == (-1, cap) and rows[cap + 2][:2] == (-1, cap)     # refused, the count left alone
    # the refused steps wrote nothing: the undo takes the last WRITTEN record, whose slot the next step gets again
    assert rows[cap + 3][:2] == (1, cap - 1) and rows[cap + 4][:2] == (cap - 1, cap) and rows[cap + 5][:2] == (-1, cap)


def test_read_resets():
    rows = trace([(ARM, 2), (STEP, 0), (STEP, 0), (READ, 0), (UNDO, 0), (STEP, 0), (READ, 0), (READ, 0)])
    assert [r[:3] for r in rows] == [(0, 0, 0), (0, 1, 1), (1, 2, 1), (2, 0, 0), (0, 0, 0), (0, 1, 1), (1, 0, 0), (0, 0, 0)]


def test_rearm_resets():
    rows = trace([(ARM, 2), (STEP, 0), (STEP, 0), (ARM, 5), (UNDO, 0), (STEP, 0), (DISARM, 0), (STEP, 0), (ARM, 1), (STEP, 0)])
    assert [r[0] for r in rows] == [0, 0, 1, 0, 0, 0, 0, -1, 0, 0]
    assert [r[1] for r in rows] == [0, 1, 2, 0, 0, 1, 0, 0, 0, 1]
    assert [r[3] for r in rows] == [1, 1, 1, 1, 1, 1, 0, 0, 1, 1]


def test_random_traces_follow_the_rule():
    rng = random.Random(7)
    for _ in range(200):
        events = [(ARM, rng.randint(1, 4))] if rng.random() < 0.9 else []
        for _ in range(40):
            ev = rng.choices([ARM, STEP, UNDO, RESTORE, READ, DISARM], weights=[1, 12, 4, 2, 2, 1])[0]
            events.append((ev, rng.randint(1, 4) if ev == ARM else 0))
        got = trace(events)
        assert got == rule(events), events
        # the log never writes past its end
        cap = 0
        for (ev, a), (v, count, _, _) in zip(events, got):
            cap = a if ev == ARM else 0 if ev == DISARM else cap
            assert 0 <= count <= cap and (ev != STEP or v < cap)


def test_bad_events_are_refused():
    out = np.zeros(4, dtype=np.int32)
    for ev, a in ((9, 0), (ARM, 0)):
        rc = L.lib().pcl_gauge_log_trace(1, L.i(np.array([ev], dtype=np.int32)), L.i(np.array([a], dtype=np.int32)), L.i(out))
        assert rc == L.EINVAL


def test_undo_and_restore_pop():
    """the two calls that take a step back take its record back"""
    src = re.sub(r"//[^\n]*", "", open(SRC).read())
    for name in ("pcl_undo_step", "pcl_restore"):
        body = src[src.index("int %s(pcl_solver *s" % name):]
        assert "s->glog.pop();" in body[:body.index("\n}\n")]


def test_whitelist_and_abi_tests_still_hold():
    """the new entry points invalidate the quiet tiles first and are bound in _lib.PROTOTYPES (the checks of
    tests/test_quiet_tiles_cpu.py and tests/test_abi.py, run on this tree)"""
    import test_abi
    import test_quiet_tiles_cpu
    eps = test_quiet_tiles_cpu.entry_points()
    for name in ("pcl_gauge_log", "pcl_gauge_log_read", "pcl_gauge_log_stats"):
        assert name in eps and name in L.PROTOTYPES
    assert "pcl_gauge_log_trace" in L.PROTOTYPES
    test_quiet_tiles_cpu.test_every_other_entry_point_invalidates_first()
    test_quiet_tiles_cpu.test_step_entry_points_drop_then_restore()
    test_abi.test_library_exports_every_declared_symbol()
