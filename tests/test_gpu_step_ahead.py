"""
GPU: step ahead (pcl_step_ahead, include/pyclaw_amd.h) changes nothing but the time.  Every
case drives pcl_bc_step from here the way evolve_to_time does -- accept or undo, dt = min(dt_max, dt * cfl_desired / cfl)
-- once with the solver armed and once not, and the two runs must agree in every byte of the final q (no sign-of-zero
normalisation), in (dt bits, Courant bits, return code) of every step call and every other logged call, and in
pcl_step_count.  The armed run must have adopted steps unless the case says otherwise.
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

import test_gpu_quiet_tiles as Q
import test_gpu_tile_handover as H

pytestmark = pytest.mark.gpu

B = pyclaw.BC
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCL_ESTATE = -5


def shockbubble(mx, my, with_src=True):
    def make():
        return problems.shockbubble(pyclaw, mx=mx, my=my, tfinal=1.0, device_callbacks=True, with_src=with_src,
                                    dt_initial=0.005 * 160 / mx, run=False)
    return make


def blob_case(src=False, dt0=1.0):
    return H.euler_case(420, 180, 1.0, H.moving_blob(0.5, 0.3), bc=(B.outflow,) * 4, src=src, dt_variable=True,
                        cfl=(0.5, 0.45), dt0=dt0)


class Run:
    """one solver handle, stepped through the C API"""

    def __init__(self, make, armed, dt_max=None, rule=1, keep_dt=False):
        """rule: what the solver is armed with (1: the dt rule, 2: the same dt again); keep_dt: what the caller does
        behind an accepted step"""
        self.rule, self.keep_dt = rule, keep_dt
        self.L = L = _lib.lib()
        self.claw = make()
        self.solver, self.solution = self.claw.solver, self.claw.solution
        s = self.solver
        s.setup(self.solution)
        s._push(self.solution.state)
        self.h = s._h
        spec = s._device_bc_spec(self.solution.state)
        self.bc, self.cs = spec[2], spec[3]
        self.spec = spec                       # (keeps the arrays behind the pointers alive)
        self.cfl_max, self.cfl_desired = float(s.cfl_max), float(s.cfl_desired)
        self.dt_max = float(s.dt_max) if dt_max is None else dt_max
        self.dt = float(s.dt_initial)
        self.armed = armed
        self.log = []
        self.k = 0
        if armed:
            self.arm(rule)

    def arm(self, on):
        _lib.check(self.L.pcl_step_ahead(self.h, on, self.cfl_desired, self.cfl_max, self.dt_max))

    def step(self, dt=None, bc=None):
        """one pcl_bc_step and what evolve_to_time does behind it; returns True if the step was accepted"""
        dt = self.dt if dt is None else dt
        cfl = ctypes.c_double(0.0)
        rc = self.L.pcl_bc_step(self.h, self.bc if bc is None else bc, self.cs, dt,
                                ctypes.cast(ctypes.byref(cfl), _lib.dp))
        c = cfl.value
        self.log.append(("bc_step", rc, float(dt).hex(), float(c).hex()))
        assert rc == 0, self.log[-1]
        self.k += 1
        ok = c <= self.cfl_max
        if not ok:
            self.log.append(("undo", self.L.pcl_undo_step(self.h)))
        if not (ok and self.keep_dt):       # (evolve_to_time called for one step keeps dt behind an accepted one)
            self.dt = min(self.dt_max, dt * self.cfl_desired / c) if c > 0.0 else self.dt_max
        return ok

    def stats(self):
        """(enqueued, adopted, dropped); not a read-only call"""
        a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        _lib.check(self.L.pcl_step_ahead_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def skip_stats(self):
        a, b = ctypes.c_long(), ctypes.c_long()
        _lib.check(self.L.pcl_tile_skip_stats(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def q_bytes(self):
        """the interior of the state as the library holds it (read-only: leaves a pending step pending)"""
        st = self.solution.state
        buf = np.empty(st.meqn * int(np.prod(st.grid.ng)))
        _lib.check(self.L.pcl_get_q(self.h, _lib.d(buf), 0))
        return buf

    def count(self):
        n = ctypes.c_long()
        _lib.check(self.L.pcl_step_count(self.h, ctypes.byref(n)))
        return n.value

    def close(self):
        q = self.q_bytes()
        out = (hashlib.sha256(q.tobytes()).hexdigest(), bool(np.isfinite(q).all()), self.count(), self.log,
               self.stats() if self.armed else (0, 0, 0))
        self.solver.teardown()
        return out


def both(make, script, dt_max=None, adopts=True, **kw):
    """script(run) drives one Run; returns (armed, plain) = (hash, finite, step count, log, ahead stats)"""
    res = []
    for armed in (True, False):
        r = Run(make, armed, dt_max, **kw)
        script(r)
        res.append(r.close())
    on, off = res
    assert on[1], "non-finite state"
    assert on[3] == off[3], [(a, b) for a, b in zip(on[3], off[3]) if a != b][:3]
    assert on[2] == off[2], "step counts differ"
    assert on[0] == off[0], "final states differ"
    enq, ado, dro = on[4]
    assert 0 <= enq - ado - dro <= 1, on[4]
    if adopts:
        assert ado > 0, on[4]
    return on, off


def steady(n):
    def script(r):
        for _ in range(n):
            r.step()
    return script


@pytest.mark.parametrize("make", [shockbubble(960, 480), shockbubble(427, 197), blob_case(dt0=0.2)],
                         ids=["shockbubble960", "shockbubble427", "blob420"])
def test_steady_run(make):
    on, _ = both(make, steady(60))
    enq, ado, dro = on[4]
    # nearly every accepted step was the one enqueued behind the step before it
    accepted = sum(1 for e in on[3] if e[0] == "bc_step") - sum(1 for e in on[3] if e[0] == "undo")
    assert ado >= accepted - 8, (on[4], accepted)


@pytest.mark.parametrize("make", [shockbubble(427, 197), blob_case(dt0=1.0)], ids=["shockbubble427", "blob420"])
def test_caller_keeps_dt(make):
    """armed with rule 2, the caller takes the same dt again behind an accepted step (evolve_to_time called per step):
    the Courant number stays away from cfl_desired, and the steps are adopted all the same"""
    on, _ = both(make, steady(40), rule=2, keep_dt=True)
    assert any(e[0] == "undo" for e in on[3])
    assert on[4][1] >= 30 and on[4][2] == 0, on[4]


def test_wrong_rule_backs_off():
    """armed with the dt rule while the caller keeps dt: every pending step is the wrong one.  The library runs ahead of
    ever fewer steps (1, 2, 4, ... steps left out behind each miss: calls 1, 3, 6, 11, 20 and 37 meet a pending step):
    40 steps cost at most 6 launches for nothing"""
    on, _ = both(blob_case(dt0=0.2), steady(40), rule=1, keep_dt=True, adopts=False)
    assert on[4][1] == 0 and 3 <= on[4][2] <= 6, on[4]


def test_long_launches_are_not_run_ahead_of():
    """a dense state on 65 x 65 tiles: every launch runs over all 4225 tiles, more than 4096 and more than a quarter of
    the grid; nothing is enqueued ahead (a wrong guess would cost a whole such launch)"""
    make = Q.euler_case(3900, 780, [B.reflecting, B.outflow, B.periodic, B.periodic], Q.dense, dt_variable=True,
                        cfl=(0.5, 0.45))
    on, _ = both(make, steady(6), adopts=False)
    assert on[4] == (0, 0, 0), on[4]


def test_rejected_steps():
    """a first dt too large, then dt growing until a step is rejected: nothing is enqueued behind a rejected step, the undo
    works there and the retaken step is right (the runs agree)"""
    seen = []

    def script(r):
        for _ in range(40):
            before = r.stats() if r.armed else None
            ok = r.step()
            if not ok:
                assert r.log[-1] == ("undo", 0)
                if r.armed:
                    after = r.stats()
                    # whatever was pending in front of the call is settled; the rejected step enqueued nothing
                    assert after[0] == before[0] and after[0] == after[1] + after[2], (before, after)
                    seen.append(after)
    on, _ = both(blob_case(dt0=1.0), script, adopts=False)
    assert seen and any(e[0] == "undo" for e in on[3])


def test_rejected_steps_steady():
    """the same run without the stats calls in between (they drop what is pending): steps are adopted around the rejected ones"""
    on, _ = both(blob_case(dt0=1.0), steady(40))
    assert any(e[0] == "undo" for e in on[3])


@pytest.mark.parametrize("what", ["ulp", "spec"])
def test_mismatch_every_fifth_step(what):
    after = []

    def script(r):
        other = np.array([B.outflow, B.outflow, B.outflow, B.reflecting], dtype=np.int32)
        for k in range(40):
            if k % 5 == 4:
                if what == "ulp":
                    r.step(dt=float(np.nextafter(r.dt, 0.0)))
                else:
                    r.step(bc=_lib.i(other))
                if r.armed:
                    after.append(r.skip_stats())         # the step asked for was not the pending one: every tile
            else:
                r.step()
    on, _ = both(blob_case(dt0=0.2), script)
    assert len(after) == 8 and all(s == 0 and c > 0 for c, s in after), after
    assert on[4][2] >= 8, on[4]


def test_dt_max_picked():
    """dt_max below what the rule predicts: the min picks dt_max, and that is the dt enqueued"""
    dt_max = 0.2 / 420 * 1.01
    on, _ = both(blob_case(dt0=0.2), steady(30), dt_max=dt_max)
    dts = [float.fromhex(e[2]) for e in on[3] if e[0] == "bc_step"]
    assert sum(1 for d in dts if d == dt_max) >= 25, dts
    assert on[4][1] >= 25, on[4]


def test_calls_between_steps():
    """pcl_put_q, a tile hook and pcl_fuse_source drop the pending step; pcl_get_q sees state n and leaves it pending"""
    events = {6: "put", 11: "words", 16: "fuse", 21: "get", 22: "get", 23: "get"}
    marks = []

    def script(r):
        L = r.L
        for k in range(30):
            r.step()
            what = events.get(k)
            if what == "put":
                buf = r.q_bytes()
                _lib.check(L.pcl_put_q(r.h, _lib.d(buf), 0))
            elif what == "words":
                ntx, nty = ctypes.c_int(), ctypes.c_int()
                _lib.check(L.pcl_tile_words(r.h, None, ctypes.byref(ntx), ctypes.byref(nty)))
            elif what == "fuse":
                _lib.check(L.pcl_fuse_source(r.h, 0, None, 0))
            elif what == "get":
                r.log.append(("get", hashlib.sha256(r.q_bytes().tobytes()).hexdigest()))
            if r.armed and k in (7, 12, 17, 24):
                marks.append((k, r.skip_stats()))
    on, _ = both(blob_case(dt0=0.2), script)
    m = dict(marks)
    # behind put, hook and fuse the next launch computed every tile; behind the gets the adopted step still skipped
    assert m[7][1] == 0 and m[12][1] == 0 and m[17][1] == 0 and m[24][1] > 0, marks
    # dropped: the three events, and the four skip_stats calls of the armed run
    assert on[4][2] == 7, on[4]


def test_undo_behind_an_accepted_armed_step():
    r = Run(blob_case(dt0=0.2), True)
    for _ in range(10):
        assert r.step()
    q = r.q_bytes()
    assert r.L.pcl_undo_step(r.h) == PCL_ESTATE
    assert np.array_equal(q.view(np.uint64), r.q_bytes().view(np.uint64))
    for _ in range(5):
        r.step()
    on = r.close()
    p = Run(blob_case(dt0=0.2), False)
    for _ in range(15):
        p.step()
    off = p.close()
    assert on[:4] == off[:4]


def quiet_cold_gas(mx, my):
    """gas at rest with a sound speed of about 1e-9 and a denser blob in it: dt = 2^19 gives a Courant number of 0.15 (along
    x, dx = 1 / 210), so the rule settles at three times that dt"""
    p = (0.15 * (1.0 / 210) / 2.0 ** 19) ** 2 / Q.GAMMA
    q = Q.uniform(mx, my, (1.0, 0.0, 0.0, p / Q.GAMMA1, 0.0))
    i, j = np.meshgrid(np.arange(mx), np.arange(my), indexing='ij')
    inside = (i - mx // 2) ** 2 + (j - my // 2) ** 2 < (min(mx, my) // 10) ** 2
    q[0][inside] = 3.0
    q[4][inside] = 1.0
    return q


def test_fused_source_dt_under_and_over_its_bound():
    """the fused source's fixed-point bound is dt <= 2^20: the rule takes dt from 2^19 to beyond it, and the steps
    enqueued ahead with such a dt compute every tile as the ordinary ones do"""
    make = H.euler_case(420, 180, 1.0, quiet_cold_gas, bc=(B.outflow,) * 4, src=True, dt_variable=True, cfl=(0.5, 0.45),
                        dt0=420 * 2.0 ** 19)
    on, _ = both(make, steady(20))
    dts = [float.fromhex(e[2]) for e in on[3] if e[0] == "bc_step"]
    assert dts[0] <= 2.0 ** 20 and sum(1 for d in dts if d > 2.0 ** 20) >= 10, dts
    both(blob_case(src=True, dt0=0.2), steady(30))


def test_form_trials():
    """the default form policy through a trial window (steps 64..71 of 320): bytes and step sequence only"""
    make = H.euler_case(600, 240, 1.5, H.moving_blob(0.6, 0.2), dt_variable=True, cfl=(0.5, 0.45), dt0=0.2)
    forms = []

    def script(r):
        for _ in range(320):
            r.step()
        ms, n, one, two = ctypes.c_double(), ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        _lib.check(r.L.pcl_step_form_stats(r.h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(one), ctypes.byref(two)))
        forms.append((one.value, two.value))
    both(make, script)
    assert all(one + two == 320 and two >= 3 for one, two in forms), forms      # both runs met the trial steps


def test_disarm_and_destroy_with_a_step_pending():
    def script(r):
        for _ in range(10):
            r.step()
        if r.armed:
            r.arm(0)                # a step is pending here
        for _ in range(10):
            r.step()
        if r.armed:
            r.arm(1)
        for _ in range(5):
            r.step()                # ... and here, when close() destroys the handle
    on, _ = both(blob_case(dt0=0.2), script)
    assert on[4][2] >= 1, on[4]
    # destroyed right behind a step, nothing read in between
    r = Run(blob_case(dt0=0.2), True)
    for _ in range(6):
        r.step()
    r.solver.teardown()


PY_RUN = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
import pyclaw_amd as pyclaw
from apps import problems
out = []
for with_src in (True, False):
    for tend in (None, 0.004):
        claw = problems.shockbubble(pyclaw, mx=960, my=480, tfinal=1.0, device_callbacks=True, with_src=with_src,
                                    dt_initial=0.005 * 160 / 960, run=False)
        solver, solution = claw.solver, claw.solution
        solver.setup(solution)
        solver.dt = solver.dt_initial
        solver.begin_resident(solution)
        frames, status = [], []
        for k in range(3):
            if tend is None:
                for _ in range(20):
                    status.append(sorted((a, float(b).hex()) for a, b in solver.evolve_to_time(solution).items()
                                         if a in ('cflmax', 'dtmin', 'dtmax', 'numsteps')))
            else:
                st = solver.evolve_to_time(solution, tend * (k + 1))
                status.append(sorted((a, float(b).hex()) for a, b in st.items() if a in ('cflmax', 'dtmin', 'dtmax', 'numsteps')))
            solver._pull(solution.state)
            frames.append(hashlib.sha256(np.ascontiguousarray(solution.state.q).tobytes()).hexdigest())
        armed = bool((getattr(solver, '_step_ahead_sent', None) or (False,))[0])
        solver.end_resident(solution)
        frames.append(hashlib.sha256(np.ascontiguousarray(solution.state.q).tobytes()).hexdigest())
        solver.teardown()
        out.append({"src": with_src, "tend": tend, "frames": frames, "status": status, "t": float(solution.t).hex(),
                    "sent": armed})
print("RESULT " + json.dumps(out))
"""


def test_through_python_resident_mode(monkeypatch, capsys):
    """resident mode with PCL_STEP_AHEAD unset (here) against =0 (the knob is read from the environment: a child
    process): per step and evolve_to_time(tend), with and without the radial source; identical frames and status"""
    import json

    def result(text):
        line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")][-1]
        return json.loads(line[len("RESULT "):])
    monkeypatch.delenv("PCL_STEP_AHEAD", raising=False)
    exec(compile(PY_RUN % {"root": ROOT}, "<resident run>", "exec"), {})
    on = result(capsys.readouterr().out)
    env = dict(os.environ, PCL_STEP_AHEAD="0")
    p = subprocess.run([sys.executable, "-c", PY_RUN % {"root": ROOT}], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    off = result(p.stdout)
    strip = lambda rs: [{k: v for k, v in r.items() if k != 'sent'} for r in rs]
    assert strip(on) == strip(off)
    assert len(on) == 4 and all(len(r["frames"]) == 4 for r in on)
    assert all(r["sent"] for r in on) and not any(r["sent"] for r in off)


def test_python_arms_in_resident_mode_only():
    claw = shockbubble(427, 197)()
    solver, solution = claw.solver, claw.solution
    solver.setup(solution)
    solver.dt = solver.dt_initial
    solver.evolve_to_time(solution)
    assert not getattr(solver, '_step_ahead_sent', None)
    solver.begin_resident(solution)
    for _ in range(12):
        solver.evolve_to_time(solution)
    assert solver._step_ahead_sent == (2, 0.45, 0.5, float(solver.dt_max))
    a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.lib().pcl_step_ahead_stats(solver._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    assert b.value >= 8, (a.value, b.value, c.value)
    solver.end_resident(solution)
    assert solver._step_ahead_sent[0] == 0
    solver.teardown()
