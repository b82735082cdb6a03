"""
GPU: a skipping launch of the one-kernel dimension-split step runs a tile-list kernel in front and the step over the
listed tiles only (classic_fused.hpp).  Every case runs with pcl_tile_skip on and off in this process and
must give byte-identical final states (no sign-of-zero normalisation) and the same sequence of step calls: dt, Courant
number and return code of every step, every undo.  The count the list kernel leaves (pcl_tile_skip_stats) must match a
host recomputation of the skip rule from the words that launch read (pcl_tile_words).
"""
import ctypes
import hashlib

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

pytestmark = pytest.mark.gpu

GAMMA = 1.4
GAMMA1 = GAMMA - 1.0
TQ_ALL = 0x01010101
B = pyclaw.BC


def host_skipped(words, ntx, nty, mx, my):
    """tiles the skip rule skips: off the frame (16 x 64 window inside the grid) and a 3 x 3 quiet neighbourhood"""
    w = words.reshape(nty, ntx)
    n = 0
    for ty in range(nty):
        for tx in range(ntx):
            x0, y0 = 60 * tx, 12 * ty            # window origin, counted from the first interior cell minus 2
            if x0 < 2 or y0 < 2 or x0 + 64 > mx + 2 or y0 + 16 > my + 2:
                continue
            n += bool((w[ty - 1:ty + 2, tx - 1:tx + 2] == TQ_ALL).all())
    return n


class Recorder:
    """Wraps the step entry points the solvers call through: sets pcl_tile_skip once per handle, logs every step call
    with the tile counts after it, and at the steps in `check` compares the count with the host's recomputation."""
    NAMES = ("pcl_bc_step", "pcl_step_hyperbolic", "pcl_undo_step")

    def __init__(self, skip, shape, check=(), hook=None):
        self.skip, self.shape, self.check, self.hook = skip, shape, set(check), hook
        self.log, self.stats, self.seen, self.checked = [], [], set(), []

    def __enter__(self):
        L = _lib.lib()
        self.orig = {n: getattr(L, n) for n in self.NAMES}

        def first(h):
            key = h.value if hasattr(h, "value") else h
            if key not in self.seen:
                self.seen.add(key)
                _lib.check(L.pcl_tile_skip(h, 1 if self.skip else 0))

        def bc_step(h, bc, cs, dt, cfl):
            first(h)
            rc = self.orig["pcl_bc_step"](h, bc, cs, dt, cfl)
            self.after("bc_step", h, rc, dt, cfl)
            return rc

        def step(h, dt, cfl):
            first(h)
            rc = self.orig["pcl_step_hyperbolic"](h, dt, cfl)
            self.after("step", h, rc, dt, cfl)
            return rc

        def undo(h):
            rc = self.orig["pcl_undo_step"](h)
            self.log.append(("undo", rc))
            return rc

        L.pcl_bc_step, L.pcl_step_hyperbolic, L.pcl_undo_step = bc_step, step, undo
        return self

    def after(self, tag, h, rc, dt, cfl):
        L = _lib.lib()
        self.log.append((tag, rc, float(dt).hex(), float(cfl[0]).hex()))
        c, s = ctypes.c_long(), ctypes.c_long()
        _lib.check(L.pcl_tile_skip_stats(h, ctypes.byref(c), ctypes.byref(s)))
        self.stats.append((c.value, s.value))
        k = len(self.stats) - 1
        if self.skip and k in self.check:
            ntx, nty = ctypes.c_int(), ctypes.c_int()
            _lib.check(L.pcl_tile_words(h, None, ctypes.byref(ntx), ctypes.byref(nty)))
            nt = ntx.value * nty.value
            assert c.value + s.value == nt, (c.value, s.value, nt)
            words = np.zeros(nt, dtype=np.uint32)
            if L.pcl_tile_words(h, words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ntx), ctypes.byref(nty)) == 0:
                sk = host_skipped(words, ntx.value, nty.value, *self.shape)
                assert s.value == sk and c.value == nt - sk, (k, c.value, s.value, sk)
                self.checked.append((k, s.value))
        if self.hook is not None:
            self.hook(k, h, self)

    def __exit__(self, *exc):
        L = _lib.lib()
        for n, f in self.orig.items():
            setattr(L, n, f)
        return False


def final_bytes(claw):
    claw.solver.teardown()
    q = np.ascontiguousarray(claw.solution.state.q)
    return hashlib.sha256(q.tobytes()).hexdigest(), bool(np.isfinite(q).all())


def run_both(make, shape, check=(), hook_factory=None):
    res = []
    for skip in (True, False):
        claw = make()
        with Recorder(skip, shape, check, hook_factory() if hook_factory else None) as rec:
            claw.run()
            h, fin = final_bytes(claw)
        res.append((h, fin, rec.log, rec.stats, rec.checked))
    on, off = res
    assert on[1], "non-finite state"
    assert on[2] == off[2], "step sequences differ"
    assert on[0] == off[0], "final states differ"
    assert all(s == 0 for _, s in off[3]), off[3]
    assert len(on[4]) == len([k for k in check if k < len(on[3])]), (on[4], check)
    return on


def skipped(run):
    return sum(s for _, s in run[3])


def controller(state, solver, tfinal):
    claw = pyclaw.Controller()
    claw.keep_copy = False
    claw.output_format = None
    claw.tfinal = tfinal
    claw.nout = 1
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    return claw


def euler_case(mx, my, bc, init, src=False, steps=20, const=None):
    def make():
        x = pyclaw.Dimension('x', 0.0, 2.0, mx)
        y = pyclaw.Dimension('y', 0.0, 2.0 * my / mx, my)
        state = pyclaw.State(pyclaw.Grid([x, y]), 5, 1)
        state.aux_global['gamma'] = GAMMA
        state.aux_global['gamma1'] = GAMMA1
        state.q[...] = init(mx, my)
        problems.sb_auxinit(state)
        solver = pyclaw.ClawSolver2D()
        solver.rp = pyclaw.riemann.rp_euler_5wave_2d
        solver.mwaves = 5
        solver.limiters = [4, 4, 4, 4, 2]
        solver.dim_split = True
        if src:
            solver.src_split = 1
            solver.step_src = pyclaw.EulerRadialSource(GAMMA1, 2)
        solver.cfl_max, solver.cfl_desired = 1.0, 0.9
        solver.dt_variable = False
        solver.dt_initial = 0.2 / max(mx, my)
        for k in range(2):
            solver.bc_lower[k], solver.bc_upper[k] = bc[2 * k], bc[2 * k + 1]
            solver.aux_bc_lower[k] = solver.aux_bc_upper[k] = pyclaw.BC.outflow
        if const is not None:
            solver.user_bc_lower = solver.user_bc_upper = pyclaw.ConstantStateBC(np.array(const))
        return controller(state, solver, steps * solver.dt_initial)
    return make


def uniform(mx, my, s=(1.0, 0.0, 0.0, 2.5, 0.0)):
    return np.broadcast_to(np.array(s).reshape(5, 1, 1), (5, mx, my)).copy()


def blob(mx, my):
    q = uniform(mx, my)
    i, j = np.meshgrid(np.arange(mx), np.arange(my), indexing='ij')
    inside = (i - mx // 2) ** 2 + (j - my // 2) ** 2 < (min(mx, my) // 8) ** 2
    q[0][inside] = 3.0
    q[3][inside] = 7.0
    q[4][inside] = 1.0
    return q


def dense(mx, my):
    rng = np.random.default_rng(5)
    q = np.empty((5, mx, my))
    q[0] = 1.0 + 0.1 * rng.random((mx, my))
    q[1] = 0.1 * rng.random((mx, my))
    q[2] = 0.05 * rng.random((mx, my))
    q[3] = 2.5 + 0.1 * rng.random((mx, my))
    q[4] = rng.random((mx, my))
    return q


@pytest.mark.parametrize("with_src", [False, True])
def test_shockbubble(with_src):
    def make():
        claw = problems.shockbubble(pyclaw, mx=960, my=480, tfinal=0.04, device_callbacks=True, with_src=with_src,
                                    dt_initial=0.005 * 160 / 960, run=False)
        claw.keep_copy = False
        claw.output_format = None
        return claw
    on = run_both(make, (960, 480), check=(20, 45))
    assert sum(1 for e in on[2] if e[0] != "undo") >= 60, len(on[2])
    assert any(e[0] == "undo" for e in on[2])        # the app's first step is rejected
    assert skipped(on) > 0 and all(s > 0 for _, s in on[4]), on[4]


def test_periodic_counts():
    on = run_both(euler_case(600, 240, [B.periodic] * 4, blob, steps=24), (600, 240), check=(5, 12, 20))
    assert skipped(on) > 0 and all(s > 0 for _, s in on[4]), on[4]


def test_sides_not_multiples_of_the_tile():
    # 427 = 7 * 60 + 7, 197 = 16 * 12 + 5: partial last tile column and row
    on = run_both(euler_case(427, 197, [B.outflow] * 4, blob, steps=25), (427, 197), check=(10,))
    assert skipped(on) > 0


@pytest.mark.parametrize("mx,my", [(100, 300), (420, 20), (110, 22)])
def test_every_tile_on_the_frame(mx, my):
    # ntx or nty < 3: no tile is off the frame, a skipping launch lists every tile
    on = run_both(euler_case(mx, my, [B.outflow] * 4, blob, steps=12), (mx, my), check=(4,))
    assert skipped(on) == 0


@pytest.mark.parametrize("bc", [[B.outflow] * 4, [B.reflecting] * 4, [B.custom] * 4, [B.periodic] * 4,
                                [B.custom, B.outflow, B.reflecting, B.periodic],
                                [B.periodic, B.periodic, B.custom, B.reflecting]])
def test_sides(bc):
    const = [1.0, 0.0, 0.0, 2.5, 0.0] if B.custom in bc else None
    on = run_both(euler_case(420, 180, bc, blob, steps=20, const=const), (420, 180), check=(8,))
    assert skipped(on) > 0


def test_put_q_between_steps():
    def hook_factory():
        def hook(k, h, rec):
            if k in (6, 11):
                L = _lib.lib()
                mx, my = 420, 180
                buf = np.empty(5 * mx * my)
                _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
                a = buf.reshape(my, mx, 5)
                a[20 + k, 30 + 2 * k, 0] += 0.25
                _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))
        return hook
    on = run_both(euler_case(420, 180, [B.periodic] * 4, blob, steps=20), (420, 180), hook_factory=hook_factory)
    assert skipped(on) > 0
    assert on[3][7][1] == 0 and on[3][12][1] == 0, on[3]


def test_auto_form_past_trial_window():
    on = run_both(euler_case(600, 240, [B.periodic] * 4, blob, steps=80), (600, 240))
    assert skipped(on) > 0


def test_dense_state_lists_every_tile():
    on = run_both(euler_case(420, 180, [B.periodic] * 4, dense, steps=10), (420, 180), check=(3, 6))
    nt = 7 * 15
    assert skipped(on) == 0 and all(c == nt for c, _ in on[3]), on[3]
