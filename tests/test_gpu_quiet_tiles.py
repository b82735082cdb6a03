"""
GPU: quiet-tile skipping of the one-kernel dimension-split step (classic_fused.hpp) changes nothing.
Every case runs twice in this process, with pcl_tile_skip on and off, and must give byte-identical final states (no
sign-of-zero normalisation) and the same sequence of steps: dt, Courant number and return code of every step call,
every undo (rejected step).  Where the case has tiles off the frame that stay quiet, the run with skipping on must
have skipped some (pcl_tile_skip_stats after every step); the dense state must skip none.
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


class Recorder:
    """Wraps the step entry points of the library object the solvers call through: sets pcl_tile_skip once per solver
    handle before its first step, records every step call and the tile counts after it, and runs the case's hook
    (hook(call_index, handle, recorder)) behind each step."""
    NAMES = ("pcl_bc_step", "pcl_step_hyperbolic", "pcl_undo_step")

    def __init__(self, skip, hook=None):
        self.skip, self.hook = skip, hook
        self.log, self.stats, self.seen = [], [], set()

    def __enter__(self):
        L = _lib.lib()
        self.orig = {n: getattr(L, n) for n in self.NAMES}

        def stats(h):
            c, s = ctypes.c_long(), ctypes.c_long()
            _lib.check(L.pcl_tile_skip_stats(h, ctypes.byref(c), ctypes.byref(s)))
            return c.value, s.value

        def first(h):
            key = h.value if hasattr(h, "value") else h
            if key not in self.seen:
                self.seen.add(key)
                _lib.check(L.pcl_tile_skip(h, 1 if self.skip else 0))

        def bc_step(h, bc, cs, dt, cfl):
            first(h)
            self.bc_args = (bc, cs, dt)
            rc = self.orig["pcl_bc_step"](h, bc, cs, dt, cfl)
            self.after("bc_step", h, rc, dt, cfl, stats)
            return rc

        def step(h, dt, cfl):
            first(h)
            rc = self.orig["pcl_step_hyperbolic"](h, dt, cfl)
            self.after("step", h, rc, dt, cfl, stats)
            return rc

        def undo(h):
            rc = self.orig["pcl_undo_step"](h)
            self.log.append(("undo", rc))
            return rc

        L.pcl_bc_step, L.pcl_step_hyperbolic, L.pcl_undo_step = bc_step, step, undo
        return self

    def after(self, tag, h, rc, dt, cfl, stats):
        self.log.append((tag, rc, float(dt).hex(), float(cfl[0]).hex()))
        self.stats.append(stats(h))
        if self.hook is not None:
            self.hook(len(self.stats) - 1, h, self)

    def __exit__(self, *exc):
        L = _lib.lib()
        for n, f in self.orig.items():
            setattr(L, n, f)
        return False


def final_bytes(claw):
    claw.solver.teardown()
    q = np.ascontiguousarray(claw.solution.state.q)
    return hashlib.sha256(q.tobytes()).hexdigest(), bool(np.isfinite(q).all())


def run_both(make, hook_factory=None):
    """make() -> Controller ready to run; returns (on, off) = (hash, finite, log, stats) of each"""
    res = []
    for skip in (True, False):
        claw = make()
        with Recorder(skip, hook_factory() if hook_factory else None) as rec:
            claw.run()
            h, fin = final_bytes(claw)
        res.append((h, fin, rec.log, rec.stats))
    on, off = res
    assert on[1], "non-finite state"
    assert on[2] == off[2], "step sequences differ"
    assert on[0] == off[0], "final states differ"
    assert len(on[3]) >= 2
    assert all(s == 0 for _, s in off[3]), off[3]
    return on, off


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


def euler_case(mx, my, bc, init, src=False, steps=20, dt_variable=False, cfl=(1.0, 0.9), dt0=0.2):
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
        solver.cfl_max, solver.cfl_desired = cfl
        solver.dt_variable = dt_variable
        solver.dt_initial = dt0 / max(mx, my)
        for k in range(2):
            solver.bc_lower[k], solver.bc_upper[k] = bc[2 * k], bc[2 * k + 1]
            solver.aux_bc_lower[k] = solver.aux_bc_upper[k] = pyclaw.BC.outflow
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


def one_cell(mx, my):
    q = uniform(mx, my)
    q[0, mx // 2, my // 2] = 1.5
    q[3, mx // 2, my // 2] = 4.0
    return q


def big_patchwork(mx, my):
    """constant patches of 300 x 80 cells (room for a quiet 3 x 3 block of tiles) with momenta +0 in some, -0 in others
    (under the fused source a -0 momentum makes the cell no fixed point of the source: those tiles must be computed)"""
    states = np.array([[1.0, 0.0, 0.0, 2.5, 0.0], [1.0, -0.0, 0.0, 2.5, 0.0], [1.0, 0.0, -0.0, 2.5, 0.0],
                       [2.0, 0.3, 0.0, 6.0, 0.25]])
    i, j = np.meshgrid(np.arange(mx), np.arange(my), indexing='ij')
    k = ((i // 300) + (j // 80) * 3) % len(states)
    return np.moveaxis(states[k], -1, 0).copy()


def dense(mx, my):
    rng = np.random.default_rng(3)
    q = np.empty((5, mx, my))
    q[0] = 1.0 + 0.1 * rng.random((mx, my))
    q[1] = 0.1 * rng.random((mx, my))
    q[2] = 0.05 * rng.random((mx, my))
    q[3] = 2.5 + 0.1 * rng.random((mx, my))
    q[4] = rng.random((mx, my))
    return q


B = pyclaw.BC


@pytest.mark.parametrize("with_src", [False, True])
def test_shockbubble(with_src):
    def make():
        claw = problems.shockbubble(pyclaw, mx=960, my=480, tfinal=0.04, device_callbacks=True, with_src=with_src,
                                    dt_initial=0.005 * 160 / 960, run=False)
        claw.keep_copy = False
        claw.output_format = None
        return claw
    on, off = run_both(make)
    assert sum(1 for e in on[2] if e[0] != "undo") >= 60, len(on[2])
    assert any(e[0] == "undo" for e in on[2])        # the app's first step is rejected
    assert skipped(on) > 0


def test_single_cell_grows():
    on, _ = run_both(euler_case(600, 240, [B.periodic] * 4, one_cell, steps=40))
    comp = [c for c, _ in on[3]]
    assert skipped(on) > 0
    # the active region grows: from the third step on every step computes at least as many tiles as the one before it,
    # and more at the end than at the start
    assert all(b >= a for a, b in zip(comp[2:], comp[3:])), comp
    assert comp[-1] > comp[2], comp


def test_patchwork_signed_zeros_src():
    on, _ = run_both(euler_case(900, 320, [B.outflow, B.reflecting, B.periodic, B.periodic], big_patchwork, src=True,
                                steps=12))
    assert skipped(on) > 0


@pytest.mark.parametrize("bc", [[B.periodic] * 4, [B.reflecting] * 4, [B.outflow] * 4,
                                [B.reflecting, B.outflow, B.periodic, B.periodic]])
def test_sides(bc):
    on, _ = run_both(euler_case(420, 180, bc, blob, steps=25))
    assert skipped(on) > 0


def test_rejected_and_retaken_steps():
    # variable dt, a first dt too large (Courant number ~0.6 > 0.5): the first step is rejected and retaken
    on, _ = run_both(euler_case(420, 180, [B.outflow] * 4, blob, steps=40, dt_variable=True, cfl=(0.5, 0.45), dt0=1.0))
    assert any(e[0] == "undo" for e in on[2]), on[2]
    assert skipped(on) > 0


def test_put_q_between_steps():
    def hook_factory():
        def hook(k, h, rec):
            if k in (8, 15):
                # one cell of the quiet gas far from the blob changes on the device between two steps
                L = _lib.lib()
                mx, my = 420, 180
                buf = np.empty(5 * mx * my)
                _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
                a = buf.reshape(my, mx, 5)
                a[20 + k, 30 + 2 * k, 0] += 0.25
                _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))
        return hook
    on, _ = run_both(euler_case(420, 180, [B.periodic] * 4, blob, steps=30), hook_factory)
    assert skipped(on) > 0
    # the steps right behind the put compute every tile
    assert on[3][9][1] == 0 and on[3][16][1] == 0, on[3]


def test_fuse_source_toggle():
    """the cfl == cfl_max path of ClawSolver.step, driven from here: undo, the step again without the fused source, the
    source back on"""
    def hook_factory():
        def hook(k, h, rec):
            if k in (6, 14):
                L = _lib.lib()
                cfl = np.zeros(1)
                _lib.check(rec.orig["pcl_undo_step"](h))
                _lib.check(L.pcl_fuse_source(h, 0, None, 0))
                _lib.check(rec.orig["pcl_bc_step"](h, *rec.bc_args, _lib.d(cfl)))
                _lib.check(L.pcl_fuse_source(h, 1, _lib.d(np.array([GAMMA1, 2.0])), 2))
                rec.log.append(("retaken", float(cfl[0]).hex()))
        return hook
    on, _ = run_both(euler_case(420, 180, [B.periodic] * 4, blob, src=True, steps=25), hook_factory)
    assert sum(1 for e in on[2] if e[0] == "retaken") == 2
    assert skipped(on) > 0


def test_auto_form_past_trial_window():
    # 80 steps: the default form policy runs its trial steps (64..71) in both forms
    on, _ = run_both(euler_case(600, 240, [B.periodic] * 4, blob, steps=80))
    assert skipped(on) > 0


def test_dense_state_skips_nothing():
    on, _ = run_both(euler_case(420, 180, [B.periodic] * 4, dense, steps=10))
    assert skipped(on) == 0


def test_acoustics():
    def make():
        claw = problems.acoustics2D(pyclaw, mx=480, my=240, tfinal=0.03, nout=1, dim_split=1, run=False)
        claw.keep_copy = False
        claw.output_format = None
        return claw
    run_both(make)


def test_shallow_water():
    def make():
        solver = pyclaw.ClawSolver2D()
        solver.rp = pyclaw.riemann.rp_shallow_2d
        solver.mwaves = 3
        solver.limiters = [4, 4, 4]
        solver.dim_split = True
        for k in range(2):
            solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.outflow
        grid = pyclaw.Grid([pyclaw.Dimension('x', -2.5, 2.5, 480), pyclaw.Dimension('y', -2.5, 2.5, 240)])
        state = pyclaw.State(grid, 3)
        state.aux_global['g'] = 1.0
        X, Y = grid.c_center
        state.q[0] = 2.0 * (np.sqrt(X ** 2 + Y ** 2) <= 0.5) + 1.0 * (np.sqrt(X ** 2 + Y ** 2) > 0.5)
        state.q[1:] = 0.0
        solver.dt_initial = 1e-3
        return controller(state, solver, 0.1)
    on, _ = run_both(make)
    assert skipped(on) > 0
