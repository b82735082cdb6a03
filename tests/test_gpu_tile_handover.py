"""
GPU: the next launch's tile list is built behind the one-kernel dimension-split step, in the kernel that hands the
Courant number over (classic_fused.hpp: handover_list_kernel).  The skipped tiles' Courant number is
published by the next launch from two dt-free maxima.  Every case runs with pcl_tile_skip on and off in this process and
must give byte-identical final states and the same sequence of step calls (dt, Courant number bits and return code of
every step, every undo: the run_both pattern of test_gpu_quiet_tiles).  After every event that must drop the pending
list (an undo, a put, pcl_tile_words, a launch the source's fixed-point bound rules out, a two-pass trial step) the
one-kernel launch that follows must compute every tile (pcl_tile_skip_stats).
"""
import ctypes

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

import test_gpu_quiet_tiles as Q

pytestmark = pytest.mark.gpu

B = pyclaw.BC
GAMMA1 = Q.GAMMA1


def euler_case(mx, my, ly, init, bc=(B.periodic,) * 4, src=False, steps=20, dt_variable=False, cfl=(1.0, 0.9),
               dt0=0.2):
    """Q.euler_case on [0, 2] x [0, ly]: dx != dy unless ly = 2 my / mx"""
    def make():
        x = pyclaw.Dimension('x', 0.0, 2.0, mx)
        y = pyclaw.Dimension('y', 0.0, ly, my)
        state = pyclaw.State(pyclaw.Grid([x, y]), 5, 1)
        state.aux_global['gamma'] = Q.GAMMA
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
        return Q.controller(state, solver, steps * solver.dt_initial)
    return make


def moving_blob(u, v):
    """gas moving at (u, v) with p = 1 everywhere, a small dense blob at rest in the middle: its sound speed and speed
    are lower, so the quiet moving gas -- most of it skipped -- carries the step's largest Courant number (the computed
    tiles around a quiet region hold the same state, so they can only tie with it)"""
    def init(mx, my):
        q = Q.uniform(mx, my, (1.0, u, v, 2.5 + 0.5 * (u * u + v * v), 0.0))
        i, j = np.meshgrid(np.arange(mx), np.arange(my), indexing='ij')
        inside = (i - mx // 2) ** 2 + (j - my // 2) ** 2 < (min(mx, my) // 10) ** 2
        q[0][inside] = 3.0
        q[1][inside] = 0.0
        q[2][inside] = 0.0
        q[3][inside] = 2.5
        q[4][inside] = 1.0
        return q
    return init


def steps_of(run):
    """(log entry, (computed, skipped)) of every recorded step call, and the indices of the entries behind an undo"""
    out, after_undo, pend = [], [], False
    for e in run[2]:
        if e[0] == "undo":
            pend = True
            continue
        if e[0] in ("step", "bc_step"):
            if pend:
                after_undo.append(len(out))
            pend = False
            out.append(e)
    assert len(out) == len(run[3])
    return out, after_undo


def courant(e):
    return float.fromhex(e[3])


@pytest.mark.parametrize("u, v", [(0.8, 0.0), (0.0, 0.8)])
def test_moving_gas_decides_courant(u, v):
    mx, my, ly = 600, 240, 1.0                          # dx = 1/300, dy = 1/240
    on, _ = Q.run_both(euler_case(mx, my, ly, moving_blob(u, v), steps=24))
    assert Q.skipped(on) > 0
    # the moving gas' Courant number, dt/d (|u| + c) along the direction it moves, is larger than the other direction's
    # (u: 300 * 1.98 dt against 240 * 1.18 dt; v: 240 * 1.98 dt against 300 * 1.18 dt) and than the blob's
    c = np.sqrt(Q.GAMMA * 1.0 / 1.0)
    steps, _ = steps_of(on)
    for e in steps:
        dt = float.fromhex(e[2])
        expect = dt * (u * mx / 2.0 + v * my / ly + c * (mx / 2.0 if u else my / ly))
        assert courant(e) >= expect * (1 - 1e-12), (e, expect)


def test_rejected_step_and_retake():
    # variable dt, a first dt too large: the first step is rejected; the later steps grow dt until some is rejected
    on, _ = Q.run_both(euler_case(420, 180, 1.0, moving_blob(0.5, 0.3), bc=(B.outflow,) * 4, steps=40, dt_variable=True,
                                  cfl=(0.5, 0.45), dt0=1.0))
    steps, after_undo = steps_of(on)
    assert after_undo, on[2]
    assert Q.skipped(on) > 0
    for k in after_undo:
        assert on[3][k][1] == 0, (k, on[3])


def test_put_undo_and_tile_words_between_steps():
    mx, my = 420, 180
    events = {6: "put", 12: "undo", 18: "words", 24: "words_null"}

    def hook_factory():
        def hook(k, h, rec):
            L = _lib.lib()
            what = events.get(k)
            if what == "put":
                buf = np.empty(5 * mx * my)
                _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
                _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))      # the same bytes back: still not read-only
            elif what == "undo":
                # the step undone and taken again from here: the retake must compute every tile
                cfl = np.zeros(1)
                _lib.check(rec.orig["pcl_undo_step"](h))
                _lib.check(rec.orig["pcl_bc_step"](h, *rec.bc_args, _lib.d(cfl)))
                c, s = ctypes.c_long(), ctypes.c_long()
                _lib.check(L.pcl_tile_skip_stats(h, ctypes.byref(c), ctypes.byref(s)))
                rec.log.append(("retaken", float(cfl[0]).hex(), s.value))
            elif what in ("words", "words_null"):
                ntx, nty = ctypes.c_int(), ctypes.c_int()
                _lib.check(L.pcl_tile_words(h, None, ctypes.byref(ntx), ctypes.byref(nty)))
                if what == "words":
                    w = np.zeros(ntx.value * nty.value, dtype=np.uint32)
                    L.pcl_tile_words(h, w.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ntx), ctypes.byref(nty))
        return hook
    on, _ = Q.run_both(euler_case(mx, my, 0.9, moving_blob(0.4, 0.2), steps=30), hook_factory)
    assert Q.skipped(on) > 0
    assert [e[2] for e in on[2] if e[0] == "retaken"] == [0]
    for k, what in events.items():
        if what != "undo":
            assert on[3][k + 1][1] == 0, (what, k, on[3])
        assert on[3][k - 1][1] > 0 or k < 3, (what, k, on[3])     # skipping before the event (the case is quiet enough)


def test_source_dt_above_fixed_point_bound():
    """under the fused source a launch whose dt exceeds the fixed-point bound (2^20) computes every tile, although the
    list built behind the launch before it is pending; the launch is undone again"""
    def hook_factory():
        def hook(k, h, rec):
            if k in (5, 11):
                L = _lib.lib()
                cfl = np.zeros(1)
                bc, cs, _ = rec.bc_args
                rec.orig["pcl_bc_step"](h, bc, cs, 2.0 ** 21, _lib.d(cfl))
                c, s = ctypes.c_long(), ctypes.c_long()
                _lib.check(L.pcl_tile_skip_stats(h, ctypes.byref(c), ctypes.byref(s)))
                _lib.check(rec.orig["pcl_undo_step"](h))
                rec.log.append(("big_dt", c.value, s.value))
        return hook
    on, _ = Q.run_both(euler_case(420, 180, 1.0, moving_blob(0.4, 0.0), src=True, steps=18), hook_factory)
    big = [e for e in on[2] if e[0] == "big_dt"]
    assert len(big) == 2 and all(e[2] == 0 and e[1] > 0 for e in big), big
    assert on[3][5][1] > 0 and on[3][11][1] > 0, on[3]      # the launches in front of them did skip
    assert on[3][6][1] == 0 and on[3][12][1] == 0, on[3]    # behind the undo: every tile again
    assert Q.skipped(on) > 0


def test_auto_form_trial_steps():
    """80 steps: the default form policy runs trial steps in both forms (steps 64..71); every one-kernel launch right
    behind a two-pass step computes every tile"""
    forms = []

    def hook_factory():
        def hook(k, h, rec):
            L = _lib.lib()
            ms, n, one, two = ctypes.c_double(), ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
            _lib.check(L.pcl_step_form_stats(h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(one), ctypes.byref(two)))
            forms.append((one.value, two.value))
        return hook
    on, _ = Q.run_both(euler_case(600, 240, 1.5, moving_blob(0.6, 0.2), steps=80), hook_factory)
    forms_on = forms[:len(on[3])]
    assert Q.skipped(on) > 0
    two_pass = [k for k in range(1, len(forms_on)) if forms_on[k][1] > forms_on[k - 1][1]]
    assert two_pass, forms_on
    for k in range(1, len(forms_on)):
        if forms_on[k][0] > forms_on[k - 1][0] and forms_on[k - 1][1] > (forms_on[k - 2][1] if k >= 2 else 0):
            assert on[3][k][1] == 0, (k, on[3][k], forms_on[k - 2:k + 1])
