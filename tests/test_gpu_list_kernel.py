"""
GPU: the tile-list kernel behind the one-kernel dimension-split step (classic_fused.hpp: handover_list_kernel, DESIGN.md
4.1a round 15) takes 1024 tiles per workgroup, reduces the skipped tiles' Courant maxima over the whole workgroup and
issues at most four atomics.  The grids here are the smallest at which that can go wrong: exactly one full workgroup,
one tile more than a multiple of a wavefront into a second one, partial tiles, and grids with fewer than three tiles
along a direction (every tile on the frame, nothing skipped).  Every case runs with pcl_tile_skip on and off (the run_both
pattern of test_gpu_quiet_tiles): byte-identical final states and the same (dt, Courant bits, return code) of every
step call -- a tile listed twice, left out or put into the wrong class's end of the list, or a Courant maximum lost in
the reduction, shows there.  At chosen steps the class counts na and nq (pcl_tile_list_classes) must equal those of the
host's recomputation of the skip rule from the words the list was built from (pcl_tile_words); the hooks give the
counts of the listed sets, not the list itself.
"""
import numpy as np
import pytest

import pyclaw_amd as pyclaw

import test_gpu_quiet_tiles as Q
import test_gpu_tile_handover as H
import test_gpu_tile_order as T

pytestmark = pytest.mark.gpu

B = pyclaw.BC


def tiles(mx, my):
    return (mx + 59) // 60, (my + 11) // 12


def run(mx, my, init, at, steps=16, **kw):
    seen = []
    on, off = Q.run_both(H.euler_case(mx, my, 2.0 * my / mx, init, steps=steps, **kw), T.class_hook((mx, my), at, seen))
    T.check_after(on, seen)
    return on, seen


@pytest.mark.parametrize("mx, my", [(1920, 384), (2400, 312), (427, 197)])
def test_workgroup_boundaries(mx, my):
    ntx, nty = tiles(mx, my)
    assert (ntx * nty, mx, my) in ((1024, 1920, 384), (1040, 2400, 312), (8 * 17, 427, 197))
    on, seen = run(mx, my, H.moving_blob(0.4, 0.2), {5, 9, 13})
    assert len(seen) == 3 and Q.skipped(on) > 0
    for k, na, nq, *_ in seen:
        assert na > 0 and nq > 0 and na + nq < ntx * nty, (k, na, nq)


@pytest.mark.parametrize("mx, my", [(100, 30), (60, 200)])
def test_every_tile_on_the_frame(mx, my):
    ntx, nty = tiles(mx, my)
    assert min(ntx, nty) < 3
    on, seen = run(mx, my, Q.blob, {4, 8})
    assert Q.skipped(on) == 0
    # the launches ran over a list all the same: every tile is on it
    assert len(seen) == 2 and all(na + nq == ntx * nty for _, na, nq, *_ in seen), [s[:3] for s in seen]


@pytest.mark.parametrize("u, v", [(0.8, 0.0), (0.0, 0.8)])
def test_skipped_gas_decides_courant(u, v):
    """the moving-blob state of test_gpu_tile_handover: the skipped gas carries the step's largest Courant number, so the
    maxima reduced over the workgroup (cx along x, cy along y) decide its bits"""
    mx, my, ly = 600, 240, 1.0
    on, _ = Q.run_both(H.euler_case(mx, my, ly, H.moving_blob(u, v), steps=24))
    assert Q.skipped(on) > 0
    c = np.sqrt(Q.GAMMA * 1.0 / 1.0)
    steps, _ = H.steps_of(on)
    for e in steps:
        dt = float.fromhex(e[2])
        expect = dt * (u * mx / 2.0 + v * my / ly + c * (mx / 2.0 if u else my / ly))
        assert H.courant(e) >= expect * (1 - 1e-12), (e, expect)


def test_dense_state_skips_nothing():
    on, seen = run(427, 197, Q.dense, {4, 9}, steps=12, bc=(B.reflecting, B.outflow, B.periodic, B.periodic))
    assert Q.skipped(on) == 0
    assert all(nq == 0 and na == 8 * 17 for _, na, nq, *_ in seen), [s[:3] for s in seen]


def test_skipped_tiles_without_a_maximum():
    """advection at u = v = 0: every cached maximum is zero, so the list kernel leaves both atomic maxima out; the
    step's Courant number is zero, bit for bit, with skipping on and off"""
    mx, my = 1920, 384

    def make():
        solver = pyclaw.ClawSolver2D()
        solver.rp = pyclaw.riemann.rp_advection_2d
        solver.mwaves = 1
        solver.limiters = [4]
        solver.dim_split = True
        for k in range(2):
            solver.bc_lower[k] = solver.bc_upper[k] = B.periodic
        grid = pyclaw.Grid([pyclaw.Dimension('x', 0.0, 1.0, mx), pyclaw.Dimension('y', 0.0, my / mx, my)])
        state = pyclaw.State(grid, 1)
        state.aux_global['u'] = 0.0
        state.aux_global['v'] = 0.0
        state.q[0] = 0.0
        state.q[0, 300:340, 100:130] = 1.0
        solver.cfl_max, solver.cfl_desired = 1.0, 1.0
        solver.dt_variable = False
        solver.dt_initial = 1.0 / mx
        return Q.controller(state, solver, 12 * solver.dt_initial)
    seen = []
    on, _ = Q.run_both(make, T.class_hook((mx, my), {4, 8}, seen))
    T.check_after(on, seen)
    assert Q.skipped(on) > 0 and len(seen) == 2
    steps, _ = H.steps_of(on)
    assert all(H.courant(e) == 0.0 for e in steps), steps
