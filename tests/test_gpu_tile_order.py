"""
GPU: a list launch of the one-kernel dimension-split step runs its listed tiles in two classes (classic_fused.hpp:
handover_list_kernel): class A, tiles that computed something in the launch before, first; class Q,
tiles that were quiet there and are listed for a neighbour or the frame, behind them.  A class-Q tile that is quiet
again does not store (its owned cells in the output buffer hold the result already), except under the fused source.
Every case runs with pcl_tile_skip on and off (the run_both pattern of test_gpu_quiet_tiles): byte-identical final
states, the same sequence of step calls.  At chosen steps the two class counts (pcl_tile_list_classes) must match a
host recomputation from the words the launch's list was built from (pcl_tile_words), and the launch after the call
must compute every tile.
"""
import ctypes

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

import test_gpu_quiet_tiles as Q
import test_gpu_tile_handover as H

pytestmark = pytest.mark.gpu

B = pyclaw.BC
TQ_ALL = 0x01010101


def host_classes(words, ntx, nty, mx, my):
    """(listed mask, class-A mask) of the tile grid: a tile off the frame with a quiet 3 x 3 neighbourhood is skipped,
    every other one listed; class A if its own word is not TQ_ALL"""
    w = words.reshape(nty, ntx)
    quiet = w == TQ_ALL
    skip = np.zeros_like(quiet)
    for ty in range(nty):
        for tx in range(ntx):
            x0, y0 = 60 * tx, 12 * ty            # window origin, counted from the first interior cell minus 2
            if x0 < 2 or y0 < 2 or x0 + 64 > mx + 2 or y0 + 16 > my + 2:
                continue
            skip[ty, tx] = quiet[ty - 1:ty + 2, tx - 1:tx + 2].all()
    return ~skip, ~skip & ~quiet


def class_hook(shape, at, seen, before=None):
    """hook for Q.run_both: at the step calls in `at` read the class counts and the words, check the counts against the
    host and keep (k, na, nq, words, listed, class A) in seen; before(k, h, rec) runs first at every step"""
    def factory():
        def hook(k, h, rec):
            if before is not None:
                before(k, h, rec)
            if k not in at or not rec.skip:
                return
            L = _lib.lib()
            c, s = ctypes.c_long(), ctypes.c_long()
            _lib.check(L.pcl_tile_skip_stats(h, ctypes.byref(c), ctypes.byref(s)))
            na, nq = ctypes.c_long(), ctypes.c_long()
            _lib.check(L.pcl_tile_list_classes(h, ctypes.byref(na), ctypes.byref(nq)))
            if na.value + nq.value == 0:
                return                                   # the launch computed every tile (no list)
            assert na.value + nq.value == c.value, (k, na.value, nq.value, c.value)
            ntx, nty = ctypes.c_int(), ctypes.c_int()
            _lib.check(L.pcl_tile_words(h, None, ctypes.byref(ntx), ctypes.byref(nty)))
            words = np.zeros(ntx.value * nty.value, dtype=np.uint32)
            _lib.check(L.pcl_tile_words(h, words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ntx), ctypes.byref(nty)))
            listed, act = host_classes(words, ntx.value, nty.value, *shape)
            assert (na.value, nq.value) == (int(act.sum()), int((listed & ~act).sum())), (k, na.value, nq.value)
            seen.append((k, na.value, nq.value, words.reshape(nty.value, ntx.value), listed, act))
        return hook
    return factory


def check_after(on, seen):
    """the launch right behind a class read computes every tile (the read is not read-only)"""
    for k, *_ in seen:
        if k + 1 < len(on[3]):
            assert on[3][k + 1][1] == 0, (k, on[3][k + 1])


def shockbubble(with_src, tfinal=0.04):
    def make():
        claw = problems.shockbubble(pyclaw, mx=960, my=480, tfinal=tfinal, device_callbacks=True, with_src=with_src,
                                    dt_initial=0.005 * 160 / 960, run=False)
        claw.keep_copy = False
        claw.output_format = None
        return claw
    return make


def every_launch(make, shape, lo, hi):
    """Two runs that read the classes at every other step call in [lo, hi), the second one offset by one.  Together
    they give the words of every launch in the window (a tile's word is a function of the state, whichever launches
    skipped), and each launch in it ran over a list in one of them.  Returns ({launch: words}, {launch: class-Q mask})."""
    seen = []
    for first in (lo, lo + 1):
        at = set(range(first, hi, 2))
        on, _ = Q.run_both(make, class_hook(shape, at, seen))
        check_after(on, [e for e in seen if e[0] in at])
        assert Q.skipped(on) > 0
    words = {k - 1: w for k, _, _, w, _, _ in seen}          # the words a list was built from: launch k - 1's
    class_q = {k: listed & ~act for k, _, _, _, listed, act in seen}
    assert len(class_q) > (hi - lo) * 3 // 4, sorted(class_q)
    return words, class_q


def q_turns_active(words, class_q):
    """launches in which some class-Q tile computed something (and stored it)"""
    return [n for n in class_q if n in words and (class_q[n] & (words[n] != TQ_ALL)).any()]


def quiet_again(words, class_q):
    """launches n in which some tile that was active in n - 2 and quiet in n - 1 (so class Q in n) is quiet again: it
    skipped its store"""
    return [n for n in class_q if n - 2 in words and n in words and
            (class_q[n] & (words[n - 2] != TQ_ALL) & (words[n] == TQ_ALL)).any()]


def test_shockbubble_classes():
    words, class_q = every_launch(shockbubble(False, tfinal=0.06), (960, 480), 6, 62)
    assert q_turns_active(words, class_q)


def test_advected_block():
    """A block of ones in zeros advected at Courant number 1 (u = 1, v = 0, dt = dx = 2^-9, periodic) moves exactly one
    cell per step, so the tiles it leaves are quiet again, bit for bit: class Q behind it skips its stores, class Q in
    front of it turns active (the window ends before the form trials of step 64)"""
    mx, my = 512, 192

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
        state.aux_global['u'] = 1.0
        state.aux_global['v'] = 0.0
        state.q[0] = 0.0
        state.q[0, 30:70, 60:130] = 1.0
        solver.cfl_max, solver.cfl_desired = 1.0, 1.0
        solver.dt_variable = False
        solver.dt_initial = 1.0 / mx
        return Q.controller(state, solver, 70 * solver.dt_initial)
    words, class_q = every_launch(make, (mx, my), 4, 62)
    assert q_turns_active(words, class_q)
    assert quiet_again(words, class_q)


def test_fused_source_keeps_stores():
    seen = []
    on, _ = Q.run_both(shockbubble(True), class_hook((960, 480), {25, 40}, seen))
    assert len(seen) == 2 and all(na > 0 and nq > 0 for _, na, nq, *_ in seen), [s[:3] for s in seen]
    check_after(on, seen)
    assert Q.skipped(on) > 0


def test_moving_blob():
    """gas moving at (0.6, 0.3) over a blob at rest: the waves it sends out reach tiles that were quiet"""
    mx, my = 600, 240
    seen = []
    on, _ = Q.run_both(H.euler_case(mx, my, 1.0, H.moving_blob(0.6, 0.3), steps=40), class_hook((mx, my), {8, 20, 33},
                                                                                                      seen))
    assert len(seen) == 3 and all(nq > 0 for _, _, nq, *_ in seen), [s[:3] for s in seen]
    check_after(on, seen)
    assert Q.skipped(on) > 0


def test_rejected_and_retaken_steps():
    mx, my = 420, 180
    seen = []
    on, _ = Q.run_both(H.euler_case(mx, my, 1.0, H.moving_blob(0.5, 0.3), bc=(B.outflow,) * 4, steps=40,
                                    dt_variable=True, cfl=(0.5, 0.45), dt0=1.0), class_hook((mx, my), {10, 25}, seen))
    _, after_undo = H.steps_of(on)
    assert after_undo, on[2]
    for k in after_undo:
        assert on[3][k][1] == 0, (k, on[3])
    check_after(on, seen)
    assert len(seen) == 2 and Q.skipped(on) > 0


def test_put_q_between_steps():
    mx, my = 420, 180

    def put(k, h, rec):
        if k in (6, 14):
            L = _lib.lib()
            buf = np.empty(5 * mx * my)
            _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
            a = buf.reshape(my, mx, 5)
            a[30 + k, 40 + 3 * k, 0] += 0.25             # a disturbance where the gas was quiet
            _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))
    seen = []
    on, _ = Q.run_both(H.euler_case(mx, my, 0.9, H.moving_blob(0.4, 0.2), steps=30),
                       class_hook((mx, my), {10, 22}, seen, before=put))
    assert on[3][7][1] == 0 and on[3][15][1] == 0, on[3]
    check_after(on, seen)
    assert len(seen) == 2 and Q.skipped(on) > 0
