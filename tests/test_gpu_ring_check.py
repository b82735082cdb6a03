"""
GPU: the ring check of the one-kernel dimension-split step (classic_fused.hpp: ring_uniform).  A listed
tile that was quiet in the launch before (class Q) compares the cells of its window it does not own with one of its own
cells and, where all are equal, returns in front of the load: quiet again, nothing to store, its cached Courant maxima
published.  Every case runs three ways in this process -- pcl_tile_skip off; skip on, pcl_tile_ring off; skip on, ring
on -- and must give byte-identical final states (no sign-of-zero normalisation) and the same sequence of step calls
(dt, Courant number bits, return code, every undo).  At chosen step calls the two runs with skipping on read the class
counts, the words the launch's list was built from and pcl_tile_ring_stats: counts and words must be the same with the
ring on and off, the ring count 0 with the ring off.  Each of those reads makes the next launch compute every tile.
"""
import ctypes

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

import test_gpu_quiet_tiles as Q
import test_gpu_tile_handover as H
import test_gpu_tile_order as T

pytestmark = pytest.mark.gpu

B = pyclaw.BC
TQ_ALL = T.TQ_ALL
MODES = ((False, True), (True, False), (True, True))      # (pcl_tile_skip, pcl_tile_ring)


class Recorder(Q.Recorder):
    """Q.Recorder that also sets pcl_tile_ring once per solver handle, in front of its first step"""

    def __init__(self, skip, ring, hook=None):
        Q.Recorder.__init__(self, skip, hook)
        self.ring, self.ring_seen = ring, set()

    def __enter__(self):
        Q.Recorder.__enter__(self)
        L = _lib.lib()
        bc_step, step = L.pcl_bc_step, L.pcl_step_hyperbolic

        def first(h):
            key = h.value if hasattr(h, "value") else h
            if key not in self.ring_seen:
                self.ring_seen.add(key)
                _lib.check(L.pcl_tile_ring(h, 1 if self.ring else 0))

        def ring_bc_step(h, *args):
            first(h)
            return bc_step(h, *args)

        def ring_step(h, *args):
            first(h)
            return step(h, *args)

        L.pcl_bc_step, L.pcl_step_hyperbolic = ring_bc_step, ring_step
        return self


def ring_stats(h):
    n = ctypes.c_long(-1)
    _lib.check(_lib.lib().pcl_tile_ring_stats(h, ctypes.byref(n)))
    return n.value


def read_launch(h):
    """(ring count, na, nq, words or None) of the last launch; words: those its list was built from, None if it computed
    every tile"""
    L = _lib.lib()
    short = ring_stats(h)
    na, nq = ctypes.c_long(), ctypes.c_long()
    _lib.check(L.pcl_tile_list_classes(h, ctypes.byref(na), ctypes.byref(nq)))
    words = None
    if na.value + nq.value > 0:
        ntx, nty = ctypes.c_int(), ctypes.c_int()
        _lib.check(L.pcl_tile_words(h, None, ctypes.byref(ntx), ctypes.byref(nty)))
        words = np.zeros(ntx.value * nty.value, dtype=np.uint32)
        _lib.check(L.pcl_tile_words(h, words.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ntx), ctypes.byref(nty)))
        words = words.reshape(nty.value, ntx.value)
    return short, na.value, nq.value, words


def run3(make, at=(), extra=None):
    """make() -> Controller ready to run.  Runs the three modes; at the step calls in `at` the runs with skipping on read
    the launch (read_launch); extra(k, h, rec) runs first behind every step call.  Returns (reads of the ring-on run as
    {k: (short, na, nq, words)}, its (hash, finite, log, stats))."""
    res = []
    for skip, ring in MODES:
        reads = {}

        def hook(k, h, rec, reads=reads, skip=skip):
            if extra is not None:
                extra(k, h, rec)
            if skip and k in at:
                reads[k] = read_launch(h)
        claw = make()
        with Recorder(skip, ring, hook) as rec:
            claw.run()
            digest, fin = Q.final_bytes(claw)
        res.append((digest, fin, rec.log, rec.stats, reads))
    off, noring, on = res
    assert on[1], "non-finite state"
    assert on[2] == noring[2] == off[2], "step sequences differ"
    assert on[0] == noring[0] == off[0], "final states differ"
    assert all(s == 0 for _, s in off[3]), off[3]
    assert on[3] == noring[3], "tile counts differ between ring on and off"
    assert sorted(on[4]) == sorted(noring[4]) == sorted(k for k in at if k < len(on[3]))
    for k in on[4]:
        a, b = on[4][k], noring[4][k]
        assert b[0] == 0, (k, b[:3])                                   # ring off: nothing took the short path
        assert a[1:3] == b[1:3], (k, a[:3], b[:3])
        assert (a[3] is None) == (b[3] is None) and (a[3] is None or (a[3] == b[3]).all()), k
        assert 0 <= a[0] <= a[2], (k, a[:3])                           # only class-Q tiles can take it
    return on[4], on[:4]


def euler(mx, my, init, bc=(B.periodic,) * 4, steps=8, src=False, user_lower=None, **kw):
    """H.euler_case with dx = dy; user_lower: solver.user_bc_lower for the sides with BC.custom"""
    inner = H.euler_case(mx, my, 2.0 * my / mx, init, bc=bc, src=src, steps=steps, **kw)

    def make():
        claw = inner()
        if user_lower is not None:
            claw.solver.user_bc_lower = user_lower
        return claw
    return make


def gas(u=0.0, v=0.0):
    return (1.0, u, v, 2.5 + 0.5 * (u * u + v * v), 0.0)


# ---- one perturbed cell in moving ambient gas, 5 x 5 tiles -----------------------------------------------------------
# Tile (tx, ty) owns the cells i in [60 tx, 60 tx + 60), j in [12 ty, 12 ty + 12) and loads two more on every side.  The
# cell lies in tile (2, 2), two cells further from the target tile than the last cell the target loads: launch 0 leaves
# the target quiet (its window is uniform), and the change launch 0 writes next to the cell, one cell downstream, lies in
# the named part of the target's ring when launch 1 -- the first that runs over a list, with the target in class Q --
# reads it.  The target must then take the full path: its word of launch 1 is not TQ_ALL, ring on or off.
PLACEMENTS = {
    # name: (cell (i, j), gas velocity towards the target, target tile (tx, ty))
    "corner": ((122, 26), (-0.5, -0.5), (1, 1)),      # reaches the diagonal neighbour's corner halo alone
    "left": ((122, 30), (-0.5, 0.0), (1, 2)),         # columns 62-63 of the left neighbour
    "right": ((177, 30), (0.5, 0.0), (3, 2)),         # columns 0-1 of the right neighbour
    "below": ((150, 26), (0.0, -0.5), (2, 1)),        # rows 14-15 of the neighbour below
    "above": ((150, 33), (0.0, 0.5), (2, 3)),         # rows 0-1 of the neighbour above
}


@pytest.mark.parametrize("comp", [4, 0], ids=["tracer", "density"])
@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_one_cell_reaches_ring(place, comp):
    (i, j), (u, v), (tx, ty) = PLACEMENTS[place]
    mx, my = 300, 60

    def init(mx, my):
        q = Q.uniform(mx, my, gas(u, v))
        q[comp, i, j] += 0.5
        return q
    make = euler(mx, my, init, steps=4)
    # the words of launch 0 are what launch 1's list was built from, those of launch 1 what launch 2's was: two runs,
    # since a read makes the next launch compute every tile
    first, _ = run3(make, at={1})
    second, _ = run3(make, at={2})
    short1, na1, nq1, w0 = first[1]
    _, _, _, w1 = second[2]
    assert w0 is not None and w1 is not None
    assert w0[ty, tx] == TQ_ALL, (place, comp, w0)               # quiet in launch 0, so class Q in launch 1
    listed, act = T.host_classes(w0.ravel(), 5, 5, mx, my)
    assert listed[ty, tx] and not act[ty, tx]
    assert w1[ty, tx] != TQ_ALL, (place, comp, w1)               # the change reached its ring: it computed
    assert w0[2, 2] != TQ_ALL and w1[2, 2] != TQ_ALL
    assert 0 < short1 < nq1, (short1, na1, nq1)                  # the other class-Q tiles of launch 1 were quiet again
    assert short1 == int((listed & ~act & (w1 == TQ_ALL)).sum()), (short1, w0, w1)


# ---- the round-7 case ------------------------------------------------------------------------------------------------
def test_advected_block():
    """a block of ones in zeros advected at Courant number 1 moves exactly one cell per step: the tiles it has left are
    quiet again and take the short path"""
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
        return Q.controller(state, solver, 60 * solver.dt_initial)
    reads, on = run3(make, at={20, 40, 58})
    assert len(reads) == 3 and all(r[0] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    assert Q.skipped(on) > 0


# ---- frame tiles -----------------------------------------------------------------------------------------------------
def frame_counts(reads, k):
    short, na, nq, words = reads[k]
    assert words is not None, k
    return short, na, nq, words


def test_frame_reflecting_zero_normal_momentum():
    """gas moving along a reflecting wall: the mirrored ghost cells hold -0 normal momentum, equal under ==.  Nothing
    ever computes: the 16 frame tiles of the 5 x 5 are the list, all class Q, all settled by the ring"""
    reads, _ = run3(euler(300, 60, lambda mx, my: Q.uniform(mx, my, gas(0.4, 0.0)),
                          bc=(B.periodic, B.periodic, B.reflecting, B.outflow), steps=8), at={2, 5})
    for k in (2, 5):
        assert frame_counts(reads, k)[:3] == (16, 0, 16), reads[k][:3]


def test_frame_reflecting_normal_momentum():
    """gas moving into a reflecting wall: the mirrored ghost cells differ, the bottom tiles compute in every launch and
    never reach the ring check; the other listed tiles are settled by it"""
    reads, _ = run3(euler(300, 60, lambda mx, my: Q.uniform(mx, my, gas(0.0, -0.3)),
                          bc=(B.periodic, B.periodic, B.reflecting, B.outflow), steps=8), at={2})
    short, na, nq, words = frame_counts(reads, 2)
    assert (words[0] != TQ_ALL).all() and (words[1:] == TQ_ALL).all(), words
    assert na == 5 and short == nq > 0, (short, na, nq)          # the wall's wave is rows away from the tiles above


@pytest.mark.parametrize("same", [True, False], ids=["ambient", "other"])
def test_frame_constant_inflow(same):
    state = gas(0.4, 0.0)
    inflow = state if same else (1.2, 0.5, 0.0, 3.0, 0.0)
    reads, _ = run3(euler(300, 60, lambda mx, my: Q.uniform(mx, my, state),
                          bc=(B.custom, B.outflow, B.outflow, B.outflow), steps=8,
                          user_lower=pyclaw.ConstantStateBC(list(inflow))), at={2})
    short, na, nq, words = frame_counts(reads, 2)
    if same:
        assert (short, na, nq) == (16, 0, 16), (short, na, nq)
    else:
        assert (words[:, 0] != TQ_ALL).all() and (words[:, 1:] == TQ_ALL).all(), words
        assert na == 5 and short == nq > 0, (short, na, nq)      # the inflow's wave is columns away from the next tiles


@pytest.mark.parametrize("bc", [(B.outflow,) * 4, (B.periodic,) * 4], ids=["outflow", "periodic"])
def test_frame_uniform(bc):
    reads, _ = run3(euler(300, 60, lambda mx, my: Q.uniform(mx, my, gas(0.3, 0.2)), bc=bc, steps=8), at={2, 5})
    for k in (2, 5):
        assert frame_counts(reads, k)[:3] == (16, 0, 16), reads[k][:3]


def test_frame_blob_all_sides():
    """a blob in the middle sends waves to every side (the sides of test_gpu_quiet_tiles.test_sides)"""
    for bc in ((B.reflecting,) * 4, (B.reflecting, B.outflow, B.periodic, B.periodic)):
        reads, on = run3(euler(300, 60, Q.blob, bc=bc, steps=30), at={2, 12, 26})
        assert reads[2][0] > 0, reads[2][:3]


def test_host_filled_ghost_cells():
    """a Python boundary function fills the ghost cells on the host in front of every step: that upload is no read-only
    call, so every launch computes every tile -- no list, no class Q, no ring check -- and the three runs agree"""
    state = gas(0.4, 0.0)

    def host_bc(st, dim, t, qbc, mbc):
        if dim.nstart == 0:
            for m in range(5):
                qbc[m, :mbc, ...] = state[m]
    reads, on = run3(euler(300, 60, Q.blob, bc=(B.custom, B.outflow, B.outflow, B.outflow), steps=12,
                           user_lower=host_bc), at={2, 7})
    assert len(reads) == 2
    for k, (short, na, nq, words) in reads.items():
        assert (short, na, nq) == (0, 0, 0) and words is None, (k, short, na, nq)
    assert Q.skipped(on) == 0, on[3]


def test_signed_zero_patches():
    """the -0 momentum patches of the quiet-tile tests, source off: +0 and -0 compare equal, a patch border is no jump,
    and the bytes still come out as they went in"""
    reads, on = run3(euler(900, 320, Q.big_patchwork, bc=(B.outflow, B.reflecting, B.periodic, B.periodic), steps=10),
                     at={2, 6})
    assert all(r[0] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    assert Q.skipped(on) > 0


# ---- partial tiles, small grids ----------------------------------------------------------------------------------------
def test_partial_tiles_427_197():
    """427 x 197: partial tiles at both upper edges, their cells past the array clamped"""
    for bc in ((B.outflow,) * 4, (B.periodic, B.periodic, B.reflecting, B.outflow)):
        reads, on = run3(euler(427, 197, Q.blob, bc=bc, steps=20), at={2, 9, 17})
        assert all(r[0] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
        assert Q.skipped(on) > 0


@pytest.mark.parametrize("mx, my", [(100, 60), (300, 20), (50, 10), (130, 20)])
def test_every_tile_on_the_frame(mx, my):
    """ntx or nty below 3: no tile is off the frame, every launch lists them all"""
    def init(mx, my):
        q = Q.uniform(mx, my, gas(0.3, 0.0))
        q[0, 3, 3] += 0.5
        return q
    reads, on = run3(euler(mx, my, init, bc=(B.outflow, B.outflow, B.reflecting, B.outflow), steps=6), at={2, 4})
    assert Q.skipped(on) == 0
    ntiles = ((mx + 59) // 60) * ((my + 11) // 12)
    assert all(r[1] + r[2] == ntiles for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    if ntiles > 4:
        assert reads[2][0] > 0, reads[2][:3]                     # tiles far from the cell


# ---- shock-bubble ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_src", [False, True])
def test_shockbubble(with_src):
    """960 x 480, 60 steps; the short path is not taken under the fused source"""
    reads, on = run3(T.shockbubble(with_src), at={10, 25, 40, 55})
    assert sum(1 for e in on[2] if e[0] != "undo") >= 60, len(on[2])
    assert len(reads) == 4 and all(r[2] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    if with_src:
        assert all(r[0] == 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    else:
        assert all(r[0] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    assert Q.skipped(on) > 0


# ---- protocol --------------------------------------------------------------------------------------------------------
def test_rejected_and_retaken_step():
    """behind an undo the retaken step computes every tile: no list, no short path"""
    counts = []

    def extra(k, h, rec):
        if rec.skip and len(rec.log) >= 2 and rec.log[-2][0] == "undo":
            counts.append((k, rec.ring, ring_stats(h), rec.stats[-1]))
    reads, on = run3(euler(420, 180, H.moving_blob(0.5, 0.3), bc=(B.outflow,) * 4, steps=40, dt_variable=True,
                           cfl=(0.5, 0.45), dt0=1.0), at={10, 25}, extra=extra)
    assert any(e[0] == "undo" for e in on[2]), on[2]
    assert counts and all(c[2] == 0 and c[3][1] == 0 for c in counts), counts
    assert any(r[0] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}


def test_put_q_and_undo_between_steps():
    """pcl_put_q between two steps, and a step undone and taken again: the launch that follows computes every tile"""
    mx, my = 420, 180
    seen = []

    def extra(k, h, rec):
        L = _lib.lib()
        if k == 6:
            buf = np.empty(5 * mx * my)
            _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
            _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))
        elif k == 12:
            cfl = np.zeros(1)
            _lib.check(rec.orig["pcl_undo_step"](h))
            _lib.check(rec.orig["pcl_bc_step"](h, *rec.bc_args, _lib.d(cfl)))
            c, s = ctypes.c_long(), ctypes.c_long()
            _lib.check(L.pcl_tile_skip_stats(h, ctypes.byref(c), ctypes.byref(s)))
            if rec.skip:
                seen.append(("retaken", rec.ring, s.value, ring_stats(h)))
        elif k == 7 and rec.skip:
            seen.append(("after put", rec.ring, rec.stats[-1][1], ring_stats(h)))
    reads, on = run3(euler(mx, my, H.moving_blob(0.4, 0.2), steps=24), at={4, 10, 18}, extra=extra)
    assert len(seen) == 4 and all(e[2] == 0 and e[3] == 0 for e in seen), seen
    assert all(r[0] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    assert Q.skipped(on) > 0


def test_auto_form_trial_window():
    """80 steps: the default form policy runs its trial steps in both forms"""
    reads, on = run3(euler(600, 240, H.moving_blob(0.6, 0.2), steps=80), at={30, 60, 78})
    assert any(r[0] > 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    assert Q.skipped(on) > 0


def test_dense_state():
    """nothing is quiet: no tile is class Q, nothing takes the short path"""
    reads, on = run3(euler(420, 180, Q.dense, steps=10), at={2, 5, 8})
    assert all(r[0] == 0 and r[2] == 0 for r in reads.values()), {k: r[:3] for k, r in reads.items()}
    assert Q.skipped(on) == 0
