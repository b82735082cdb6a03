"""
GPU: row reuse in the x sweeps of the one-kernel dimension-split step (classic_fused.hpp).  A
wavefront does not compute an x sweep whose row -- every component, all 64 columns of the tile's window -- holds the same
bits as the row it swept before: it takes that row's shortcut or copies that row's result.  Every case runs twice in
this process, pcl_tile_rowreuse off and on (tile skipping and the ring check at their defaults), and must give
byte-identical final states (no sign-of-zero normalisation), the same sequence of step calls (dt, Courant number bits,
return code, every undo), the same tile counts behind every step call and, at chosen step calls, the same class counts
and quiet words.  Where the count can be recomputed on the host (tests/test_row_reuse_cpu.py: the first launch of a run
computes every tile of the initial state) pcl_tile_rowreuse_stats must equal it; with the switch off it is 0.

The tile subsets of a decomposed block (unbooked launches: the switch reaches them, the counter does not) run in one
process on a block whose eight neighbours are itself, as in tests/test_gpu_halo.py: test_decomposed_block_tile_subsets.
"""
import ctypes

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems
from oracle import oracle as O

import test_gpu_quiet_tiles as Q
import test_gpu_ring_check as R
import test_gpu_tile_handover as H
import test_row_reuse_cpu as HOST

pytestmark = pytest.mark.gpu

B = pyclaw.BC
BCNAME = {B.periodic: 'periodic', B.outflow: 'outflow', B.reflecting: 'reflecting', B.custom: 'const'}
PER = (B.periodic,) * 4
planar = HOST.planar


class Recorder(Q.Recorder):
    """Q.Recorder (skipping on) that also sets pcl_tile_rowreuse once per solver handle, in front of its first step"""

    def __init__(self, reuse, hook=None):
        Q.Recorder.__init__(self, True, hook)
        self.reuse, self.reuse_seen = reuse, set()

    def __enter__(self):
        Q.Recorder.__enter__(self)
        L = _lib.lib()
        bc_step, step = L.pcl_bc_step, L.pcl_step_hyperbolic

        def first(h):
            key = h.value if hasattr(h, "value") else h
            if key not in self.reuse_seen:
                self.reuse_seen.add(key)
                _lib.check(L.pcl_tile_rowreuse(h, 1 if self.reuse else 0))

        def reuse_bc_step(h, *args):
            first(h)
            return bc_step(h, *args)

        def reuse_step(h, *args):
            first(h)
            return step(h, *args)

        L.pcl_bc_step, L.pcl_step_hyperbolic = reuse_bc_step, reuse_step
        return self


def reuse_stats(h):
    n = ctypes.c_long(-1)
    _lib.check(_lib.lib().pcl_tile_rowreuse_stats(h, ctypes.byref(n)))
    return n.value


def run2(make, at=(0, 3), extra=None):
    """make() -> Controller ready to run.  Runs with the switch off, then on; behind the step calls in `at` both runs
    read (sweeps reused, ring count, na, nq, words or None) of the launch (each read makes the next launch compute every
    tile); extra(k, h, rec) runs first behind every step call.  Returns ({k: sweeps reused} of the run with the switch
    on, its (hash, finite, log, stats))."""
    res = []
    for reuse in (False, True):
        reads = {}

        def hook(k, h, rec, reads=reads):
            if extra is not None:
                extra(k, h, rec)
            if k in at:
                reads[k] = (reuse_stats(h),) + R.read_launch(h)
        claw = make()
        with Recorder(reuse, hook) as rec:
            claw.run()
            digest, fin = Q.final_bytes(claw)
        res.append((digest, fin, rec.log, rec.stats, reads))
    off, on = res
    assert on[1], "non-finite state"
    assert on[2] == off[2], "step sequences differ"
    assert on[0] == off[0], "final states differ"
    assert on[3] == off[3], "tile counts differ"
    assert sorted(on[4]) == sorted(off[4]) == sorted(k for k in at if k < len(on[3])), (sorted(on[4]), len(on[3]))
    for k in on[4]:
        a, b = on[4][k], off[4][k]
        print("step call %d: sweeps reused %d (switch off %d), ring %d, na %d, nq %d" % ((k, a[0], b[0]) + a[1:4]))
        assert b[0] == 0, (k, b[:4])                                   # switch off: nothing reused
        assert a[0] >= 0 and a[1:4] == b[1:4], (k, a[:4], b[:4])       # ring count, na, nq
        assert (a[4] is None) == (b[4] is None) and (a[4] is None or (a[4] == b[4]).all()), k
    return {k: v[0] for k, v in on[4].items()}, on[:4]


def euler(mx, my, init, bc=PER, steps=4, src=False, const=None, **kw):
    return R.euler(mx, my, init, bc=bc, steps=steps, src=src,
                   user_lower=None if const is None else pyclaw.ConstantStateBC(list(const)), **kw)


def host_count(q, bc=PER, const=None, bitwise=True):
    return HOST.reuse_count(HOST.fill_ghosts(q, tuple(BCNAME[b] for b in bc), const), bitwise)


def first_launch(mx, my, q, bc=PER, const=None, steps=4, **kw):
    """runs q off / on; returns (sweeps reused by the first launch, its host recomputation)"""
    reads, on = run2(euler(mx, my, lambda *_: q.copy(), bc=bc, steps=steps, const=const, **kw))
    assert on[3][0] == (HOST_TILES(mx, my), 0), on[3][0]              # one kernel, every tile
    return reads[0], host_count(q, bc, const)


def HOST_TILES(mx, my):
    return ((mx + 59) // 60) * ((my + 11) // 12)


# ---- planar front ----------------------------------------------------------------------------------------------------
def test_planar_front_counted():
    """120 x 48, 2 x 4 full tiles, periodic: every row of every tile holds the jumps and computes; every wavefront reuses
    three of its four sweeps"""
    got, host = first_launch(120, 48, planar(120, 48))
    assert host == 96 and got == 96, (got, host)


def test_planar_front_against_the_oracle(coracle):
    """the planar state's first step, with the switch on, equals the oracle's dimension-split step bit for bit"""
    mx, my, mbc = 120, 48, 2
    q = planar(mx, my)
    claw = euler(mx, my, lambda *_: q.copy(), steps=1)()
    with Recorder(True) as rec:
        claw.run()
        n = len([e for e in rec.log if e[0] != "undo"])
        claw.solver.teardown()
    assert n == 1, rec.log
    out = np.ascontiguousarray(claw.solution.state.q)
    qbc = np.asfortranarray(HOST.fill_ghosts(q, ('periodic',) * 4))
    ref = qbc.copy("F")
    par = np.array([Q.GAMMA, Q.GAMMA1])
    mth = np.array([4, 4, 4, 4, 2], dtype=np.int32)
    method = np.array([1, 2, -1, 0, 0, 0, 0], dtype=np.int32)
    dx, dy = (2.0 - 0.0) / float(mx), (2.0 * my / mx - 0.0) / float(my)          # Dimension.d of R.euler's grid
    dt = 0.2 / max(mx, my)
    coracle.step2ds(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, qbc, ref, None, dx, dy, dt, method, mth, 1)
    coracle.step2ds(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, ref, ref, None, dx, dy, dt, method, mth, 2)
    want = ref[:, mbc:-mbc, mbc:-mbc]
    assert (want != q).any()
    assert out.tobytes() == np.ascontiguousarray(want).tobytes(), "max |diff| = %g" % np.abs(out - want).max()


@pytest.mark.parametrize("j", range(24))
def test_one_odd_row(j):
    """one row perturbed in one component, at every position of a wavefront's order and in both halo pairs"""
    q = planar(120, 48)
    q[4, :, j] += 0.25
    got, host = first_launch(120, 48, q, steps=2)
    assert 80 <= host < 96 and got == host, (j, got, host)


def test_signed_zero_transverse_momentum():
    q = planar(120, 48)
    q[2, :, 17] = -0.0
    got, host = first_launch(120, 48, q)
    assert host_count(q, bitwise=False) == 96 and host == 92 and got == host, (got, host)


def test_signed_zero_at_rest():
    """gas at rest with a tracer jump; one row's x momentum is -0"""
    q = Q.uniform(120, 48)
    q[4, 30:90] = 1.0
    q[1, :, 5] = -0.0
    got, host = first_launch(120, 48, q)
    assert host_count(q, bitwise=False) == 96 and host == 92 and got == host, (got, host)


@pytest.mark.parametrize("x", [58, 59, 60, 61])
def test_difference_in_a_halo_column(x):
    """one cell next to the tile edge at x = 60: the owner's rows differ, and so do the neighbour's, which holds the
    cell in a halo column only"""
    q = planar(120, 48)
    q[0, x, 17] += 0.5
    got, host = first_launch(120, 48, q)
    assert host == 96 - 4 and got == host, (x, got, host)


def rectangle(mx, my):
    q = Q.uniform(mx, my)
    q[0, 20:33, 15:21] = 3.0
    q[3, 20:33, 15:21] = 7.0
    return q


@pytest.mark.parametrize("init", [rectangle, Q.blob], ids=["rectangle", "disc"])
def test_shortcut_rows_next_to_computed_rows(init):
    """a blob that touches some rows of a tile: rows that take the shortcut before and behind rows that compute, equal
    rows among both kinds"""
    q = init(120, 48)
    got, host = first_launch(120, 48, q, steps=6)
    assert 0 < host < 96 and got == host, (got, host)


def test_partial_tiles_427_197():
    """rows past the array are not swept, columns past it repeat the last one"""
    bc = (B.outflow,) * 4
    q = planar(427, 197)
    got, host = first_launch(427, 197, q, bc=bc)
    assert host == 8 * (16 * 12 + 5) and got == host, (got, host)


# ---- frame -----------------------------------------------------------------------------------------------------------
WALL = (B.periodic, B.periodic, B.reflecting, B.outflow)


def test_frame_reflecting_zero_normal_momentum():
    """the mirrored ghost rows hold -0: they chain with each other, not with the +0 rows above them"""
    q = planar(120, 48)
    got, host = first_launch(120, 48, q, bc=WALL)
    assert host_count(q, WALL, bitwise=False) == 96 and host == 94 and got == host, (got, host)


def test_frame_reflecting_normal_momentum():
    q = planar(120, 48)
    q[2] = -0.3 * q[0]
    q[3] += 0.5 * 0.09 * q[0]
    got, host = first_launch(120, 48, q, bc=WALL)
    assert host == 94 and got == host, (got, host)


def test_frame_constant_inflow():
    """constant-state inflow on the left as in the shock-bubble, outflow elsewhere"""
    bc = (B.custom, B.outflow, B.outflow, B.outflow)
    inflow = (1.2, 0.5, 0.0, 3.0, 0.0)
    q = planar(120, 48)
    got, host = first_launch(120, 48, q, bc=bc, const=inflow)
    assert host == 96 and got == host, (got, host)


def test_frame_outflow():
    bc = (B.outflow,) * 4
    q = planar(120, 48)
    got, host = first_launch(120, 48, q, bc=bc)
    assert host == 96 and got == host, (got, host)


# ---- fused source ----------------------------------------------------------------------------------------------------
def test_shockbubble_fused_source():
    """240 x 120 with the fused source: the source acts at the store, behind the sweeps"""
    def make():
        claw = problems.shockbubble(pyclaw, mx=240, my=120, tfinal=0.04, device_callbacks=True, with_src=True,
                                    dt_initial=0.005 * 160 / 240, run=False)
        claw.keep_copy = False
        claw.output_format = None
        return claw
    reads, on = run2(make, at={0, 4, 9})
    assert len(reads) == 3 and all(n > 0 for n in reads.values()), reads


# ---- several launches ------------------------------------------------------------------------------------------------
def test_rejected_and_retaken_step():
    reads, on = run2(euler(420, 180, H.moving_blob(0.5, 0.3), bc=(B.outflow,) * 4, steps=40, dt_variable=True,
                           cfl=(0.5, 0.45), dt0=1.0), at={0, 10, 25})
    assert any(e[0] == "undo" for e in on[2]), on[2]
    assert all(n > 0 for n in reads.values()), reads


def test_put_q_and_undo_between_steps():
    mx, my = 420, 180

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
    reads, on = run2(euler(mx, my, H.moving_blob(0.4, 0.2), steps=24), at={4, 7, 13, 18}, extra=extra)
    assert len(reads) == 4 and all(n > 0 for n in reads.values()), reads
    assert Q.skipped(on) > 0


def test_auto_form_trial_window():
    """80 steps: the default form policy runs its trial steps in both forms (pcl_step_form_stats behind the last calls)"""
    forms = []

    def extra(k, h, rec):
        if k >= 79:
            ms, n = ctypes.c_double(), ctypes.c_long()
            one, two = ctypes.c_long(), ctypes.c_long()
            _lib.check(_lib.lib().pcl_step_form_stats(h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(one),
                                                      ctypes.byref(two)))
            forms.append((rec.reuse, k, one.value, two.value))
    reads, on = run2(euler(600, 240, H.moving_blob(0.6, 0.2), steps=80), at={30, 60, 78}, extra=extra)
    assert any(n > 0 for n in reads.values()), reads
    assert Q.skipped(on) > 0
    for reuse in (False, True):
        last = [f for f in forms if f[0] == reuse][-1]
        assert last[2] >= 4 and last[3] >= 4 and last[2] + last[3] >= 80, forms


# ---- decomposed block ------------------------------------------------------------------------------------------------
def test_decomposed_block_tile_subsets(monkeypatch):
    """a block whose 8 neighbours are itself, exchange-ahead order of the one-kernel step: every step is an interior and
    a rim launch over tile subsets (pcl_halo_can_overlap == 2).  Planar front with one odd row; accepted steps, a
    rejected one with its retake, an upload in between.  Switch off and on give the same bytes and Courant numbers, and
    so does the undecomposed block with local periodic fills."""
    import test_gpu_halo as HALO
    lib = _lib.lib()
    monkeypatch.setenv("PCL_HALO_OVERLAP", "1")
    mx, my, g = 300, 200, 2
    q0 = planar(mx, my)
    q0[4, :, 77] += 0.25
    q0 = np.asfortranarray(q0)
    dt = 2e-3 * 100 / mx
    res = []
    for with_comm, reuse in ((False, True), (True, False), (True, True)):
        h = HALO.make_solver(_lib, mx, my)
        try:
            if with_comm:
                uid = ctypes.create_string_buffer(128)
                _lib.check(lib.pcl_comm_unique_id(uid))
                _lib.check(lib.pcl_comm_init(h, 1, 0, uid, _lib.i(np.zeros(8, dtype=np.int32))))
                yes = ctypes.c_int(0)
                _lib.check(lib.pcl_halo_can_overlap(h, ctypes.byref(yes)))
                assert yes.value == 2
                _lib.check(lib.pcl_halo_exchange_ahead(h, 2))
                bc = np.full(4, -1, dtype=np.int32)
            else:
                bc = np.full(4, 2, dtype=np.int32)
            _lib.check(lib.pcl_tile_rowreuse(h, 1 if reuse else 0))
            poison = np.full((5, mx + 2 * g, my + 2 * g), np.nan, order="F")
            _lib.check(lib.pcl_put_q(h, _lib.d(poison), 1))
            _lib.check(lib.pcl_put_q(h, _lib.d(q0), 0))
            consts = np.zeros(4 * 8)
            cfls = []

            def step(d):
                cfl = ctypes.c_double()
                _lib.check(lib.pcl_bc_step(h, _lib.i(bc), _lib.d(consts), d, ctypes.cast(ctypes.byref(cfl), _lib.dp)))
                cfls.append(cfl.value.hex())
            step(dt)
            step(dt)
            step(3 * dt)
            _lib.check(lib.pcl_undo_step(h))
            step(0.7 * dt)
            step(dt)
            mid = np.zeros_like(q0)
            _lib.check(lib.pcl_get_q(h, _lib.d(mid), 0))
            _lib.check(lib.pcl_put_q(h, _lib.d(np.asfortranarray(mid[:, ::-1, :])), 0))
            step(dt)
            step(dt)
            out = np.zeros_like(q0)
            _lib.check(lib.pcl_get_q(h, _lib.d(out), 0))
            ms, n = ctypes.c_double(), ctypes.c_long()
            one, two = ctypes.c_long(), ctypes.c_long()
            _lib.check(lib.pcl_step_form_stats(h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(one), ctypes.byref(two)))
            res.append((out.tobytes(), cfls, (one.value, two.value)))
        finally:
            lib.pcl_destroy(h)
    local, off, on = res
    print("Courant numbers", [float.fromhex(c) for c in on[1]], "forms (one kernel, two passes)", off[2], on[2])
    assert 0.1 < float.fromhex(on[1][0]) < 1.0
    assert off[2] == on[2] == (7, 0), (off[2], on[2])            # every step of the decomposed runs in the one-kernel form
    assert off[1] == on[1] == local[1], "Courant numbers differ"
    assert off[0] == on[0], "switch off and on differ"
    assert on[0] == local[0], "decomposed block differs from the periodic one"
    assert on[0] != q0.tobytes() and np.isfinite(np.frombuffer(on[0])).all()


# ---- dense -----------------------------------------------------------------------------------------------------------
def test_dense_random_state():
    """no two rows are equal: nothing is reused in any launch"""
    q = Q.dense(420, 180)
    assert host_count(q) == 0
    reads, on = run2(euler(420, 180, lambda *_: q.copy(), steps=10), at={0, 2, 5, 8})
    assert len(reads) == 4 and all(n == 0 for n in reads.values()), reads
