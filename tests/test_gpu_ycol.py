"""
GPU: the column shortcut in the y sweeps of the one-kernel dimension-split step (classic_fused.hpp, DESIGN.md 4.1a, round
14).  A y sweep puts four columns into one wavefront; where each of them is constant over the 16 rows of the tile's
window while the columns differ from each other, the wavefront takes the wave speeds of its own cells and stores
nothing.  Every case runs twice in this process, pcl_tile_ycol off and on (tile skipping, the ring check and the row
reuse at their defaults), and must give byte-identical final states (no sign-of-zero normalisation, NaN bits included),
the same sequence of step calls (dt, Courant number bits, return code, every undo), the same tile counts behind every
step call and, at chosen step calls, the same ring count, class counts, quiet words and row-reuse count.  Where the
count can be recomputed on the host (tests/test_ycol_cpu.py on the oracle's x-swept array: the first launch of a run
computes every tile of the initial state) pcl_tile_ycol_stats must equal it; with the switch off it is 0.

The tile subsets of a decomposed block (unbooked launches: the switch reaches them, the counter does not) run in one
process on a block whose eight neighbours are itself, as in tests/test_gpu_row_reuse.py.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

import test_gpu_quiet_tiles as Q
import test_gpu_ring_check as R
import test_gpu_row_reuse as RR
import test_gpu_tile_handover as H
import test_row_reuse_cpu as ROWS
import test_ycol_cpu as HOST

pytestmark = pytest.mark.gpu

B = pyclaw.BC
BCNAME = RR.BCNAME
PER = (B.periodic,) * 4
OUT = (B.outflow,) * 4
planar, ramp = ROWS.planar, HOST.ramp


class Recorder(Q.Recorder):
    """Q.Recorder (skipping on) that also sets pcl_tile_ycol once per solver handle, in front of its first step"""

    def __init__(self, ycol, hook=None):
        Q.Recorder.__init__(self, True, hook)
        self.ycol, self.ycol_seen = ycol, set()

    def __enter__(self):
        Q.Recorder.__enter__(self)
        L = _lib.lib()
        bc_step, step = L.pcl_bc_step, L.pcl_step_hyperbolic

        def first(h):
            key = h.value if hasattr(h, "value") else h
            if key not in self.ycol_seen:
                self.ycol_seen.add(key)
                _lib.check(L.pcl_tile_ycol(h, 1 if self.ycol else 0))

        def ycol_bc_step(h, *args):
            first(h)
            return bc_step(h, *args)

        def ycol_step(h, *args):
            first(h)
            return step(h, *args)

        L.pcl_bc_step, L.pcl_step_hyperbolic = ycol_bc_step, ycol_step
        return self


def ycol_stats(h):
    n = ctypes.c_long(-1)
    _lib.check(_lib.lib().pcl_tile_ycol_stats(h, ctypes.byref(n)))
    return n.value


def final_bytes(claw):
    claw.solver.teardown()
    q = np.ascontiguousarray(claw.solution.state.q)
    return hashlib.sha256(q.tobytes()).hexdigest(), bool(np.isfinite(q).all())


def run2(make, at=(0, 3), extra=None, finite=True):
    """make() -> Controller ready to run.  Runs with the switch off, then on; behind the step calls in `at` both runs
    read (column shortcuts, sweeps reused, ring count, na, nq, words or None) of the launch (each read makes the next
    launch compute every tile); extra(k, h, rec) runs first behind every step call.  Returns ({k: column shortcuts} of
    the run with the switch on, its (hash, finite, log, stats))."""
    res = []
    for ycol in (False, True):
        reads = {}

        def hook(k, h, rec, reads=reads):
            if extra is not None:
                extra(k, h, rec)
            if k in at:
                reads[k] = (ycol_stats(h), RR.reuse_stats(h)) + R.read_launch(h)
        claw = make()
        with Recorder(ycol, hook) as rec:
            claw.run()
            digest, fin = final_bytes(claw)
        res.append((digest, fin, rec.log, rec.stats, reads))
    off, on = res
    assert on[1] == off[1] and (on[1] or not finite), "non-finite state"
    assert on[2] == off[2], "step sequences differ"
    assert on[0] == off[0], "final states differ"
    assert on[3] == off[3], "tile counts differ"
    assert sorted(on[4]) == sorted(off[4]) == sorted(k for k in at if k < len(on[3])), (sorted(on[4]), len(on[3]))
    for k in on[4]:
        a, b = on[4][k], off[4][k]
        print("step call %d: column shortcuts %d (switch off %d), sweeps reused %d, ring %d, na %d, nq %d"
              % ((k, a[0], b[0]) + a[1:5]))
        assert b[0] == 0, (k, b[:5])                                   # switch off: no shortcut
        assert a[0] >= 0 and a[1:5] == b[1:5], (k, a[:5], b[:5])       # sweeps reused, ring count, na, nq
        assert (a[5] is None) == (b[5] is None) and (a[5] is None or (a[5] == b[5]).all()), k
    return {k: v[0] for k, v in on[4].items()}, on[:4]


def euler(mx, my, init, bc=PER, steps=4, src=False, const=None, **kw):
    return R.euler(mx, my, init, bc=bc, steps=steps, src=src,
                   user_lower=None if const is None else pyclaw.ConstantStateBC(list(const)), **kw)


def host_kinds(coracle, mx, my, q, bc=PER, const=None):
    """the kinds of every tile's 16 groups (test_ycol_cpu.group_kinds) in the first launch of R.euler's run of q"""
    g = ROWS.fill_ghosts(q, tuple(BCNAME[b] for b in bc), const)
    d = (2.0 - 0.0) / float(mx)                         # Dimension.d of R.euler's grid, dx = dy
    qx = HOST.x_swept(coracle, g, d, d, 0.2 / max(mx, my))
    return {(tx, ty): "".join(HOST.group_kinds(*HOST.window(g, qx, tx, ty)))
            for ty in range((my + 11) // 12) for tx in range((mx + 59) // 60)}


def first_launch(coracle, mx, my, q, bc=PER, const=None, steps=2, finite=True, **kw):
    """runs q off / on; returns (column shortcuts of the first launch, the host's kinds per tile)"""
    reads, on = run2(euler(mx, my, lambda *_: q.copy(), bc=bc, steps=steps, const=const, **kw), at={0}, finite=finite)
    assert on[3][0] == (RR.HOST_TILES(mx, my), 0), on[3][0]           # one kernel, every tile
    kinds = host_kinds(coracle, mx, my, q, bc, const)
    host = sum(k.count("c") for k in kinds.values())
    assert reads[0] == host, (reads[0], host)
    return host, kinds


# ---- planar front ----------------------------------------------------------------------------------------------------
def test_planar_front_counted(coracle):
    """180 x 36, 3 x 3 tiles: all rows bit-identical; 24 steps, the count read at four of them"""
    q = planar(180, 36)
    host, kinds = first_launch(coracle, 180, 36, q, steps=24)
    assert host >= 18 and set("".join(kinds.values())) == {"u", "c"}, kinds
    reads, on = run2(euler(180, 36, lambda *_: q.copy(), steps=24), at={0, 5, 12, 23})
    assert len(reads) == 4 and all(n > 0 for n in reads.values()), reads
    assert len([e for e in on[2] if e[0] != "undo"]) >= 20


def test_ramp_every_group(coracle):
    """every column differs from its neighbours: all 16 groups of all 9 tiles"""
    host, kinds = first_launch(coracle, 180, 36, ramp(180, 36), steps=6)
    assert host == 9 * 16, kinds


# ---- one odd cell ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", [3, 4, 59, 60, 61, 62])        # group boundary 3 | 4 of the grid, tile boundary 59 | 60
@pytest.mark.parametrize("row", [0, 1, 2, 13, 14, 15])
def test_one_odd_cell(coracle, row, col):
    """one cell of the ramp changed, in window row `row` of tile row 1: only the groups that hold it -- in this tile
    column, in the neighbour whose halo columns hold it, in the tile row whose halo rows hold it, and one group further
    where the x sweep carries it over a group boundary -- compute"""
    q = ramp(180, 36)
    q[4, col, 12 + row - 2] += 0.5
    host, kinds = first_launch(coracle, 180, 36, q)
    full = "".join(kinds.values()).count("f")
    assert 1 <= full <= 8 and host == 9 * 16 - full, (row, col, kinds)
    assert set(kinds[(2, 1)]) == {"c"} and set(kinds[(1, 2)] if row < 12 else kinds[(1, 0)]) == {"c"}, kinds


# ---- signed zeros, non-finite cells ----------------------------------------------------------------------------------
# The guard looks at the cells the y sweep would store, and those come out of this launch's x sweeps.  On the states
# below the x sweep's full solve has already turned a -0 into +0 and an infinity's neighbourhood into NaNs (which equal
# nothing: a jump) when the y sweep sees them; what remains for these cases is that off and on agree in every bit and
# that the count is the host's, whose guard tests/test_ycol_cpu.py pins on windows written down by hand.
def test_minus_zero_transverse_momentum(coracle):
    q = ramp(180, 36)
    q[2, 40:48] = -0.0
    host, kinds = first_launch(coracle, 180, 36, q, steps=4)
    assert host > 0, kinds


def test_minus_zero_everywhere_at_rest(coracle):
    """gas at rest, both momenta and the tracer -0 in some columns and +0 in others, density varying from column to
    column"""
    q = ramp(180, 36)
    q[1] = 0.0
    q[1, 20:70], q[2, 50:110], q[4] = -0.0, -0.0, 0.0
    q[4, 90:150] = -0.0
    host, kinds = first_launch(coracle, 180, 36, q, steps=4)
    assert host > 0, kinds


def test_minus_zero_tracer(coracle):
    q = ramp(180, 36)
    q[4, 100:104] = -0.0
    host, kinds = first_launch(coracle, 180, 36, q, steps=4)
    assert host > 0, kinds


def test_infinite_tracer(coracle):
    """an infinite component equals itself and its difference is a NaN: the NaN bits are the parent's"""
    q = ramp(180, 36)
    q[4, 77] = np.inf
    host, kinds = first_launch(coracle, 180, 36, q, steps=4, finite=False)
    assert 0 < host < 9 * 16, kinds


# ---- frame -----------------------------------------------------------------------------------------------------------
WALL = (B.periodic, B.periodic, B.reflecting, B.outflow)


def test_reflecting_lower_side(coracle):
    """the mirrored ghost rows hold -0 normal momentum in halo lanes, which are not stored: tile row 0 keeps the shortcut"""
    host, kinds = first_launch(coracle, 180, 36, ramp(180, 36), bc=WALL, steps=6)
    assert host == 9 * 16, kinds


def test_reflecting_lower_side_normal_momentum(coracle):
    q = ramp(180, 36)
    q[2] = -0.3 * q[0]
    q[3] += 0.5 * 0.09 * q[0]
    host, kinds = first_launch(coracle, 180, 36, q, bc=WALL, steps=6)
    assert 0 < host < 9 * 16 and all(set(kinds[(tx, 0)]) == {"f"} for tx in range(3)), kinds


@pytest.mark.parametrize("bc", [OUT, PER, (B.periodic, B.periodic, B.outflow, B.outflow),
                                (B.reflecting, B.outflow, B.outflow, B.reflecting)],
                         ids=["outflow", "periodic", "mixed", "walls"])
@pytest.mark.parametrize("shape", [(200, 50), (427, 197)])
def test_sides_partial_tiles(coracle, bc, shape):
    """partial tiles: groups past the array are skipped, rows past it repeat the last input row"""
    mx, my = shape
    host, kinds = first_launch(coracle, mx, my, ramp(mx, my), bc=bc)
    assert host > 0, kinds


def test_constant_inflow(coracle):
    """constant-state inflow on the left as in the shock-bubble, outflow elsewhere"""
    bc = (B.custom, B.outflow, B.outflow, B.outflow)
    inflow = (1.2, 0.5, 0.0, 3.0, 0.0)
    host, kinds = first_launch(coracle, 200, 50, planar(200, 50), bc=bc, const=inflow, steps=12)
    assert host > 0 and kinds[(0, 0)][0] == "c", kinds


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
    assert len(reads) == 3 and any(n > 0 for n in reads.values()), reads


# ---- several launches ------------------------------------------------------------------------------------------------
def test_shockbubble_960_rejected_first_step():
    def make():
        claw = problems.shockbubble(pyclaw, mx=960, my=480, tfinal=0.04, device_callbacks=True, with_src=False,
                                    dt_initial=0.005 * 160 / 960, run=False)
        claw.keep_copy = False
        claw.output_format = None
        return claw
    reads, on = run2(make, at={1, 20, 45})
    assert sum(1 for e in on[2] if e[0] != "undo") >= 60, len(on[2])
    assert any(e[0] == "undo" for e in on[2])        # the app's first step is rejected
    assert Q.skipped(on) > 0
    assert all(n > 0 for n in reads.values()), reads


def test_put_q_between_steps():
    mx, my = 420, 180

    def init(mx, my):
        q = H.moving_blob(0.4, 0.0)(mx, my)
        q[:, :90] = ramp(90, my)                       # a strip of y-uniform columns next to the quiet gas
        return q

    def extra(k, h, rec):
        if k in (6, 12):
            L = _lib.lib()
            buf = np.empty(5 * mx * my)
            _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
            a = buf.reshape(my, mx, 5)
            a[20 + k, 30 + 2 * k, 4] += 0.25              # one cell of the strip changes on the device
            _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))
    reads, on = run2(euler(mx, my, init, bc=OUT, steps=20), at={4, 7, 13, 18}, extra=extra)
    assert len(reads) == 4 and all(n > 0 for n in reads.values()), reads
    assert Q.skipped(on) > 0


# ---- decomposed block ------------------------------------------------------------------------------------------------
def test_decomposed_block_tile_subsets(monkeypatch):
    """a block whose 8 neighbours are itself, exchange-ahead order of the one-kernel step: every step is an interior and
    a rim launch over tile subsets (pcl_halo_can_overlap == 2).  y-uniform columns with one odd cell; accepted steps, a
    rejected one with its retake, an upload in between.  Switch off and on give the same bytes and Courant numbers, and
    so does the undecomposed block with local periodic fills."""
    import test_gpu_halo as HALO
    lib = _lib.lib()
    monkeypatch.setenv("PCL_HALO_OVERLAP", "1")
    mx, my, g = 300, 200, 2
    q0 = planar(mx, my)
    q0[0] += (np.arange(mx) % 7)[:, None] / 64.0
    q0[4, 131, 77] += 0.25
    q0 = np.asfortranarray(q0)
    dt = 2e-3 * 100 / mx
    res = []
    for with_comm, ycol in ((False, True), (True, False), (True, True)):
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
            _lib.check(lib.pcl_tile_ycol(h, 1 if ycol else 0))
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
    assert 0.1 < float.fromhex(on[1][0]) < 1.0
    assert off[2] == on[2] == (7, 0), (off[2], on[2])            # every step of the decomposed runs in the one-kernel form
    assert off[1] == on[1] == local[1], "Courant numbers differ"
    assert off[0] == on[0], "switch off and on differ"
    assert on[0] == local[0], "decomposed block differs from the periodic one"
    assert on[0] != q0.tobytes() and np.isfinite(np.frombuffer(on[0])).all()


# ---- dense -----------------------------------------------------------------------------------------------------------
def test_dense_random_state(coracle):
    """no column is constant: no shortcut in any launch"""
    q = Q.dense(180, 36)
    host, kinds = first_launch(coracle, 180, 36, q, steps=3)
    assert host == 0 and set("".join(kinds.values())) == {"f"}
    reads, on = run2(euler(420, 180, lambda *_: Q.dense(420, 180), steps=10), at={0, 2, 5, 8})
    assert len(reads) == 4 and all(n == 0 for n in reads.values()), reads


# ---- the other solvers of the one-kernel step ------------------------------------------------------------------------
def test_acoustics():
    """a pressure pulse planar in x"""
    def make():
        claw = problems.acoustics2D(pyclaw, mx=240, my=96, tfinal=0.05, nout=1, dim_split=1, run=False)
        x = claw.solution.state.grid.x.center
        claw.solution.state.q[0] = (np.abs(x) <= 0.3)[:, None] * (1.0 + np.cos(np.pi * x / 0.3))[:, None]
        claw.solution.state.q[1:] = 0.0
        claw.keep_copy = False
        claw.output_format = None
        return claw
    reads, on = run2(make, at={0, 3, 8})
    assert len(reads) == 3 and all(n > 0 for n in reads.values()), reads


def test_shallow_water():
    """a dam break planar in x"""
    def make():
        solver = pyclaw.ClawSolver2D()
        solver.rp = pyclaw.riemann.rp_shallow_2d
        solver.mwaves = 3
        solver.limiters = [4, 4, 4]
        solver.dim_split = True
        for k in range(2):
            solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.outflow
        grid = pyclaw.Grid([pyclaw.Dimension('x', -2.5, 2.5, 240), pyclaw.Dimension('y', -1.0, 1.0, 96)])
        state = pyclaw.State(grid, 3)
        state.aux_global['g'] = 1.0
        X, Y = grid.c_center
        state.q[0] = 2.0 * (X <= 0.0) + 1.0 * (X > 0.0)
        state.q[1:] = 0.0
        solver.dt_initial = 1e-3
        return Q.controller(state, solver, 0.1)
    reads, on = run2(make, at={0, 3, 8})
    assert all(n > 0 for n in reads.values()), reads


def test_advection():
    """a smooth profile in x carried along x: every column differs from its neighbour"""
    mx, my = 240, 96

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
        state.aux_global['v'] = 0.5
        state.q[0] = (1.0 + np.sin(2.0 * np.pi * grid.x.center))[:, None]
        solver.cfl_max, solver.cfl_desired = 1.0, 0.9
        solver.dt_variable = False
        solver.dt_initial = 0.8 / mx
        return Q.controller(state, solver, 12 * solver.dt_initial)
    reads, on = run2(make, at={0, 3, 8})
    assert len(reads) == 3 and all(n > 0 for n in reads.values()), reads
