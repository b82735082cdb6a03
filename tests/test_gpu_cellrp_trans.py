"""
GPU: the unsplit 2-D step of a user-written Riemann solver with a transverse body (pyclaw.CellRiemann(...,
transverse=...), pcl_create_cellrp).  The library compiles its own unsplit x and y kernels around the two
bodies, so a built-in solver restated as bodies (apps/problems.py) must give the bits of the built-in path: against the
frozen oracle's step2 through the solver handle, on the tile edges of the kernels (60 owned cells per strip, 14 or 10 owned
slices per workgroup), on states with flat stretches (jump-free wavefronts take zero pieces and the body's speeds), and
through the public interface against the same run with the built-in solver.  A system the library does not have (2-D
Burgers) is checked against a numpy statement of step2.f + flux2.f on dyadic data, where every operation is exact.
'exact' arithmetic; comparisons are equalities.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyclaw_amd as pyclaw
from apps import problems
from oracle import oracle as O
from pyclaw_amd import _lib as L

PCL_RP_CELL = 100
ACOUSTICS_PAR = [1.0, 4.0, 2.0, 2.0]


def stats():
    n, h = C.c_long(), C.c_long()
    L.check(L.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def unsplit_config(meqn, mwaves, shape, d, mbc, order, mthlim, par, trans, maux=0, math=0):
    cfg = L.Config()
    cfg.ndim = 2
    for k in range(2):
        cfg.n[k] = shape[k]
        cfg.d[k] = d[k]
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = mbc, meqn, mwaves, maux
    for k, v in enumerate([1, order, trans, 0, 0, 0, maux]):
        cfg.method[k] = v
    for k, m in enumerate(mthlim):
        cfg.mthlim[k] = m
    cfg.rp = PCL_RP_CELL
    for k, v in enumerate(par):
        cfg.rp_params[k] = v
    cfg.math = math
    return cfg


class Handle(object):
    """an unsplit PCL_RP_CELL solver handle (method[2] = trans) created with its Riemann solver attached"""

    def __init__(self, body, tbody, meqn, mwaves, shape, d, mbc, order, mthlim, par, trans, maux=0, aux=(), math=0):
        self.rp = pyclaw.CellRiemann(body, meqn, mwaves, 2, aux=aux, transverse=tbody).compile(['exact', 'fast', 'strict'][math])
        self.cfg = unsplit_config(meqn, mwaves, shape, d, mbc, order, mthlim, par, trans, maux, math)
        self.h = C.c_void_p()
        L.check(L.lib().pcl_create_cellrp(C.byref(self.cfg), self.rp._rp, C.byref(self.h)))

    def put_aux(self, aux):
        assert aux.flags.f_contiguous
        L.check(L.lib().pcl_put_aux(self.h, L.d(aux)))
        return self

    def try_step(self, q0, dt):
        lib = L.lib()
        cfl = C.c_double()
        L.check(lib.pcl_put_q(self.h, L.d(q0), 1))
        rc = lib.pcl_step_hyperbolic(self.h, dt, C.cast(C.byref(cfl), L.dp))
        return rc, cfl.value

    def step(self, q0, dt):
        """one unsplit step over q0 (ghost cells included); the new array with ghosts and the Courant number"""
        rc, cfl = self.try_step(q0, dt)
        L.check(rc)
        out = np.empty_like(q0, order="F")
        L.check(L.lib().pcl_get_q(self.h, L.d(out), 1))
        return out, cfl

    def close(self):
        L.lib().pcl_destroy(self.h)
        self.h = None


def inner(mbc):
    """the unsplit step updates interior cells; the oracle also dirties ghost cells nobody reads (test_gpu_classic.py)"""
    return (slice(None), slice(mbc, -mbc), slice(mbc, -mbc))


# name -> (normal body, transverse body, oracle id, meqn, mwaves, parameters, listed aux)
SOLVERS = {
    "advection": ("ADVECTION_2D_RP", "ADVECTION_2D_RPT", O.RP_ADVECTION_2D, 1, 1, [0.7, -0.4], ()),
    "acoustics": ("ACOUSTICS_2D_RP", "ACOUSTICS_2D_RPT", O.RP_ACOUSTICS_2D, 3, 2, ACOUSTICS_PAR, ()),
    "shallow": ("SHALLOW_2D_RP", "SHALLOW_2D_RPT", O.RP_SHALLOW_2D, 3, 3, [1.0], ()),
    "vc_acoustics": ("VC_ACOUSTICS_2D_RP", "VC_ACOUSTICS_2D_RPT", O.RP_VC_ACOUSTICS_2D, 3, 2, [], (0, 1)),
    "vc_advection": ("VC_ADVECTION_2D_RP", "VC_ADVECTION_2D_RPT", O.RP_VC_ADVECTION_2D, 1, 1, [], (0, 1)),
}
LIMITERS = {1: [[4], [1]], 2: [[4, 4], [1, 2]], 3: [[4, 4, 4], [1, 2, 3]]}


def state_of(name, rng, shape):
    """q with ghost cells; shallow water: h in [0.5, 1.5] and small momenta, so that every intermediate depth is positive"""
    meqn = SOLVERS[name][3]
    if name == "shallow":
        q = 0.1 * rng.standard_normal((meqn,) + shape)
        q[0] = rng.uniform(0.5, 1.5, shape)
        return np.asfortranarray(q)
    return np.asfortranarray(rng.standard_normal((meqn,) + shape))


def aux_of(name, rng, shape):
    """noisy positive coefficients (impedance and sound speed, or edge velocities); None for the solvers without aux"""
    return np.asfortranarray(rng.uniform(0.5, 2.0, (2,) + shape)) if SOLVERS[name][6] else None


def check_step2(coracle, name, q0, aux, mx, my, mbc, lims, orders, transs):
    body, tbody, rp, meqn, mwaves, par, listed = SOLVERS[name]
    par8 = np.array(list(par) + [0.0] * (8 - len(par)))
    maux = 2 if listed else 0
    dx, dy, dt = 2.0 / mx, 2.0 / my, 0.2 / max(mx, my)
    for lim in lims:
        for order in orders:
            for trans in transs:
                method = np.array([1, order, trans, 0, 0, 0, maux], dtype=np.int32)
                ref = q0.copy("F")
                _, cfl_ref = coracle.step2(rp, par8, max(mx, my), mbc, mx, my, q0.copy("F"), ref, aux, dx, dy, dt, method,
                                           np.array(lim, dtype=np.int32))
                hd = Handle(getattr(problems, body), getattr(problems, tbody), meqn, mwaves, (mx, my), (dx, dy), mbc, order, lim,
                            par, trans, maux, listed)
                try:
                    if listed:
                        hd.put_aux(aux)
                    out, cfl = hd.step(q0, dt)
                finally:
                    hd.close()
                i = inner(mbc)
                assert np.isfinite(ref[i]).all()
                assert np.array_equal(out[i], ref[i]), (lim, order, trans, np.abs(out[i] - ref[i]).max())
                assert cfl == cfl_ref and cfl > 0, (lim, order, trans)


@pytest.mark.parametrize("mx,my", [(1, 1), (7, 5), (61, 15), (29, 61)])
@pytest.mark.parametrize("name", sorted(SOLVERS))
def test_restated_solvers_against_the_oracle(coracle, name, mx, my):
    """(61, 15): one cell over the 60-cell strip and one slice over the 14 a workgroup of the x phase owns; (29, 61): one
    over two workgroups of the y phase and over its 60-row strip"""
    rng = np.random.default_rng(7 * mx + my + len(name))
    shape = (mx + 4, my + 4)
    q0 = state_of(name, rng, shape)
    check_step2(coracle, name, q0, aux_of(name, rng, shape), mx, my, 2, LIMITERS[SOLVERS[name][4]], (1, 2), (0, 1, 2))


def test_vc_advection_with_edge_velocities_of_both_signs(coracle):
    """(the positive coefficients above leave the down-going part zero: here dmin and dmax both act)"""
    rng = np.random.default_rng(23)
    mx, my = 61, 15
    q0 = state_of("vc_advection", rng, (mx + 4, my + 4))
    aux = np.asfortranarray(rng.standard_normal((2, mx + 4, my + 4)))
    check_step2(coracle, "vc_advection", q0, aux, mx, my, 2, LIMITERS[1][:1], (2,), (1, 2))


@pytest.mark.parametrize("name", sorted(SOLVERS))
def test_restated_solvers_with_three_ghost_layers(coracle, name):
    rng = np.random.default_rng(5 + len(name))
    mx, my, mbc = 61, 15, 3
    shape = (mx + 2 * mbc, my + 2 * mbc)
    q0 = state_of(name, rng, shape)
    check_step2(coracle, name, q0, aux_of(name, rng, shape), mx, my, mbc, LIMITERS[SOLVERS[name][4]][:1], (2,), (2,))


# ---- the kernels with 12 slices per workgroup ------------------------------------------------------------------------------
VELOCITIES = [0.7, -0.4, 1.1, -0.9, 0.3, -1.3, 0.55, -0.15]


@pytest.mark.parametrize("mx,my", [(21, 11), (61, 31), (13, 61)])
@pytest.mark.parametrize("meqn", [8, 7])
def test_independent_scalars_take_the_kernels_of_twelve_slices(coracle, meqn, mx, my):
    """meqn = mwaves = 8 (and 7) advected scalars, ten owned slices per workgroup: the x phase cuts rows (11 = 10 + 1,
    31 = 3 * 10 + 1), the y phase columns (21 = 2 * 10 + 1, 61 = 6 * 10 + 1).  Component k is advection_2d with the
    velocities (p[k], -p[k] / 2); the Courant number is the largest of them."""
    rng = np.random.default_rng(13 * mx + my + meqn)
    mbc = 2
    q0 = np.asfortranarray(rng.standard_normal((meqn, mx + 4, my + 4)))
    par = VELOCITIES[:meqn]
    dx, dy, dt = 2.0 / mx, 2.0 / my, 0.2 / max(mx, my)
    has, slices = C.c_int(), C.c_int()
    for order, trans in ((2, 2), (2, 1), (1, 1), (2, 0)):
        hd = Handle(problems.SCALARS_2D_RP, problems.SCALARS_2D_RPT, meqn, meqn, (mx, my), (dx, dy), mbc, order, [4] * meqn,
                    par, trans)
        try:
            L.check(L.lib().pcl_cellrp_transverse(hd.rp._rp, C.byref(has), C.byref(slices)))
            out, cfl = hd.step(q0, dt)
        finally:
            hd.close()
        assert (has.value, slices.value) == (1, 12)
        method = np.array([1, order, trans, 0, 0, 0, 0], dtype=np.int32)
        cfls = []
        for k in range(meqn):
            qk = np.asfortranarray(q0[k:k + 1])
            ref = qk.copy("F")
            par8 = np.array([par[k], -0.5 * par[k]] + [0.0] * 6)
            _, c = coracle.step2(O.RP_ADVECTION_2D, par8, max(mx, my), mbc, mx, my, qk, ref, None, dx, dy, dt, method,
                                 np.array([4], dtype=np.int32))
            cfls.append(c)
            assert np.array_equal(out[k][2:-2, 2:-2], ref[0][2:-2, 2:-2]), (order, trans, k)
        assert cfl == max(cfls), (order, trans)


# ---- flat stretches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["acoustics", "shallow"])
def test_flat_stretches_take_zero_pieces_and_the_speeds_of_the_body(coracle, name):
    """the state of test_gpu_cellrp.py::test_flat_stretches_take_the_speeds_of_the_body_2d -- a block of 170 x 150 equal
    cells inside noise, whole constant rows and columns -- under the unsplit step with order_trans = 2: wavefronts of
    either phase inside them are jump-free, give zero pieces without calling the transverse body and take speeds(), the
    normal body again.  (Shallow water: the same places with constants that are a physical state, depth first.)"""
    rng = np.random.default_rng(3 + len(name))
    mx, my = 257, 200
    q0 = state_of(name, rng, (mx + 4, my + 4))
    meqn = q0.shape[0]
    flat = {"acoustics": lambda m: (0.25 * (m + 1), -0.5 * (m + 1), 1.5 + m),
            "shallow": lambda m: ((0.75, 0.05, -0.1)[m], (1.25, -0.1, 0.05)[m], (0.5, 0.15, 0.1)[m])}[name]
    for m in range(meqn):
        q0[m, 40:210, 30:180], q0[m, :, 190:194], q0[m, 230:236, :] = flat(m)
    check_step2(coracle, name, q0, None, mx, my, 2, LIMITERS[SOLVERS[name][4]], (2,), (2,))


# ---- a system the library does not have -------------------------------------------------------------------------------------
def burgers_fluctuations(ql, qr):
    """BURGERS_2D_RP in numpy, any float type"""
    half = ql.dtype.type(0.5)
    wave = qr - ql
    s = half * (ql + qr)
    transonic = (qr > 0) & (ql < 0)
    amdq = np.where(transonic, -half * (ql * ql), np.minimum(s, 0) * wave)
    apdq = np.where(transonic, half * (qr * qr), np.maximum(s, 0) * wave)
    return s, amdq, apdq


def step2_increments(q, dtdx, dtdy, mbc):
    """The x sweeps of step2.f with flux2.f for order = 1, order_trans = 1, no capacity function, over q[i, j] with ghost
    cells: the increment of every cell and the Courant number.  Slices j = 0 .. my+1, interfaces i = 1 .. mx+1
    (flux2.f:97-117): the Godunov update qadd, and the transverse parts of both fluctuations (BURGERS_2D_RPT) as
    gadd(., 1, .) / gadd(., 2, .) at the lower / upper edge of the cell the fluctuation enters (flux2.f:162-189); step2.f
    then adds qadd - dtdy (gadd2 - gadd1) to the slice itself, -dtdy gadd1 to the slice below and +dtdy gadd2 to the one
    above (step2.f:130-137)."""
    I, J = q.shape
    mx, my = I - 2 * mbc, J - 2 * mbc
    half = q.dtype.type(0.5)
    rows = slice(mbc - 1, mbc + my + 1)
    ql, qr = q[mbc - 1:mbc + mx, rows], q[mbc:mbc + mx + 1, rows]        # interface a = mbc .. mbc+mx, between a-1 and a
    s, amdq, apdq = burgers_fluctuations(ql, qr)
    cfl = (dtdx * np.abs(s)).max()
    sb = half * (ql + qr)
    lo, hi = np.minimum(sb, 0), np.maximum(sb, 0)
    left, right = slice(mbc - 1, mbc + mx), slice(mbc, mbc + mx + 1)      # the cells left / right of those interfaces
    qadd, g1, g2 = (np.zeros((I, my + 2), dtype=q.dtype) for _ in range(3))
    qadd[right] -= dtdx * apdq
    qadd[left] -= dtdx * amdq
    g1[left] -= half * dtdx * (lo * amdq)
    g2[left] -= half * dtdx * (hi * amdq)
    g1[right] -= half * dtdx * (lo * apdq)
    g2[right] -= half * dtdx * (hi * apdq)
    dq = np.zeros_like(q)
    dq[:, rows] += qadd - dtdy * (g2 - g1)
    dq[:, mbc - 2:mbc + my] -= dtdy * g1
    dq[:, mbc:mbc + my + 2] += dtdy * g2
    return dq, cfl


def step2_numpy(q, dtd, mbc):
    dqx, cx = step2_increments(q, dtd, dtd, mbc)
    dqy, cy = step2_increments(q.T, dtd, dtd, mbc)           # the y sweeps read qold as well (step2.f:165-218)
    return q + dqx + dqy.T, max(cx, cy)


@pytest.mark.parametrize("mx,my", [(7, 5), (61, 15)])
def test_burgers_2d_against_a_numpy_step2(mx, my):
    """q integer multiples of 1/16 in [-2, 2] of both signs, dt/dx = dt/dy = 1/4: every product and sum of the first-order
    step with transverse increments is exact in double precision whatever the order of operations (the smallest unit is
    2^-19), which the long-double recomputation below verifies; the comparison with the device is then an equality."""
    rng = np.random.default_rng(mx)
    mbc = 2
    q0 = rng.integers(-32, 33, size=(mx + 2 * mbc, my + 2 * mbc)).astype(np.float64) / 16.0
    assert (q0 > 0).any() and (q0 < 0).any()
    ref, cfl_ref = step2_numpy(q0, 0.25, mbc)
    refl, cfll = step2_numpy(q0.astype(np.longdouble), np.longdouble(0.25), mbc)
    assert np.array_equal(ref.astype(np.longdouble), refl) and np.longdouble(cfl_ref) == cfll
    d = 1.0 / 64
    hd = Handle(problems.BURGERS_2D_RP, problems.BURGERS_2D_RPT, 1, 1, (mx, my), (d, d), mbc, 1, [0], [], 1)
    try:
        out, cfl = hd.step(np.asfortranarray(q0[None]), 0.25 * d)
    finally:
        hd.close()
    i = (slice(mbc, -mbc), slice(mbc, -mbc))
    assert np.array_equal(out[0][i], ref[i]), np.abs(out[0][i] - ref[i]).max()
    assert cfl == cfl_ref
    # the transverse increments are part of it: the Godunov update alone is another array
    plain, _ = step2_increments(q0, 0.25, 0.0, mbc)
    assert not np.array_equal(ref[i], (q0 + plain + step2_increments(q0.T, 0.25, 0.0, mbc)[0].T)[i])


# ---- the attach rules on the device ------------------------------------------------------------------------------------------
def test_an_unsplit_solver_keeps_its_transverse_body():
    mx, my = 7, 5
    cfg = unsplit_config(3, 2, (mx, my), (0.1, 0.1), 2, 2, [4, 4], ACOUSTICS_PAR, 2)
    h = C.c_void_p()
    # nothing attached: not constructible
    assert L.lib().pcl_create_cellrp(C.byref(cfg), None, C.byref(h)) == L.EINVAL and not h.value
    plain = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2).compile()
    assert L.lib().pcl_create_cellrp(C.byref(cfg), plain._rp, C.byref(h)) == L.EINVAL and not h.value
    rng = np.random.default_rng(2)
    q0 = np.asfortranarray(rng.standard_normal((3, mx + 4, my + 4)))
    hd = Handle(problems.ACOUSTICS_2D_RP, problems.ACOUSTICS_2D_RPT, 3, 2, (mx, my), (0.1, 0.1), 2, 2, [4, 4], ACOUSTICS_PAR, 2)
    try:
        before, cfl0 = hd.step(q0, 0.01)
        assert L.lib().pcl_cellrp_attach(hd.h, plain._rp) == L.EINVAL
        assert b"transverse" in L.lib().pcl_last_error()
        after, cfl1 = hd.step(q0, 0.01)             # the module attached before is still there
        assert np.array_equal(after, before) and cfl1 == cfl0 and not np.array_equal(before[inner(2)], q0[inner(2)])
    finally:
        hd.close()


def test_a_step_before_the_aux_array_was_put_is_refused():
    hd = Handle(problems.VC_ADVECTION_2D_RP, problems.VC_ADVECTION_2D_RPT, 1, 1, (7, 5), (0.1, 0.1), 2, 2, [4], [], 2, 2, (0, 1))
    try:
        q0 = np.asfortranarray(np.ones((1, 11, 9)))
        rc, _ = hd.try_step(q0, 0.01)
        assert rc == L.EINVAL and b"reads aux arrays and there are none" in L.lib().pcl_last_error()
        out, _ = hd.put_aux(np.asfortranarray(np.ones((2, 11, 9)))).step(q0, 0.01)       # and with it the step runs
        assert np.array_equal(out, q0)
    finally:
        hd.close()


# ---- the public interface ----------------------------------------------------------------------------------------------------
def traced(solver):
    """(dt, Courant number) of every hyperbolic step, rejected ones included"""
    log, inner_step = [], solver.step_hyperbolic

    def step_hyperbolic(solution):
        inner_step(solution)
        log.append((solver.dt, solver.cfl.get_cached_max()))
    solver.step_hyperbolic = step_hyperbolic
    return log


def acoustics_claw(user, math='exact', order_trans=2, vc=False):
    make = problems.vc_acoustics2D if vc else problems.acoustics2D
    claw = make(pyclaw, mx=61, my=59, run=False, math=math, dim_split=0, user_rp=user)
    s = claw.solver
    s.order_trans = order_trans
    s.bc_lower[0], s.bc_upper[0] = pyclaw.BC.reflecting, pyclaw.BC.outflow
    s.bc_lower[1], s.bc_upper[1] = pyclaw.BC.outflow, pyclaw.BC.reflecting
    assert isinstance(s.rp, pyclaw.CellRiemann) == bool(user)
    return claw


def run_steps(claw, nsteps, change=None, resident=False):
    """nsteps accepted steps, one evolve_to_time call each; change = (step, function of the claw) runs in front of that step"""
    solver, solution = claw.solver, claw.solution
    log = traced(solver)
    solver.setup(solution)
    solver.dt = solver.dt_initial
    if resident:
        solver.begin_resident(solution)
    for k in range(nsteps):
        if change is not None and change[0] == k:
            change[1](claw)
        solver.evolve_to_time(solution)
    if resident:
        solver.end_resident(solution)
    q = solution.state.q.copy()
    solver.teardown()
    return q, log


@pytest.mark.parametrize("vc,order_trans", [(False, 2), (False, 1), (True, 2), (True, 1)])
def test_claw_solver_2d_unsplit_equals_the_built_in_run(vc, order_trans):
    """12 steps of a 61 x 59 box, reflecting / outflow sides, variable dt: q, every dt and every Courant number of the run
    with the built-in solver"""
    q_ref, log_ref = run_steps(acoustics_claw(False, order_trans=order_trans, vc=vc), 12)
    q, log = run_steps(acoustics_claw(True, order_trans=order_trans, vc=vc), 12)
    assert len(log) >= 12 and log == log_ref
    assert np.array_equal(q, q_ref)
    assert np.abs(q).max() > 0


def test_params_reassigned_mid_run_compile_nothing():
    """the sound speed changes behind step 5.  The built-in solver reads its parameters at setup(): its run is set up again
    there on the state it has reached, with aux_global changed alike."""
    new = [1.0, 2.25, 1.5, 1.5]          # rho, bulk, cc, zz

    claw = acoustics_claw(False)
    solver, solution = claw.solver, claw.solution
    log_ref = traced(solver)
    solver.setup(solution)
    solver.dt = solver.dt_initial
    for k in range(5):
        solver.evolve_to_time(solution)
    for key, v in zip(('rho', 'bulk', 'cc', 'zz'), new):
        solution.state.aux_global[key] = v
    solver.setup(solution)                # (evolve_to_time has brought q back to the host; dt is kept)
    for k in range(5):
        solver.evolve_to_time(solution)
    q_ref = solution.state.q.copy()
    solver.teardown()

    claw = acoustics_claw(True)
    claw.solver.rp.compile()              # whatever this process compiled before: the counts start behind it
    n0 = stats()[0]

    def change(c):
        c.solver.rp.params = new
    q, log = run_steps(claw, 10, change=(5, change))
    assert stats()[0] == n0
    assert log == log_ref and np.array_equal(q, q_ref)
    assert log[5] != log[4]


def test_a_rejected_step_is_retaken_with_the_same_bits():
    def too_large(claw):
        claw.solver.dt_initial = 4.0 * claw.solver.dt_initial
        return claw
    q_ref, log_ref = run_steps(too_large(acoustics_claw(False)), 4)
    q, log = run_steps(too_large(acoustics_claw(True)), 4)
    assert log_ref[0][1] > 0.5 and len(log_ref) == 5           # the first step was rejected (cfl_max = 0.5) and retaken
    assert log == log_ref and np.array_equal(q, q_ref)


def test_resident_run_with_a_gauge_writes_the_same_file(tmp_path):
    out = []
    for user in (False, True):
        claw = acoustics_claw(user)
        grid = claw.solution.state.grid
        grid.gauge_path = str(tmp_path / ("user" if user else "builtin")) + os.sep
        grid.add_gauges([((30 + 0.5) * grid.d[0], (12 + 0.5) * grid.d[1])])       # Grid.add_gauges: index = floor(x / d)
        assert grid.gauges == [[30, 12]]
        q, log = run_steps(claw, 16, resident=True)
        for f in grid.gauge_files:
            f.close()
        files = [open(f.name, "rb").read() for f in grid.gauge_files]
        out.append((q, log, files))
    (q_ref, log_ref, files_ref), (q, log, files) = out
    assert len(files) == 1 and files[0].count(b"\n") == 16
    assert files == files_ref and log == log_ref and np.array_equal(q, q_ref)


def test_fast_mode_is_within_the_projects_gate_of_exact():
    """unsplit acoustics on the 61 x 59 box, 'fast' against 'exact': rtol 1e-12 of the exact run's largest value, the gate
    of the 'fast' arithmetic as test_gpu_cellrp.py::test_fast_mode_is_within_the_projects_gate_of_exact
    applies it (that test states the figure inline; there is no name to import)."""
    q_ref, _ = run_steps(acoustics_claw(True), 10)
    q, _ = run_steps(acoustics_claw(True, math='fast'), 10)
    print("fast against exact: max |diff| = %g" % np.abs(q - q_ref).max())
    assert np.abs(q - q_ref).max() <= 1e-12 * np.abs(q_ref).max()
