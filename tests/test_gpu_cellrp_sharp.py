"""
GPU: user-written Riemann solvers in the SharpClaw stages (pyclaw.CellRiemann(..., sharpclaw=True),
pcl_cellrp_compile_sharp).  A built-in solver restated as a body (apps/problems.py) and compiled at run
time into the library's own SharpClaw kernels gives the bits of the built-in solver: one pcl_sharp_dq through a raw
pcl_create_cellrp handle against the frozen oracle called with the built-in id -- every reconstruction, aux lists, a
capacity function, f-waves, weno_order 7 and 17, the wave-based reconstruction, and a system the library lacks in 2-D --
and SharpClawSolver1D / 2D runs against the built-in runs.

Shapes: at order 5 a 64-lane strip owns 58 cells and a tile holds 16 slices across, so 1-D mx in {1, 58, 59} and 2-D
(1, 1), (9, 5), (59, 17) cross every boundary of the kernel; order 7 owns 56 cells (57), order 17 owns 46 (47).
The library caches every compile by its key, so no text is compiled twice however many cases share it.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyclaw_amd as pyclaw
from apps import problems, psystem
from oracle import driver as D
from oracle import oracle as O
from pyclaw_amd import _lib as L
import test_sharpclaw_matrix_cpu as M

PCL_RP_CELL = 100
MX_1D = [1, 58, 59]
SHAPES_2D = [(1, 1), (9, 5), (59, 17)]
ACOUSTICS_PAR = [1.0, 4.0, 2.0, 2.0]


def stats():
    n, h = C.c_long(), C.c_long()
    L.check(L.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def user_dq(body, meqn, mwaves, shape, d, dt, q, par=(), lim=2, order=5, cd=0, aux=None, aux_list=(), mcapa=0, fwave=False,
            mthlim=None, math='exact'):
    """One pcl_sharp_dq of a solver created with pcl_create_cellrp around `body` -> (dq with ghost cells, Courant number)"""
    lib = L.lib()
    ndim = len(shape)
    rp = pyclaw.CellRiemann(body, meqn, mwaves, ndim, aux=aux_list, fwave=fwave, capa=mcapa > 0, sharpclaw=True)
    rp.compile(math, sharp=(lim, order, cd))
    cfg = L.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k], cfg.d[k] = shape[k], d[k]
    cfg.mbc = (order + 1) // 2
    cfg.meqn, cfg.mwaves, cfg.rp = meqn, mwaves, PCL_RP_CELL
    cfg.maux = 0 if aux is None else aux.shape[0]
    cfg.method[1], cfg.method[4], cfg.method[5], cfg.method[6] = 2, cd, mcapa, cfg.maux
    for k, m in enumerate(mthlim or [1] * 8):
        cfg.mthlim[k] = m
    cfg.fwave = int(fwave)
    for k, v in enumerate(par):
        cfg.rp_params[k] = v
    cfg.kind, cfg.lim_type = 1, lim
    cfg.math = {'exact': 0, 'fast': 1, 'strict': 2}[math]
    h = C.c_void_p()
    L.check(lib.pcl_create_cellrp(C.byref(cfg), rp._rp, C.byref(h)))
    try:
        L.check(lib.pcl_put_q(h, L.d(q), 1))
        if aux is not None:
            L.check(lib.pcl_put_aux(h, L.d(aux)))
        cfl = C.c_double()
        L.check(lib.pcl_sharp_dq(h, dt, C.cast(C.byref(cfl), L.dp)))
        L.check(lib.pcl_select(h, 3))
        out = np.zeros_like(q)
        L.check(lib.pcl_get_q(h, L.d(out), 1))
    finally:
        lib.pcl_destroy(h)
    return out, cfl.value


class oracle_state(object):
    """the oracle's module state (weno_order, mthlim, char_decomp) for one block, put back behind it"""

    def __init__(self, coracle, order=5, mthlim=None, cd=0):
        self.o, self.order, self.mthlim, self.cd = coracle, order, mthlim, cd

    def __enter__(self):
        self.o.set_weno_order(self.order)
        self.o.set_sharp_mthlim(self.mthlim or [1] * 8)
        self.o.set_char_decomp(self.cd)
        return self.o

    def __exit__(self, *exc):
        self.o.set_weno_order(5)
        self.o.set_sharp_mthlim([1] * 8)
        self.o.set_char_decomp(0)


def inner(q, g):
    return (slice(None),) + (slice(g, -g),) * (q.ndim - 1)


def same(out, cfl, ref, cfl_ref, g):
    i = inner(ref, g)
    assert np.isfinite(ref[i]).all() and np.abs(ref[i]).max() > 0 and cfl_ref > 0
    assert np.array_equal(out[i], ref[i]), np.abs(out[i] - ref[i]).max()
    assert cfl == cfl_ref


def p8(par):
    return list(par) + [0.0] * (8 - len(par))


def state_of(name, rng, shape):
    """random states of the kind tests/test_gpu_sharpclaw.py draws"""
    if name == "shallow":
        h = 0.5 + rng.random(shape)
        return np.asfortranarray(np.stack([h, h * 0.3 * rng.standard_normal(shape), h * 0.3 * rng.standard_normal(shape)]))
    n = {"acoustics1": 2, "acoustics2": 3, "scalar": 1}[name]
    return np.asfortranarray(rng.standard_normal((n,) + shape))


def coefficients(rng, n, shape):
    """noisy coefficients in [0.5, 2]"""
    return np.asfortranarray(0.5 + 1.5 * rng.random((n,) + shape))


TVD = [4, 1, 2]          # lim_type 1: one limiter per component, all different


# ---- 1: the 1-D solvers, every reconstruction --------------------------------------------------------------------------
@pytest.mark.parametrize("mx", MX_1D)
@pytest.mark.parametrize("name,lim", [("acoustics", 1), ("acoustics", 2), ("acoustics", 3), ("burgers", 2)])
def test_flux1_against_the_oracle(coracle, name, lim, mx):
    g = 3
    rng = np.random.default_rng(100 * mx + lim)
    dx, dt = 1.0 / mx, 0.2 / mx
    if name == "acoustics":
        body, rp, meqn, mwaves, par, q = problems.ACOUSTICS_1D_RP, O.RP_ACOUSTICS_1D, 2, 2, ACOUSTICS_PAR, state_of("acoustics1", rng, (mx + 2 * g,))
    else:
        body, rp, meqn, mwaves, par, q = problems.BURGERS_1D_RP, O.RP_BURGERS_1D, 1, 1, [], state_of("scalar", rng, (mx + 2 * g,))
    with oracle_state(coracle, mthlim=TVD):
        ref, cfl_ref = coracle.sharp_flux1(rp, p8(par), lim, mwaves, 0, g, mx, q, None, dx, dt)
    out, cfl = user_dq(body, meqn, mwaves, (mx,), (dx,), dt, q, par, lim=lim, mthlim=TVD)
    same(out, cfl, ref, cfl_ref, g)


# ---- 2: the 2-D solvers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx,my", SHAPES_2D)
@pytest.mark.parametrize("name,lim", [("acoustics", 1), ("acoustics", 2), ("acoustics", 3), ("advection", 2), ("shallow", 2)])
def test_flux2_against_the_oracle(coracle, name, lim, mx, my):
    g = 3
    rng = np.random.default_rng(1000 * mx + 10 * my + lim)
    shape = (mx + 2 * g, my + 2 * g)
    dx, dy, dt = 1.0 / mx, 0.8 / my, 0.02 / max(mx, my)
    body, rp, meqn, mwaves, par, q = {
        "acoustics": (problems.ACOUSTICS_2D_RP, O.RP_ACOUSTICS_2D, 3, 2, ACOUSTICS_PAR, state_of("acoustics2", rng, shape)),
        "advection": (problems.ADVECTION_2D_RP, O.RP_ADVECTION_2D, 1, 1, [0.8, -0.6], state_of("scalar", rng, shape)),
        "shallow": (problems.SHALLOW_2D_RP, O.RP_SHALLOW_2D, 3, 3, [9.81], state_of("shallow", rng, shape))}[name]
    with oracle_state(coracle, mthlim=TVD):
        ref, cfl_ref = coracle.sharp_flux2(rp, p8(par), lim, mwaves, 0, g, mx, my, q, None, dx, dy, dt)
    out, cfl = user_dq(body, meqn, mwaves, (mx, my), (dx, dy), dt, q, par, lim=lim, mthlim=TVD)
    same(out, cfl, ref, cfl_ref, g)


# ---- 3: aux lists -- the x pass reads aux from global memory, the y pass from the tile -----------------------------------
@pytest.mark.parametrize("mx", MX_1D)
def test_flux1_with_aux(coracle, mx):
    g = 3
    rng = np.random.default_rng(7 * mx)
    q, aux = state_of("scalar", rng, (mx + 2 * g,)), coefficients(rng, 1, (mx + 2 * g,))
    dx, dt = 1.0 / mx, 0.1 / mx
    with oracle_state(coracle):
        ref, cfl_ref = coracle.sharp_flux1(O.RP_ADVECTION_COLOR_1D, p8([]), 2, 1, 0, g, mx, q, aux, dx, dt)
    out, cfl = user_dq(problems.ADVECTION_COLOR_1D_RP, 1, 1, (mx,), (dx,), dt, q, aux=aux, aux_list=(0,))
    same(out, cfl, ref, cfl_ref, g)


@pytest.mark.parametrize("mx,my", SHAPES_2D)
@pytest.mark.parametrize("name", ["vc_acoustics", "vc_advection"])
def test_flux2_with_aux(coracle, name, mx, my):
    g = 3
    rng = np.random.default_rng(1000 * mx + my + len(name))
    shape = (mx + 2 * g, my + 2 * g)
    aux = coefficients(rng, 2, shape)
    dx, dy, dt = 1.0 / mx, 0.8 / my, 0.02 / max(mx, my)
    body, rp, meqn, mwaves, q = {
        "vc_acoustics": (problems.VC_ACOUSTICS_2D_RP, O.RP_VC_ACOUSTICS_2D, 3, 2, state_of("acoustics2", rng, shape)),
        "vc_advection": (problems.VC_ADVECTION_2D_RP, O.RP_VC_ADVECTION_2D, 1, 1, state_of("scalar", rng, shape))}[name]
    with oracle_state(coracle):
        ref, cfl_ref = coracle.sharp_flux2(rp, p8([]), 2, mwaves, 0, g, mx, my, q, aux, dx, dy, dt)
    out, cfl = user_dq(body, meqn, mwaves, (mx, my), (dx, dy), dt, q, aux=aux, aux_list=(0, 1))
    same(out, cfl, ref, cfl_ref, g)


# ---- 4: a capacity function in the second of three aux planes ---------------------------------------------------------
@pytest.mark.parametrize("mx", MX_1D)
def test_flux1_with_a_capacity_function(coracle, mx):
    g = 3
    rng = np.random.default_rng(11 * mx)
    q, aux = state_of("acoustics1", rng, (mx + 2 * g,)), coefficients(rng, 3, (mx + 2 * g,))
    dx, dt = 1.0 / mx, 0.1 / mx
    with oracle_state(coracle):
        ref, cfl_ref = coracle.sharp_flux1(O.RP_ACOUSTICS_1D, p8(ACOUSTICS_PAR), 2, 2, 2, g, mx, q, aux, dx, dt)
        flat, _ = coracle.sharp_flux1(O.RP_ACOUSTICS_1D, p8(ACOUSTICS_PAR), 2, 2, 0, g, mx, q, aux, dx, dt)
    assert not np.array_equal(ref[inner(ref, g)], flat[inner(ref, g)])
    out, cfl = user_dq(problems.ACOUSTICS_1D_RP, 2, 2, (mx,), (dx,), dt, q, ACOUSTICS_PAR, aux=aux, mcapa=2)
    same(out, cfl, ref, cfl_ref, g)


@pytest.mark.parametrize("mx,my", SHAPES_2D)
def test_flux2_with_a_capacity_function(coracle, mx, my):
    g = 3
    rng = np.random.default_rng(13 * mx + my)
    shape = (mx + 2 * g, my + 2 * g)
    q, aux = state_of("acoustics2", rng, shape), coefficients(rng, 3, shape)
    dx, dy, dt = 1.0 / mx, 0.8 / my, 0.01 / max(mx, my)
    with oracle_state(coracle):
        ref, cfl_ref = coracle.sharp_flux2(O.RP_ACOUSTICS_2D, p8(ACOUSTICS_PAR), 2, 2, 2, g, mx, my, q, aux, dx, dy, dt)
        flat, _ = coracle.sharp_flux2(O.RP_ACOUSTICS_2D, p8(ACOUSTICS_PAR), 2, 2, 0, g, mx, my, q, aux, dx, dy, dt)
    assert not np.array_equal(ref[inner(ref, g)], flat[inner(ref, g)])
    out, cfl = user_dq(problems.ACOUSTICS_2D_RP, 3, 2, (mx, my), (dx, dy), dt, q, ACOUSTICS_PAR, aux=aux, mcapa=2)
    same(out, cfl, ref, cfl_ref, g)


# ---- 5: f-waves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx,my,lin", [(1, 1, 1.0), (9, 5, 1.0), (59, 17, 1.0), (59, 17, 2.0)])
def test_flux2_psystem_fwave_body(coracle, mx, my, lin):
    """the p-system's f-wave body on the checkerboard medium of tests/test_gpu_sharpclaw_fwave.py: bit for bit with the
    linear stress law; with the exponential one to the 1e-13 that test holds the built-in solver to (the device's exp()
    is an ulp off glibc's)"""
    q, aux, mcapa, dx, dy, dt = M.psystem_inputs(mx, my, lin, False)
    ref, cfl_ref = M.psystem_oracle(coracle, 2, mx, my, q, aux, mcapa, dx, dy, dt)
    out, cfl = user_dq(psystem.PSYSTEM_FWAVE_2D_RP, 3, 2, (mx, my), (dx, dy), dt, q, aux=aux, aux_list=(0, 1, 2, 3), fwave=True)
    i = inner(ref, 3)
    err = np.abs(out[i] - ref[i]).max()
    print("psystem body %dx%d lin=%g: max |dq - ref| = %g, cfl diff %g" % (mx, my, lin, err, cfl - cfl_ref))
    assert np.isfinite(ref[i]).all() and np.abs(ref[i]).max() > 0
    if lin == 1.0:
        assert np.array_equal(out[i], ref[i]), err
        assert cfl == cfl_ref
    else:
        assert err <= 1e-13 and abs(cfl - cfl_ref) <= 1e-13


# ---- 6: orders the built-in solver may lack ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mx,my", [(57, 17), (17, 57)])
def test_shallow_2d_at_weno_order_7(coracle, mx, my):
    """shallow_2d has built-in SharpClaw kernels of weno_order 5 alone (refused below at mbc 4); its body gets order 7 from
    the run-time compile.  A strip owns 56 cells at this order: 57 crosses it, in x and in y.  (The compile of this text
    takes 0.8 s on the CPU, that of ACOUSTICS_1D_RP at order 17 below 1.7 s: both fit a test, so neither was replaced by
    a lower order or a smaller system.)"""
    g = 4
    rng = np.random.default_rng(mx)
    q = state_of("shallow", rng, (mx + 2 * g, my + 2 * g))
    dx, dy, dt = 1.0 / mx, 1.0 / my, 0.01 / max(mx, my)
    with oracle_state(coracle, order=7):
        ref, cfl_ref = coracle.sharp_flux2(O.RP_SHALLOW_2D, p8([9.81]), 2, 3, 0, g, mx, my, q, None, dx, dy, dt)
    out, cfl = user_dq(problems.SHALLOW_2D_RP, 3, 3, (mx, my), (dx, dy), dt, q, [9.81], order=7)
    same(out, cfl, ref, cfl_ref, g)
    dq = np.full_like(q, 7.0)
    c = C.c_double()
    rc = L.lib().pcl_sharp_flux2(O.RP_SHALLOW_2D, L.d(np.array(p8([9.81]))), 2, 3, 3, 0, 0, g, mx, my, L.d(q), L.d(dq), None,
                                 dx, dy, dt, C.cast(C.byref(c), L.dp))
    assert rc == L.EINVAL and b"weno_order 5 (mbc 3) only" in L.lib().pcl_last_error() and np.all(dq == 7.0)


@pytest.mark.parametrize("mx", [1, 47])
def test_acoustics_1d_at_weno_order_17(coracle, mx):
    g = 9
    q = state_of("acoustics1", np.random.default_rng(17 + mx), (mx + 2 * g,))
    dx, dt = 1.0 / mx, 0.5 / mx
    with oracle_state(coracle, order=17):
        ref, cfl_ref = coracle.sharp_flux1(O.RP_ACOUSTICS_1D, p8(ACOUSTICS_PAR), 2, 2, 0, g, mx, q, None, dx, dt)
    out, cfl = user_dq(problems.ACOUSTICS_1D_RP, 2, 2, (mx,), (dx,), dt, q, ACOUSTICS_PAR, order=17)
    same(out, cfl, ref, cfl_ref, g)


# ---- 7: the wave-based reconstruction ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx", MX_1D)
@pytest.mark.parametrize("lim,mth", [(1, [3, 5]), (2, [1, 1])])
def test_flux1_wave_based(coracle, lim, mth, mx):
    g = 3
    q = state_of("acoustics1", np.random.default_rng(31 * mx + lim), (mx + 2 * g,))
    if mx > 9:
        q[:, g + mx // 4:g + mx // 4 + 9] = 0.25      # a constant stretch: waves of zero norm
    dx, dt = 1.0 / mx, 0.2 / mx
    with oracle_state(coracle, mthlim=mth, cd=1):
        ref, cfl_ref = coracle.sharp_flux1(O.RP_ACOUSTICS_1D, p8(ACOUSTICS_PAR), lim, 2, 0, g, mx, q, None, dx, dt)
    out, cfl = user_dq(problems.ACOUSTICS_1D_RP, 2, 2, (mx,), (dx,), dt, q, ACOUSTICS_PAR, lim=lim, cd=1, mthlim=mth)
    same(out, cfl, ref, cfl_ref, g)


# ---- 8: a system the library lacks in 2-D --------------------------------------------------------------------------------
def test_burgers_2d_from_the_1d_oracle(coracle):
    """q_t + (q^2/2)_x + (q^2/2)_y = 0 has no built-in 2-D solver.  flux2 is flux1 slice by slice (flux2.f90): the x result
    of each row, then the y result of each column, added in the kernel's order (0 + dq_x) + dq_y; the Courant number is
    the maximum over all the slices flux2 sweeps, one ghost slice on either side included."""
    mx, my, g = 59, 17, 3
    q = state_of("scalar", np.random.default_rng(5917), (mx + 2 * g, my + 2 * g))
    dx, dy, dt = 1.0 / mx, 0.8 / my, 0.01 / mx
    ref, cfl_ref = np.zeros_like(q), 0.0
    dqy = np.zeros_like(q)
    with oracle_state(coracle):
        for j in range(g - 1, g + my + 1):
            d1, c = coracle.sharp_flux1(O.RP_BURGERS_1D, p8([]), 2, 1, 0, g, mx, np.asfortranarray(q[:, :, j]), None, dx, dt)
            cfl_ref = max(cfl_ref, c)
            if g <= j < g + my:
                ref[:, g:-g, j] = 0.0 + d1[:, g:-g]
        for i in range(g - 1, g + mx + 1):
            d1, c = coracle.sharp_flux1(O.RP_BURGERS_1D, p8([]), 2, 1, 0, g, my, np.asfortranarray(q[:, i, :]), None, dy, dt)
            cfl_ref = max(cfl_ref, c)
            if g <= i < g + mx:
                dqy[:, i, g:-g] = d1[:, g:-g]
    ref = ref + dqy
    out, cfl = user_dq(problems.BURGERS_2D_RP, 1, 1, (mx, my), (dx, dy), dt, q)
    same(out, cfl, ref, cfl_ref, g)


# ---- the launcher's refusals and the fused dq source ---------------------------------------------------------------------
def test_no_fused_dq_source_on_a_cell_handle():
    lib = L.lib()
    rp = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2, sharpclaw=True).compile(sharp=(2, 5, 0))
    cfg = L.Config()
    cfg.ndim = 2
    cfg.n[0] = cfg.n[1] = 8
    cfg.d[0] = cfg.d[1] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux, cfg.rp = 3, 3, 2, 1, PCL_RP_CELL
    cfg.method[1], cfg.method[6] = 2, 1
    cfg.kind, cfg.lim_type = 1, 2
    h = C.c_void_p()
    L.check(lib.pcl_create_cellrp(C.byref(cfg), rp._rp, C.byref(h)))
    try:
        p = (C.c_double * 2)(0.4, 2.0)
        assert lib.pcl_sharp_fuse_dq_src(h, 1, p, 2) == L.EINVAL
        assert b"PCL_RP_CELL" in lib.pcl_last_error() and b"own pass" in lib.pcl_last_error()
        assert lib.pcl_sharp_fuse_dq_src(h, 0, None, 0) == L.OK
    finally:
        lib.pcl_destroy(h)


# ---- the public interface ------------------------------------------------------------------------------------------------
def traced(solver):
    """(dt, Courant number) behind every step, rejected ones included"""
    log, inner_step = [], solver.step

    def step(solution):
        r = inner_step(solution)
        log.append((solver.dt, solver.cfl.get_cached_max()))
        return r
    solver.step = step
    return log


def run_steps(claw, nsteps, change=None):
    """nsteps accepted steps, one evolve_to_time call each; change = (step, function of the claw) runs in front of that step"""
    solver, solution = claw.solver, claw.solution
    log = traced(solver)
    solver.setup(solution)
    solver.dt = solver.dt_initial
    for k in range(nsteps):
        if change is not None and change[0] == k:
            change[1](claw)
        solver.evolve_to_time(solution)
    q = solution.state.q.copy()
    solver.teardown()
    return q, log


def acoustics2d_claw(user, time_integrator='SSP104', math='exact', **kw):
    return problems.acoustics2D(pyclaw, mx=40, my=40, solver_type='sharpclaw', time_integrator=time_integrator, run=False,
                                math=math, user_rp=user, **kw)


@pytest.mark.parametrize("ti,nsteps", [('SSP104', 3), ('SSP33', 4)])
def test_sharpclaw_solver_2d_equals_the_built_in_run(ti, nsteps):
    """outflow on every side: device boundary conditions, so every stage is one fused pcl_sharp_bc_stage call"""
    q_ref, log_ref = run_steps(acoustics2d_claw(False, ti), nsteps)
    claw = acoustics2d_claw(True, ti)
    assert isinstance(claw.solver.rp, pyclaw.CellRiemann) and claw.solver.rp.sharpclaw
    q, log = run_steps(claw, nsteps)
    assert len(log) >= nsteps and log == log_ref
    assert np.isfinite(q_ref).all() and np.array_equal(q, q_ref)


def acoustics1d_claw(user):
    _, claw = problems.acoustics1D(pyclaw, mx=100, solver_type='sharpclaw', time_integrator='Euler', user_rp=user, run=False)
    claw.solver.cfl_max, claw.solver.cfl_desired = 0.2, 0.15
    return claw


def test_sharpclaw_solver_1d_euler_equals_the_built_in_run():
    q_ref, log_ref = run_steps(acoustics1d_claw(False), 6)
    q, log = run_steps(acoustics1d_claw(True), 6)
    assert len(log) >= 6 and log == log_ref
    assert np.isfinite(q_ref).all() and np.array_equal(q, q_ref)


def test_a_rejected_step_is_retaken_with_the_same_bits():
    def too_large(claw):
        claw.solver.dt_initial = 0.2
        return claw
    q_ref, log_ref = run_steps(too_large(acoustics2d_claw(False)), 2)
    q, log = run_steps(too_large(acoustics2d_claw(True)), 2)
    assert log_ref[0][1] > 0.5 and len(log_ref) >= 3           # the first step was rejected (cfl_max = 0.5) and retaken
    assert log == log_ref and np.array_equal(q, q_ref)


def test_params_reassigned_between_two_steps_compile_nothing():
    """the sound speed changes behind step 2.  The built-in solver reads its parameters at setup(): its run is set up again
    there on the state it has reached, with aux_global changed alike."""
    new = [1.0, 2.25, 1.5, 1.5]          # rho, bulk, cc, zz

    claw = acoustics2d_claw(False)
    solver, solution = claw.solver, claw.solution
    log_ref = traced(solver)
    solver.setup(solution)
    solver.dt = solver.dt_initial
    for k in range(2):
        solver.evolve_to_time(solution)
    for key, v in zip(('rho', 'bulk', 'cc', 'zz'), new):
        solution.state.aux_global[key] = v
    solver.setup(solution)                # (evolve_to_time has brought q back to the host; dt is kept)
    for k in range(2):
        solver.evolve_to_time(solution)
    q_ref = solution.state.q.copy()
    solver.teardown()

    claw = acoustics2d_claw(True)
    claw.solver.rp.compile(sharp=(2, 5, 0))        # whatever this process compiled before: the counts start behind it
    n0 = stats()[0]

    def change(c):
        c.solver.rp.params = new
    q, log = run_steps(claw, 4, change=(2, change))
    assert stats()[0] == n0
    assert log == log_ref and np.array_equal(q, q_ref)
    assert log[2] != log[1]


def test_a_cell_dq_source_beside_the_user_solver():
    """a CellDqSource runs as its own pass behind the two directional passes, for the user solver as for the built-in one"""
    def with_src(claw):
        claw.solver.dq_src = pyclaw.CellDqSource("dq[0] = -c.dt * p[0] * q[0]; dq[1] = c.dt * p[0] * q[2];", params=[0.75])
        return claw
    q_ref, log_ref = run_steps(with_src(acoustics2d_claw(False)), 2)
    q_plain, _ = run_steps(acoustics2d_claw(False), 2)
    q, log = run_steps(with_src(acoustics2d_claw(True)), 2)
    assert not np.array_equal(q_ref, q_plain)
    assert log == log_ref and np.array_equal(q, q_ref)


def test_fast_mode_is_within_the_gate_of_test_sharpclaw_fast_math(coracle):
    """math='fast': 2-D acoustics against the oracle's exact run, within the 1e-12 (relative to max |q|) that
    tests/test_gpu_sharpclaw.py::test_sharpclaw_fast_math holds the built-in solver to"""
    claw = acoustics2d_claw(True, math='fast', tfinal=0.05, nout=1)
    claw.run()
    p = D.acoustics2d_problem(mx=40, my=40, solver_type='sharpclaw')
    D.run(p, coracle, 0.05, 1)
    q = claw.frames[claw.nout].state.q
    err = np.max(np.abs(q - p.q))
    print("fast mode: max |q - oracle| = %g, max |q| = %g" % (err, np.abs(p.q).max()))
    assert err < 1e-12 * np.abs(p.q).max()
