"""
GPU: the SharpClaw combinations added with the p-system kernels -- ``psystem_fwave_2d`` in the directional WENO/tvd2
kernels (aux planes per lane in x, through the LDS tile in y; with and without a capacity function) and the wave-based
reconstruction (char_decomp = 1) in 1-D with aux arrays and a capacity function -- against the C oracle, bit for bit
wherever no ``exp()`` is involved.  Inputs and their oracle-side soundness: tests/test_sharpclaw_matrix_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as O
import test_sharpclaw_matrix_cpu as M
from test_fwave import CC, K, RHO, ZZ

MBC = M.MBC
INNER = (slice(None), slice(MBC, -MBC), slice(MBC, -MBC))


def flux2(rp, par, lim, meqn, mwaves, mcapa, mx, my, q, aux, dx, dy, dt, mthlim=None):
    """pcl_sharp_flux2 (layer 1) -> rc, dq, cfl; the module's mthlim set for the call and put back"""
    from pyclaw_amd import _lib as L
    lib = L.lib()
    dq = np.zeros_like(q)
    cfl = C.c_double()
    p8 = np.array(list(par) + [0.0] * (8 - len(par)))
    if mthlim is not None:
        L.check(lib.pcl_sharp_module_mthlim(L.i(np.array(mthlim, dtype=np.int32)), len(mthlim)))
    try:
        rc = lib.pcl_sharp_flux2(rp, L.d(p8), lim, meqn, mwaves, 0 if aux is None else aux.shape[0], mcapa, MBC, mx, my,
                                 L.d(q), L.d(dq), None if aux is None else L.d(aux), dx, dy, dt, C.cast(C.byref(cfl), L.dp))
    finally:
        L.check(lib.pcl_sharp_module_mthlim(L.i(np.ones(8, dtype=np.int32)), 8))
    return rc, dq, cfl.value


@pytest.mark.parametrize("mx,my", M.SHAPES)
@pytest.mark.parametrize("lin", [1.0, 2.0])
@pytest.mark.parametrize("capa", [False, True])
@pytest.mark.parametrize("lim", [1, 2, 3])
def test_flux2_psystem(coracle, mx, my, lin, capa, lim):
    """device dq == the oracle's flux2 with rp_fwave_normal on a checkerboard medium: bit for bit with the linear
    stress law, to the 1e-13 of test_hip_psystem_fwave with the exponential one (the device's exp() is an ulp off)"""
    from pyclaw_amd import _lib as L
    q, aux, mcapa, dx, dy, dt = M.psystem_inputs(mx, my, lin, capa)
    ref, cfl_ref = M.psystem_oracle(coracle, lim, mx, my, q, aux, mcapa, dx, dy, dt)
    assert np.isfinite(ref[INNER]).all() and np.abs(ref[INNER]).max() > 0
    rc, dq, cfl = flux2(O.RP_PSYSTEM_FWAVE_2D, [], lim, 3, 2, mcapa, mx, my, q, aux, dx, dy, dt, M.TVD_MTHLIM)
    L.check(rc)
    err = np.abs(dq[INNER] - ref[INNER]).max()
    print("psystem flux2 %dx%d lin=%g capa=%d lim=%d: max |dq - ref| = %g, cfl diff %g" % (mx, my, lin, capa, lim, err, cfl - cfl_ref))
    if lin == 1.0:
        assert np.array_equal(dq[INNER], ref[INNER]), err
        assert cfl == cfl_ref
    else:
        assert err <= 1e-13 and abs(cfl - cfl_ref) <= 1e-13


def test_flux2_psystem_capacity_matters(coracle):
    q, aux, mcapa, dx, dy, dt = M.psystem_inputs(59, 57, 1.0, True)
    rc, with_capa, _ = flux2(O.RP_PSYSTEM_FWAVE_2D, [], 2, 3, 2, mcapa, 59, 57, q, aux, dx, dy, dt)
    rc2, without, _ = flux2(O.RP_PSYSTEM_FWAVE_2D, [], 2, 3, 2, 0, 59, 57, q, aux, dx, dy, dt)
    assert rc == 0 and rc2 == 0 and not np.array_equal(with_capa[INNER], without[INNER])


@pytest.mark.parametrize("lim", [1, 2, 3])
def test_flux2_psystem_uniform_equals_acoustics(lim):
    """uniform linear medium: the device's p-system dq is its acoustics_2d dq under p = -K eps, (u, v) = m / rho, to the
    tolerance of test_oracle_psystem_linear_uniform_equals_acoustics"""
    mx, my = 40, 31
    qa, qp, aux = M.uniform_pair(mx, my)
    dx, dy, dt = 0.05, 0.06, 0.01
    rc_a, ra, cfl_a = flux2(O.RP_ACOUSTICS_2D, [RHO, K, CC, ZZ], lim, 3, 2, 0, mx, my, qa, None, dx, dy, dt, M.TVD_MTHLIM)
    rc_p, rp, cfl_p = flux2(O.RP_PSYSTEM_FWAVE_2D, [], lim, 3, 2, 0, mx, my, qp, aux, dx, dy, dt, M.TVD_MTHLIM)
    assert rc_a == 0 and rc_p == 0
    back = np.stack([-K * rp[0], rp[1] / RHO, rp[2] / RHO])
    assert np.abs(ra[INNER]).max() > 0
    assert np.abs(back[INNER] - ra[INNER]).max() < 2e-14 and abs(cfl_a - cfl_p) < 2e-14


def sharp_config(L, rp, meqn, mwaves, maux, fwave):
    cfg = L.Config()
    cfg.ndim = 2
    cfg.n[0] = cfg.n[1] = 8
    cfg.d[0] = cfg.d[1] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux, cfg.rp = 3, meqn, mwaves, maux, rp
    cfg.method[1], cfg.method[6] = 2, maux
    cfg.kind, cfg.lim_type, cfg.fwave = 1, 2, fwave
    return cfg


def test_fwave_flag_must_match_the_solver():
    from pyclaw_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    assert lib.pcl_create(C.byref(sharp_config(L, O.RP_PSYSTEM_FWAVE_2D, 3, 2, 4, 0)), C.byref(h)) == L.EINVAL
    assert b"f-waves" in lib.pcl_last_error()
    assert lib.pcl_create(C.byref(sharp_config(L, O.RP_VC_ACOUSTICS_2D, 3, 2, 2, 1)), C.byref(h)) == L.EINVAL
    assert b"f-wave" in lib.pcl_last_error()
    L.check(lib.pcl_create(C.byref(sharp_config(L, O.RP_PSYSTEM_FWAVE_2D, 3, 2, 4, 1)), C.byref(h)))
    lib.pcl_destroy(h)
    # the 1-D elasticity f-wave solver stays a classic-only solver (no rp1 for it in the SharpClaw oracle)
    cfg = sharp_config(L, O.RP_ELASTICITY_FWAVE_1D, 2, 2, 3, 1)
    cfg.ndim = 1
    assert lib.pcl_create(C.byref(cfg), C.byref(h)) == L.EINVAL


# ---- SharpClawSolver2D on apps/psystem.py ---------------------------------------------------------------------------
def psystem_claw(time_integrator, linearity, nsteps, dt):
    import pyclaw_amd as pyclaw
    from apps import psystem
    claw = psystem.psystem2D(pyclaw, 32, 24, solver_type='sharpclaw', lower=(0.0, 0.0), upper=(4.0, 3.0), bc='periodic',
                             linearity=linearity, amplitude=1.0, center=(2.0, 1.5), time_integrator=time_integrator,
                             tfinal=nsteps * dt, nout=1, run=False)
    claw.solver.dt_variable = False
    claw.solver.dt_initial = dt                 # a power of two: n * dt is exact, every step has the same length
    return claw


def test_psystem_solver_euler_replay(coracle):
    """3 forward-Euler steps on the periodic checkerboard == q += flux2(q) of the oracle with periodic ghost cells for q
    and aux, bit for bit (linear stress law)"""
    dt, nsteps = 2.0 ** -6, 3
    claw = psystem_claw('Euler', 1, nsteps, dt)
    q = claw.solution.state.q.copy(order='F')
    aux = claw.solution.state.aux.copy(order='F')
    dx, dy = claw.solution.state.grid.d
    claw.run()
    assert claw.solver.status['numsteps'] == nsteps
    wrap = lambda a: np.asfortranarray(np.pad(a, ((0, 0), (MBC, MBC), (MBC, MBC)), mode='wrap'))
    auxbc = wrap(aux)
    for _ in range(nsteps):
        dq, cfl = coracle.sharp_flux2(O.RP_PSYSTEM_FWAVE_2D, [0.0], 2, 2, 0, MBC, 32, 24, wrap(q), auxbc, dx, dy, dt)
        q = q + dq[INNER]
    out = claw.frames[1].state.q
    assert np.isfinite(q).all() and np.abs(q[1:]).max() > 0
    assert np.array_equal(out, q), np.abs(out - q).max()


def test_psystem_solver_ssp104_conserves(coracle):
    """SSP104 on the same grid (exponential law): finite, and the sum of every component is kept to rounding.  The f-wave
    fluctuations of a cell and its two interfaces telescope, so only rounding is left: each of the 10 stages of a step
    adds to a cell dtdx * (four fluctuation terms) and combines registers, a handful of roundings of size
    eps * max(|q|, dtdx * |f|) per cell and stage; 8 of them per cell and stage bounds the drift of the sum."""
    dt, nsteps = 2.0 ** -6, 3
    claw = psystem_claw('SSP104', 2, nsteps, dt)
    st = claw.solution.state
    q0, aux = st.q.copy(order='F'), st.aux
    sigma = np.exp(aux[1] * q0[0]) - 1.0
    scale = max(np.abs(q0).max(), np.abs(sigma).max()) * (1.0 + 4.0 * dt / min(st.grid.d))
    claw.run()
    q1 = claw.frames[1].state.q
    assert np.isfinite(q1).all() and np.abs(q1[1:]).max() > 0 and not np.array_equal(q1, q0)
    tol = 8 * q0[0].size * 10 * nsteps * 2.0 ** -52 * scale
    for m in range(3):
        drift = abs(q1[m].sum() - q0[m].sum())
        print("component %d: drift of the sum %g (bound %g)" % (m, drift, tol))
        assert drift <= tol


# ---- char_decomp = 1 with aux arrays and a capacity function -------------------------------------------------------
def flux1_wave(rp, par, lim, mth, meqn, mwaves, mcapa, mx, q, aux, dx, dt):
    from pyclaw_amd import _lib as L
    lib = L.lib()
    dq = np.zeros_like(q)
    cfl = C.c_double()
    L.check(lib.pcl_sharp_module_char_decomp(1))
    L.check(lib.pcl_sharp_module_mthlim(L.i(np.array([mth] * mwaves, dtype=np.int32)), mwaves))
    try:
        rc = lib.pcl_sharp_flux1(rp, L.d(np.array(par + [0.0] * (8 - len(par)))), lim, meqn, mwaves,
                                 0 if aux is None else aux.shape[0], mcapa, MBC, mx, L.d(q), L.d(dq),
                                 None if aux is None else L.d(aux), dx, dt, C.cast(C.byref(cfl), L.dp))
    finally:
        L.check(lib.pcl_sharp_module_char_decomp(0))
        L.check(lib.pcl_sharp_module_mthlim(L.i(np.ones(8, dtype=np.int32)), 8))
    return rc, dq, cfl.value


@pytest.mark.parametrize("rp,capa", M.WAVE_CASES)
@pytest.mark.parametrize("lim,mth", M.WAVE_LIMS)
@pytest.mark.parametrize("mx", M.WAVE_MX)
def test_flux1_wave_based_aux_capa_bitexact(coracle, rp, capa, lim, mth, mx):
    """pcl_sharp_flux1 with char_decomp = 1 == the oracle's flux1, bit for bit, Courant number included: the solvers
    without aux arrays with a capacity function, the colour equation (velocity of both signs in aux(1)) without and
    with one; strip boundaries at 58 cells"""
    from pyclaw_amd import _lib as L
    q, par, meqn, mwaves, aux, mcapa, dx, dt = M.wave_inputs(rp, capa, lim, mx)
    ref, cfl_ref = M.wave_oracle(coracle, rp, par, lim, mth, mwaves, mcapa, mx, q, aux, dx, dt)
    assert np.isfinite(ref[:, MBC:-MBC]).all() and np.abs(ref[:, MBC:-MBC]).max() > 0
    rc, dq, cfl = flux1_wave(rp, par, lim, mth, meqn, mwaves, mcapa, mx, q, aux, dx, dt)
    L.check(rc)
    assert np.array_equal(dq[:, MBC:-MBC], ref[:, MBC:-MBC]), np.abs(dq - ref)[:, MBC:-MBC].max()
    assert cfl == cfl_ref


def test_flux1_wave_based_capacity_matters():
    q, par, meqn, mwaves, aux, mcapa, dx, dt = M.wave_inputs(O.RP_EULER_1D, True, 2, 59)
    rc, with_capa, cfl_w = flux1_wave(O.RP_EULER_1D, par, 2, 1, meqn, mwaves, mcapa, 59, q, aux, dx, dt)
    rc2, without, cfl_n = flux1_wave(O.RP_EULER_1D, par, 2, 1, meqn, mwaves, 0, 59, q, aux, dx, dt)
    assert rc == 0 and rc2 == 0
    assert not np.array_equal(with_capa[:, MBC:-MBC], without[:, MBC:-MBC]) and cfl_w != cfl_n


def test_color_1d_wave_based_solver_replay(coracle):
    """SharpClawSolver1D, char_decomp = 1, advection_color_1d: 120 cells, periodic, 5 SSP104 steps == the host replay of
    the same steps with the oracle's flux1 and the SSP104 formulas of pyclaw_amd/sharpclaw.py, bit for bit"""
    import pyclaw_amd as pyclaw
    mx, nsteps, dt = 120, 5, 2.0 ** -8
    solver = pyclaw.SharpClawSolver1D()
    solver.rp = pyclaw.riemann.rp_advection_color_1d
    solver.char_decomp, solver.lim_type, solver.time_integrator, solver.mwaves = 1, 2, 'SSP104', 1
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    solver.aux_bc_lower[0] = solver.aux_bc_upper[0] = pyclaw.BC.periodic
    solver.dt_variable, solver.dt_initial = False, dt
    grid = pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx))
    state = pyclaw.State(grid, 1, 1)
    state.aux[0] = 0.1 + 0.8 * np.sin(2 * np.pi * grid.x.edge[:-1])          # the velocity at the left edge, both signs
    state.q[0] = np.exp(-60.0 * (grid.x.center - 0.4) ** 2)
    q, aux, dx = state.q.copy(order='F'), state.aux.copy(order='F'), grid.d[0]
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution, claw.solver = pyclaw.Solution(state), solver
    claw.tfinal, claw.nout = nsteps * dt, 1
    claw.run()
    assert solver.status['numsteps'] == nsteps
    wrap = lambda a: np.asfortranarray(np.pad(a, ((0, 0), (MBC, MBC)), mode='wrap'))
    auxbc = wrap(aux)
    coracle.set_char_decomp(1)
    try:
        dq = lambda s: coracle.sharp_flux1(O.RP_ADVECTION_COLOR_1D, [0.0] * 8, 2, 1, 0, MBC, mx, wrap(s), auxbc, dx, dt)[0][:, MBC:-MBC]
        for _ in range(nsteps):
            q = M.ssp104(q, dq)
    finally:
        coracle.set_char_decomp(0)
    out = claw.frames[1].state.q
    assert np.isfinite(q).all() and not np.array_equal(q, state.q * 0)
    assert np.array_equal(out, q), np.abs(out - q).max()
