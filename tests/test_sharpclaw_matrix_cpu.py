"""
SharpClaw solver matrix, the part that needs no GPU: the host checks of ``SharpClawSolver.setup`` for the combinations
the kernels cover (p-system f-wave solver in 2-D; char_decomp = 1 with aux arrays and a capacity function in 1-D), and
the oracle-only anchors of tests/test_gpu_sharpclaw_fwave.py -- the inputs built here are the ones the GPU tests use,
so a fixture whose oracle result is not finite and non-zero, or a broken variable mapping, shows up here first.
"""
import numpy as np
import pytest

from oracle import oracle as O
from test_fwave import CC, K, RHO, ZZ, checkerboard_aux

MBC = 3
SHAPES = [(1, 1), (9, 5), (58, 58), (59, 57), (120, 75)]      # the shapes of test_flux2_euler_bitexact
TVD_MTHLIM = [4, 1, 2]                                        # lim_type 1: one limiter per component, all different


# ---- fixtures shared with the GPU tests ---------------------------------------------------------------------------
def psystem_inputs(mx, my, lin, capa):
    """q, aux (checkerboard medium as in test_hip_psystem_fwave, plus a capacity plane when asked), mcapa, dx, dy, dt"""
    rng = np.random.default_rng(1000 * mx + 10 * my + int(lin) + (5 if capa else 0))
    shape = (mx + 2 * MBC, my + 2 * MBC)
    aux = checkerboard_aux(shape, lin, rng)
    q = np.asfortranarray(0.3 * rng.standard_normal((3,) + shape))
    aux[3] = q[0]
    mcapa = 0
    if capa:
        aux = np.asfortranarray(np.concatenate([aux, (0.5 + rng.random(shape))[None]]))
        mcapa = 5
    dx, dy = 1.0 / mx, 0.9 / my
    return q, aux, mcapa, dx, dy, 0.3 * min(dx, dy) / 2.0


def psystem_oracle(coracle, lim, mx, my, q, aux, mcapa, dx, dy, dt):
    coracle.set_sharp_mthlim(TVD_MTHLIM)
    try:
        return coracle.sharp_flux2(O.RP_PSYSTEM_FWAVE_2D, [0.0], lim, 2, mcapa, MBC, mx, my, q, aux, dx, dy, dt)
    finally:
        coracle.set_sharp_mthlim([1] * 8)


def uniform_pair(mx, my):
    """acoustics state and its p-system twin in the uniform linear medium (rho, K) of test_fwave"""
    rng = np.random.default_rng(3)
    shape = (mx + 2 * MBC, my + 2 * MBC)
    p, u, v = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    qa = np.asfortranarray(np.stack([p, u, v]))
    qp = np.asfortranarray(np.stack([-p / K, RHO * u, RHO * v]))
    aux = checkerboard_aux(shape, 1.0, rng, hetero=False)
    aux[3] = qp[0]
    return qa, qp, aux


def state_1d_aux(rp, rng, n, capa):
    """q, rp_params, meqn, mwaves, aux, mcapa for the wave-based 1-D cases: the five solvers without aux arrays get one
    capacity plane; the colour equation a velocity of both signs in aux(1) and, when asked, a capacity plane after it"""
    if rp == O.RP_ADVECTION_COLOR_1D:
        q = np.asfortranarray(rng.standard_normal((1, n)))
        planes = [rng.standard_normal(n)]
        planes[0][n // 3:n // 3 + 4] = 0.0                       # a stagnant stretch: the speed is exactly zero
        if capa:
            planes.append(0.5 + rng.random(n))
        return q, [], 1, 1, np.asfortranarray(np.stack(planes)), 2 if capa else 0
    if rp == O.RP_EULER_1D:
        rho = 1 + 0.3 * rng.random(n); u = 0.6 * (rng.random(n) - .5); p = 1 + 0.3 * rng.random(n)
        rho[n // 2:] *= 0.4
        q, par, mw = np.asfortranarray(np.stack([rho, rho * u, p / 0.4 + 0.5 * rho * u * u])), [1.4, 0.4], 3
    elif rp == O.RP_SHALLOW_1D:
        h = 1 + 0.3 * rng.random(n); h[n // 3:] += 0.5
        q, par, mw = np.asfortranarray(np.stack([h, h * 0.4 * (rng.random(n) - .5)])), [9.81], 2
    elif rp == O.RP_ACOUSTICS_1D:
        q = rng.standard_normal((2, n)); q[:, n // 4:n // 4 + 9] = 0.25      # a constant stretch: waves of zero norm
        q, par, mw = np.asfortranarray(q), [1.0, 4.0, 2.0, 2.0], 2
    elif rp == O.RP_BURGERS_1D:
        q, par, mw = np.asfortranarray(rng.standard_normal((1, n))), [], 1
    else:
        q, par, mw = np.asfortranarray(rng.standard_normal((1, n))), [0.7], 1
    aux = np.asfortranarray((0.5 + rng.random(n))[None]) if capa else None
    return q, par, q.shape[0], mw, aux, 1 if capa else 0


WAVE_CASES = [(O.RP_ADVECTION_1D, True), (O.RP_ACOUSTICS_1D, True), (O.RP_BURGERS_1D, True), (O.RP_EULER_1D, True),
              (O.RP_SHALLOW_1D, True), (O.RP_ADVECTION_COLOR_1D, False), (O.RP_ADVECTION_COLOR_1D, True)]
WAVE_LIMS = [(2, 1), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5)]
WAVE_MX = [57, 58, 59, 333]


def wave_inputs(rp, capa, lim, mx):
    rng = np.random.default_rng(1000 * rp + mx + lim + (7 if capa else 0))
    return state_1d_aux(rp, rng, mx + 2 * MBC, capa) + (1.0 / mx, 0.2 / mx)


def wave_oracle(coracle, rp, par, lim, mth, mwaves, mcapa, mx, q, aux, dx, dt):
    coracle.set_char_decomp(1)
    coracle.set_sharp_mthlim([mth] * mwaves)
    try:
        return coracle.sharp_flux1(rp, par + [0.0] * (8 - len(par)), lim, mwaves, mcapa, MBC, mx, q, aux, dx, dt)
    finally:
        coracle.set_char_decomp(0)
        coracle.set_sharp_mthlim([1] * 8)


def ssp104(q, dq):
    """one SSP104 step with the formulas of pyclaw_amd/sharpclaw.py (step): dq(stage) -> deltaq"""
    s1 = q + dq(q) / 6.
    for _ in range(4):
        s1 = s1 + dq(s1) / 6.
    s2 = q / 25. + (9. / 25) * s1
    s1 = 15. * s2 - 5. * s1
    for _ in range(4):
        s1 = s1 + dq(s1) / 6.
    return s2 + 0.6 * s1 + 0.1 * dq(s1)


# ---- host checks of setup ------------------------------------------------------------------------------------------
def _setup_error(solver):
    """what setup(None) ends in: the checks come first, then the first touch of the (absent) solution"""
    try:
        solver.setup(None)
    except Exception as e:          # noqa: BLE001
        return e
    return None


@pytest.mark.parametrize("lim", [1, 2])
@pytest.mark.parametrize("rp", ["advection_color_1d", "advection_1d", "euler_1d"])
def test_setup_admits_wave_based_1d(rp, lim):
    import pyclaw_amd as pyclaw
    s = pyclaw.SharpClawSolver1D()
    s.char_decomp, s.lim_type = 1, lim
    s.rp = pyclaw.riemann.get(rp)
    s.mwaves = s.rp.mwaves
    assert not isinstance(_setup_error(s), NotImplementedError)


@pytest.mark.parametrize("lim", [1, 2, 3])
def test_setup_admits_psystem_2d(lim):
    import pyclaw_amd as pyclaw
    s = pyclaw.SharpClawSolver2D()
    s.rp, s.fwave, s.mwaves, s.lim_type = pyclaw.riemann.rp_psystem_fwave_2d, True, 2, lim
    assert not isinstance(_setup_error(s), NotImplementedError)


@pytest.mark.parametrize("ndim,attrs", [(2, {}), (1, {"lim_type": 3}), (1, {"weno_order": 7}), (1, {"fwave": True})])
def test_setup_keeps_refusing(ndim, attrs):
    import pyclaw_amd as pyclaw
    s = pyclaw.SharpClawSolver2D() if ndim == 2 else pyclaw.SharpClawSolver1D()
    s.char_decomp = 1
    s.rp = pyclaw.riemann.rp_acoustics_2d if ndim == 2 else pyclaw.riemann.rp_acoustics_1d
    s.mwaves = 2
    for k, v in attrs.items():
        setattr(s, k, v)
    with pytest.raises(NotImplementedError):
        s.setup(None)


# ---- oracle-only anchors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lim", [1, 2, 3])
def test_oracle_psystem_sharp_uniform_equals_acoustics(coracle, lim):
    """linear law, uniform medium: the p-system is acoustics (p = -K eps, (u, v) = m / rho); flux2 with the f-wave
    solver == flux2 with the reference-pinned acoustics solver, to the tolerance of
    test_oracle_psystem_linear_uniform_equals_acoustics"""
    mx, my = 40, 31
    qa, qp, aux = uniform_pair(mx, my)
    dx, dy, dt = 0.05, 0.06, 0.01
    coracle.set_sharp_mthlim(TVD_MTHLIM)
    try:
        ra, cfl_a = coracle.sharp_flux2(O.RP_ACOUSTICS_2D, [RHO, K, CC, ZZ], lim, 2, 0, MBC, mx, my, qa, None, dx, dy, dt)
        rp, cfl_p = coracle.sharp_flux2(O.RP_PSYSTEM_FWAVE_2D, [0.0], lim, 2, 0, MBC, mx, my, qp, aux, dx, dy, dt)
    finally:
        coracle.set_sharp_mthlim([1] * 8)
    inner = (slice(None), slice(MBC, -MBC), slice(MBC, -MBC))
    back = np.stack([-K * rp[0], rp[1] / RHO, rp[2] / RHO])
    assert np.abs(ra[inner]).max() > 0
    assert np.abs(back[inner] - ra[inner]).max() < 2e-14
    assert abs(cfl_a - cfl_p) < 2e-14


@pytest.mark.parametrize("mx,my", SHAPES)
@pytest.mark.parametrize("lin", [1.0, 2.0])
@pytest.mark.parametrize("capa", [False, True])
@pytest.mark.parametrize("lim", [1, 2, 3])
def test_oracle_psystem_inputs_are_sound(coracle, mx, my, lin, capa, lim):
    q, aux, mcapa, dx, dy, dt = psystem_inputs(mx, my, lin, capa)
    ref, cfl = psystem_oracle(coracle, lim, mx, my, q, aux, mcapa, dx, dy, dt)
    inner = (slice(None), slice(MBC, -MBC), slice(MBC, -MBC))
    assert np.isfinite(ref[inner]).all() and np.abs(ref[inner]).max() > 0 and 0 < cfl < np.inf


def test_oracle_psystem_capacity_matters(coracle):
    q, aux, mcapa, dx, dy, dt = psystem_inputs(9, 5, 1.0, True)
    with_capa, _ = psystem_oracle(coracle, 2, 9, 5, q, aux, mcapa, dx, dy, dt)
    without, _ = psystem_oracle(coracle, 2, 9, 5, q, aux, 0, dx, dy, dt)
    assert not np.array_equal(with_capa, without)


@pytest.mark.parametrize("rp,capa", WAVE_CASES)
@pytest.mark.parametrize("lim,mth", WAVE_LIMS)
@pytest.mark.parametrize("mx", WAVE_MX)
def test_oracle_wave_based_inputs_are_sound(coracle, rp, capa, lim, mth, mx):
    q, par, meqn, mwaves, aux, mcapa, dx, dt = wave_inputs(rp, capa, lim, mx)
    ref, cfl = wave_oracle(coracle, rp, par, lim, mth, mwaves, mcapa, mx, q, aux, dx, dt)
    assert np.isfinite(ref[:, MBC:-MBC]).all() and np.abs(ref[:, MBC:-MBC]).max() > 0 and 0 < cfl < np.inf
    if mcapa:
        other, _ = wave_oracle(coracle, rp, par, lim, mth, mwaves, 0, mx, q, aux, dx, dt)
        assert not np.array_equal(other[:, MBC:-MBC], ref[:, MBC:-MBC])


def test_psystem_app_checkerboard():
    """apps/psystem.py: both materials present in equal parts on a whole number of periods, the pulse inverts the
    stress law of each cell"""
    import pyclaw_amd as pyclaw
    from apps import psystem
    claw = psystem.psystem2D(pyclaw, 32, 24, solver_type='sharpclaw', lower=(0.0, 0.0), upper=(4.0, 3.0), bc='periodic',
                             linearity=2, amplitude=1.0, center=(2.0, 1.5), run=False)
    st = claw.solution.state
    assert st.aux.shape == (4, 32, 24) and claw.solver.fwave is True
    assert np.count_nonzero(st.aux[0] == 1.0) == np.count_nonzero(st.aux[0] == 4.0) == 32 * 24 // 2
    assert np.array_equal(st.aux[0], st.aux[1]) and (st.aux[2] == 2.0).all()
    assert st.aux[0, 0, 0] == 1.0 and st.aux[0, 4, 0] == 4.0 and st.aux[0, 0, 4] == 4.0 and st.aux[0, 4, 4] == 1.0
    sigma = np.exp(st.aux[1] * st.q[0]) - 1.0
    assert abs(sigma.max() - 1.0) < 0.05 and np.unravel_index(sigma.argmax(), sigma.shape) in [(15, 11), (15, 12), (16, 11), (16, 12)]
    assert not st.q[1:].any()
