"""
GPU: explicit Runge-Kutta schemes from a Butcher tableau in the SharpClaw solvers (time_integrator = 'RK', 'SSP22', 'RK44',
'DP5'): the stage registers, pcl_rk_take and the combination kernel (sharpclaw.hpp: rk_lincomb_kernel) under the Python
step, against the numpy restatement of the step on the oracle (tests/rk_reference.py) -- bit for bit in 'exact' mode,
every stage's Courant number included.
"""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rk_reference as RK
from apps import problems
from oracle import driver as D
from oracle import oracle as O
from pyclaw_amd import rk_tableaus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a user tableau with a zero inside a row, a zero weight and coefficients of exactly 1.0 (consistent, first order)
USER = dict(a=[[0., 0., 0., 0.], [1., 0., 0., 0.], [0.25, 0.25, 0., 0.], [0.5, 0., 0.5, 0.]],
            b=[1. / 6., 0., 2. / 3., 1. / 6.], c=[0., 1., 0.5, 1.])
EULER = dict(a=[[0.]], b=[1.], c=[0.])


def tableau(scheme):
    if isinstance(scheme, dict):
        return rk_tableaus.validate(scheme['a'], scheme['b'], scheme['c'])
    tab = rk_tableaus.TABLEAUS[scheme]
    return tab['a'], tab['b'], tab['c']


def set_scheme(solver, scheme):
    if isinstance(scheme, dict):
        solver.time_integrator = 'RK'
        solver.a, solver.b, solver.c = scheme['a'], scheme['b'], scheme['c']
    else:
        solver.time_integrator = scheme


# ---- the problems: the product's controller and the oracle driver's record of the same run ----------------------------------
def advection_1d(pyclaw, mx, custom_lower=False):
    solver = pyclaw.SharpClawSolver1D()
    solver.rp = pyclaw.riemann.rp_advection_1d
    solver.mwaves = 1
    solver.bc_lower[0] = pyclaw.BC.custom if custom_lower else pyclaw.BC.periodic
    solver.bc_upper[0] = pyclaw.BC.outflow if custom_lower else pyclaw.BC.periodic
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx)), 1)
    state.aux_global['u'] = 1.0
    xc = state.grid.x.center
    state.q[0, :] = np.sin(2 * np.pi * xc) + 0.5 * np.cos(4 * np.pi * xc)
    claw = pyclaw.Controller()
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    bcs = ([D.CUSTOM], [D.OUTFLOW]) if custom_lower else ([D.PERIODIC], [D.PERIODIC])
    p = D.Problem(q=state.q.copy('F'), d=(1.0 / float(mx),), rp=O.RP_ADVECTION_1D, rp_params=[1.0], mwaves=1, limiters=[1],
                  bc_lower=bcs[0], bc_upper=bcs[1], solver_type='sharpclaw', cfl_max=2.5, cfl_desired=2.45)
    return claw, p, 0.4 / mx


def acoustics_1d(pyclaw, mx):
    _, claw = problems.acoustics1D(pyclaw, mx=mx, solver_type='sharpclaw', run=False)
    p = D.acoustics1d_problem(mx=mx, solver_type='sharpclaw', cfl_max=2.5, cfl_desired=2.45)
    return claw, p, 0.4 / mx


def burgers_1d(pyclaw, mx):
    solver = pyclaw.SharpClawSolver1D()
    solver.rp = pyclaw.riemann.rp_burgers_1d
    solver.mwaves = 1
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx)), 1)
    xc = state.grid.x.center
    state.q[0, :] = 1.0 + 0.5 * np.sin(2 * np.pi * xc)
    claw = pyclaw.Controller()
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    p = D.Problem(q=state.q.copy('F'), d=(1.0 / float(mx),), rp=O.RP_BURGERS_1D, rp_params=[], mwaves=1, limiters=[1],
                  bc_lower=[D.PERIODIC], bc_upper=[D.PERIODIC], solver_type='sharpclaw', cfl_max=2.5, cfl_desired=2.45)
    return claw, p, 0.25 / mx


def acoustics_2d(pyclaw, mx=37, my=21):
    claw = problems.acoustics2D(pyclaw, mx=mx, my=my, solver_type='sharpclaw', run=False)
    p = D.acoustics2d_problem(mx=mx, my=my, solver_type='sharpclaw')
    return claw, p, p.dt_initial


MAKE = {"advection_1d": advection_1d, "acoustics_1d": acoustics_1d, "burgers_1d": burgers_1d}


def device_run(claw, scheme, dt, nsteps):
    """nsteps steps of the fixed length dt; returns (q, t, the Courant number of every stage in order)"""
    solver, solution = claw.solver, claw.solution
    set_scheme(solver, scheme)
    solver.dt_variable = False
    solver.setup(solution)
    seen = []
    solver.cfl._reduce = lambda v: (seen.append(v), v)[1]
    solver.dt = dt
    try:
        for n in range(nsteps):
            solver.evolve_to_time(solution)
    finally:
        solver.teardown()
    return solution.state.q.copy('F'), solution.t, seen


def reference_run(p, coracle, scheme, dt, nsteps, times=None):
    a, b, c = tableau(scheme)
    D.setup(p)
    p.dt = dt
    seen = []
    for n in range(nsteps):
        cfls = RK.rk_step(p, coracle, a, b, c, times=times)
        assert len(cfls) == len(b)
        seen += cfls
    return p.q, p.t, seen


# ---- 5: bit for bit against the restated step -------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ['RK44', 'DP5', USER], ids=['RK44', 'DP5', 'user'])
@pytest.mark.parametrize("problem", ["advection_1d", "acoustics_1d"])
def test_1d_step_equals_reference(coracle, problem, scheme):
    """mx = 61: 67 cells per component with their ghosts, an odd count, and register bases that are 8 but not 16 bytes
    aligned (lead = 13 doubles): the kernel's head and tail elements both carry cells"""
    import pyclaw_amd as pyclaw
    claw, p, dt = MAKE[problem](pyclaw, 61)
    q0 = p.q.copy()
    q, t, cfls = device_run(claw, scheme, dt, 3)
    qr, tr, cflr = reference_run(p, coracle, scheme, dt, 3)
    print("%s: max |device - reference| = %g, stages %d" % (problem, np.abs(q - qr).max(), len(cfls)))
    assert t == tr and len(cfls) == 3 * len(tableau(scheme)[1])
    assert cfls == cflr
    assert np.array_equal(q, qr)
    assert np.abs(qr - q0).max() > 1e-3


@pytest.mark.parametrize("scheme", ['RK44', 'DP5', USER], ids=['RK44', 'DP5', 'user'])
def test_2d_step_equals_reference(coracle, scheme):
    """37 x 21 acoustics, WENO5, mbc 3: the increments of the reference come from sharp_flux2"""
    import pyclaw_amd as pyclaw
    claw, p, dt = acoustics_2d(pyclaw)
    q0 = p.q.copy()
    q, t, cfls = device_run(claw, scheme, dt, 3)
    qr, tr, cflr = reference_run(p, coracle, scheme, dt, 3)
    assert t == tr and cfls == cflr
    assert np.array_equal(q, qr), np.abs(q - qr).max()
    assert np.abs(qr - q0).max() > 1e-3


def test_user_written_riemann_solver_under_a_tableau_scheme(coracle):
    """ACOUSTICS_1D_RP as a CellRiemann(sharpclaw=True) under RK44: the same reference, bit for bit"""
    import pyclaw_amd as pyclaw
    _, claw = problems.acoustics1D(pyclaw, mx=61, solver_type='sharpclaw', user_rp=True, run=False)
    p = D.acoustics1d_problem(mx=61, solver_type='sharpclaw', cfl_max=2.5, cfl_desired=2.45)
    q, t, cfls = device_run(claw, 'RK44', 0.4 / 61, 3)
    qr, tr, cflr = reference_run(p, coracle, 'RK44', 0.4 / 61, 3)
    assert t == tr and cfls == cflr
    assert np.array_equal(q, qr), np.abs(q - qr).max()


# ---- 6: the one-stage tableau is Euler --------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ["advection_1d", "acoustics_2d"])
def test_one_stage_tableau_gives_eulers_bits(problem):
    import pyclaw_amd as pyclaw

    def run(scheme):
        claw, p, dt = acoustics_2d(pyclaw) if problem == "acoustics_2d" else advection_1d(pyclaw, 61)
        return device_run(claw, scheme, dt / 4, 3), p.q
    (q, t, cfls), q0 = run(EULER)
    (qe, te, cfle), _ = run('Euler')
    assert t == te and cfls == cfle and len(cfls) == 3
    assert np.array_equal(q, qe) and np.abs(q - q0).max() > 0


# ---- 7: stage times reach the boundary conditions ---------------------------------------------------------------------------
def test_stage_times_reach_a_cell_bc(coracle):
    """A CellBC writes q = c.t into the lower ghost cells.  RK44 has c = (0, 1/2, 1/2, 1), so a step whose stages all saw t,
    or all t + dt, is another result: the reference evaluated with those times says so."""
    import pyclaw_amd as pyclaw
    claw, p, dt = advection_1d(pyclaw, 61, custom_lower=True)
    claw.solver.user_bc_lower = pyclaw.CellBC("q[0] = c.t;")

    def lower(idim, t, qbc, mbc):
        qbc[0, :mbc] = t
    p.user_bc_lower = lower
    q, t, cfls = device_run(claw, 'RK44', dt, 3)

    def ref(times):
        claw2, p2, _ = advection_1d(pyclaw, 61, custom_lower=True)
        p2.user_bc_lower = lower
        return reference_run(p2, coracle, 'RK44', dt, 3, times=times)
    qr, tr, cflr = ref(None)
    assert t == tr and cfls == cflr
    assert np.array_equal(q, qr), np.abs(q - qr).max()
    for name, wrong in (("t", lambda t, dt, i: t), ("t + dt", lambda t, dt, i: t + dt)):
        qw, _, _ = ref(wrong)
        print("stages at %s: max |difference| = %g" % (name, np.abs(qw - qr).max()))
        assert not np.array_equal(qw, q)


# ---- 8: sources -------------------------------------------------------------------------------------------------------------
DAMP = "for (int m = 0; m < MEQN; m++) dq[m] = -c.dt * p[0] * q[m];"


def test_sources_cell_python_and_reference_agree(coracle):
    """deltaq += -dt k q added by a CellDqSource on the device, by a Python dq_src through the host, and in the reference"""
    import pyclaw_amd as pyclaw
    k = 3.0

    def run(src):
        claw, p, dt = acoustics_1d(pyclaw, 61)
        claw.solver.dq_src = src
        return device_run(claw, 'RK44', dt, 3), p, dt
    (qc, tc, cflc), p, dt = run(pyclaw.CellDqSource(DAMP, params=[k]))
    (qp, tp, cflp), _, _ = run(lambda solver, state, dt: -dt * k * state.q)
    p.dq_src = lambda p, q, aux, dt: -dt * k * q
    qr, tr, cflr = reference_run(p, coracle, 'RK44', dt, 3)
    (q0, _, _), _, _ = run(None)
    assert tc == tp == tr and cflc == cflp == cflr
    assert np.array_equal(qc, qr), np.abs(qc - qr).max()
    assert np.array_equal(qp, qr), np.abs(qp - qr).max()
    assert np.abs(q0 - qr).max() > 1e-4              # the source is what the result shows


# ---- 9: rejection -----------------------------------------------------------------------------------------------------------
GROW = "for (int m = 0; m < MEQN; m++) dq[m] = c.dt * p[0] * q[m];"


def test_rejected_in_the_second_stage(coracle):
    """Burgers with a growing source: the second stage's Courant number is larger than the first's (the reference says by
    how much), cfl_max sits between them.  step() returns False, q on the device keeps its bits, half the dt is accepted."""
    import pyclaw_amd as pyclaw
    from pyclaw_amd import _lib
    k = 40.0
    a, b, c = tableau('RK44')
    claw, p, dt = burgers_1d(pyclaw, 61)
    p.dq_src = lambda p, q, aux, dt: dt * k * q
    D.setup(p)
    p.dt = dt
    q0 = p.q.copy()
    free = RK.rk_step(p, coracle, a, b, c)
    assert len(free) == 4 and free[1] > free[0] * 1.01
    cfl_max = 0.5 * (free[0] + free[1])

    solver, solution = claw.solver, claw.solution
    solver.time_integrator = 'RK44'
    solver.dq_src = pyclaw.CellDqSource(GROW, params=[k])
    solver.cfl_max, solver.cfl_desired = cfl_max, 0.9 * cfl_max
    solver.setup(solution)
    seen = []
    solver.cfl._reduce = lambda v: (seen.append(v), v)[1]
    try:
        solver.begin_resident(solution)
        solver.dt = dt
        assert solver.step(solution) is False
        assert seen == free[:2]
        on_device = np.empty(q0.shape, order='F')
        _lib.check(_lib.lib().pcl_get_q(solver._h, _lib.d(on_device), 0))
        assert np.array_equal(on_device, q0)
        solver.dt = dt / 2
        del seen[:]
        assert solver.step(solution) is not False
        solver.end_resident(solution)
    finally:
        solver.teardown()
    p.q, p.t, p.dt, p.cfl_max = q0, 0.0, dt / 2, cfl_max
    half = RK.rk_step(p, coracle, a, b, c)
    assert len(half) == 4 and seen == half and max(half) <= cfl_max
    assert np.array_equal(solution.state.q, p.q)


# ---- 10: resident mode and ranks --------------------------------------------------------------------------------------------
def test_resident_mode_gives_the_same_bytes():
    import pyclaw_amd as pyclaw

    def run(resident):
        claw, p, dt = acoustics_2d(pyclaw)
        solver, solution = claw.solver, claw.solution
        solver.time_integrator = 'RK44'
        solver.setup(solution)
        solver.dt = solver.dt_initial
        if resident:
            solver.begin_resident(solution)
        for tend in (0.02, 0.05):
            solver.evolve_to_time(solution, tend)
        if resident:
            solver.end_resident(solution)
        steps = solver.status['numsteps']
        solver.teardown()
        return solution.state.q.copy('F'), solution.t, steps
    q, t, n = run(False)
    qr, tr, nr = run(True)
    assert t == tr == 0.05 and n == nr and n >= 2
    assert q.tobytes() == qr.tobytes()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_ranks_give_the_single_blocks_bytes(tmp_path):
    """64 x 32 acoustics with RK44 to t = 0.04: two processes on this GPU, halo strips and the Courant maximum through the
    host (tests/rk_mp_worker.py), against the same run on one block"""
    import pyclaw_amd as pyclaw
    import rk_mp_worker as W
    claw = W.make_claw(pyclaw)
    claw.run()
    single = claw.frames[claw.nout].state.q
    assert claw.solver.status['numsteps'] >= 2
    out = str(tmp_path / "assembled.npy")
    port = free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port), "PCL_HALO_TRANSPORT": "host", "PCL_FORCE_DEVICE": "0",
                    "TORCHELASTIC_RUN_ID": "rk%d" % port})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "rk_mp_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for pr in procs:
            o, _ = pr.communicate(timeout=120)
            outs.append(o)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    codes = [pr.returncode for pr in procs]
    assert codes == [0, 0], "exit codes %s\n%s" % (codes, "\n----\n".join(o[-1500:] for o in outs))
    assert "2 distinct blocks" in outs[0], outs[0][-1500:]
    assembled = np.load(out)
    assert assembled.shape == single.shape and assembled.tobytes() == np.ascontiguousarray(single).tobytes()


# ---- 11: memory -------------------------------------------------------------------------------------------------------------
def held(solver):
    from pyclaw_amd import _lib
    n = C.c_int(-1)
    _lib.check(_lib.lib().pcl_rk_stages(solver._h, -1, C.byref(n)))
    return n.value


def test_stage_registers_exist_only_for_a_tableau_scheme():
    import pyclaw_amd as pyclaw
    claw, p, dt = acoustics_2d(pyclaw)
    solver, solution = claw.solver, claw.solution
    counts = []
    for ti in ('SSP104', 'DP5', 'SSP33', 'SSP22', 'Euler'):
        solver.time_integrator = ti
        solver.setup(solution)
        counts.append(held(solver))
        solver.teardown()
        assert solver._h is None
    assert counts == [0, 6, 0, 2, 0]


# ---- 12: the C entry points: the combination itself, and what they refuse ---------------------------------------------------
def make_handle(L, kind, n=(29,), meqn=2, math=0):
    cfg = L.Config()
    cfg.ndim = len(n)
    for k in range(len(n)):
        cfg.n[k], cfg.d[k] = n[k], 1.0 / n[k]
    cfg.mbc = 3 if kind else 2
    cfg.meqn, cfg.mwaves, cfg.rp = meqn, 2, (O.RP_ACOUSTICS_1D if len(n) == 1 else O.RP_ACOUSTICS_2D)
    cfg.method[1] = 2
    cfg.mthlim[0] = cfg.mthlim[1] = 4
    for k, v in enumerate([1.0, 1.0, 1.0, 1.0]):
        cfg.rp_params[k] = v
    cfg.kind, cfg.lim_type, cfg.math = kind, 2 * kind, math
    h = C.c_void_p()
    L.check(L.lib().pcl_create(C.byref(cfg), C.byref(h)))
    return h


def put(L, h, reg, arr):
    L.check(L.lib().pcl_select(h, reg))
    L.check(L.lib().pcl_put_q(h, L.d(arr), 1))
    L.check(L.lib().pcl_select(h, 0))


def get(L, h, reg, shape):
    out = np.empty(shape, order='F')
    L.check(L.lib().pcl_select(h, reg))
    L.check(L.lib().pcl_get_q(h, L.d(out), 1))
    L.check(L.lib().pcl_select(h, 0))
    return out


def lincomb(L, h, Dr, Ar, stages, coef):
    st = np.array(stages, dtype=np.int32)
    cf = np.array(coef, dtype=np.float64)
    return L.lib().pcl_rk_lincomb(h, Dr, Ar, len(stages), L.i(st), L.d(cf))


@pytest.mark.parametrize("n", [(29,), (61,), (37, 21)], ids=str)
@pytest.mark.parametrize("math", [0, 1], ids=['exact', 'fast'])
def test_combination_kernel_against_numpy(n, math):
    """pcl_rk_lincomb with 0, 1, 4, 6 and 16 terms, D another register and D == A, against the left-to-right sum in numpy:
    equal bits in 'exact'; in 'fast' (products may be fused into the sums: each step's rounding error is at most the
    unfused one's, eps/2 |partial sum| + eps/2 |product|) within (n + 1) eps sum|terms|.  A register whose coefficient is
    0.0 holds NaN and is not read."""
    from pyclaw_amd import _lib as L
    rng = np.random.default_rng(len(n) * 100 + n[0])
    shape = (2 if len(n) == 1 else 3,) + tuple(k + 6 for k in n)
    h = make_handle(L, 1, n, meqn=shape[0], math=math)
    try:
        got = C.c_int()
        L.check(L.lib().pcl_rk_stages(h, 16, C.byref(got)))
        assert got.value == 16
        K = [np.asfortranarray(rng.standard_normal(shape)) for j in range(16)]
        for j in range(16):
            put(L, h, 3, K[j])
            L.check(L.lib().pcl_rk_take(h, j))
        q, s1 = (np.asfortranarray(rng.standard_normal(shape)) for _ in range(2))
        put(L, h, 0, q)
        put(L, h, 1, s1)
        for nterms in (0, 1, 4, 6, 16):
            stages = list(rng.permutation(16)[:nterms])
            coef = list(rng.standard_normal(nterms))
            if nterms >= 4:
                coef[1] = 1.0
            want, mag = q, np.abs(q)
            for j, cj in zip(stages, coef):
                want = want + cj * K[j]
                mag = mag + np.abs(cj * K[j])
            L.check(lincomb(L, h, 2, 0, stages, coef))           # S2 = Q + ...
            L.check(lincomb(L, h, 1, 1, stages, coef))           # S1 += ..., in place
            a, b = get(L, h, 2, shape), get(L, h, 1, shape)
            want1 = s1
            for j, cj in zip(stages, coef):
                want1 = want1 + cj * K[j]
            if math == 0:
                assert np.array_equal(a, want) and np.array_equal(b, want1), nterms
            else:
                tol = (nterms + 1) * np.finfo(float).eps * mag
                assert (np.abs(a - want) <= tol).all(), nterms
            s1 = b
            assert np.array_equal(get(L, h, 0, shape), q)
        # a zero coefficient: the register is not read
        put(L, h, 3, np.full(shape, np.nan, order='F'))
        L.check(L.lib().pcl_rk_take(h, 5))
        L.check(lincomb(L, h, 2, 0, [4, 5, 6], [0.5, 0.0, 1.0]))
        want = (q + 0.5 * K[4]) + 1.0 * K[6]
        a = get(L, h, 2, shape)
        if math == 0:
            assert np.array_equal(a, want)
        else:
            assert np.isfinite(a).all() and np.abs(a - want).max() < 1e-14
    finally:
        L.lib().pcl_destroy(h)


def test_entry_points_refuse_and_leave_the_state_alone():
    from pyclaw_amd import _lib as L
    lib = L.lib()
    one = np.array([1.0])
    # a classic solver
    h = make_handle(L, 0)
    try:
        n = C.c_int(-1)
        assert lib.pcl_rk_stages(h, 2, C.byref(n)) == L.ESTATE and b"classic solver" in lib.pcl_last_error()
        assert n.value == 0
        assert lib.pcl_rk_take(h, 0) == L.ESTATE and b"classic solver" in lib.pcl_last_error()
        assert lincomb(L, h, 0, 0, [0], one) == L.ESTATE and b"classic solver" in lib.pcl_last_error()
    finally:
        lib.pcl_destroy(h)
    h = make_handle(L, 1)
    try:
        rng = np.random.default_rng(5)
        shape = (2, 35)
        regs = {r: np.asfortranarray(rng.standard_normal(shape)) for r in (0, 1, 2, 3)}
        for r, v in regs.items():
            put(L, h, r, v)
        # before the registers exist
        assert lincomb(L, h, 1, 0, [0], one) == L.ESTATE and b"no stage registers" in lib.pcl_last_error()
        assert lib.pcl_rk_take(h, 0) == L.ESTATE and b"no stage registers" in lib.pcl_last_error()
        n = C.c_int(-1)
        L.check(lib.pcl_rk_stages(h, 2, C.byref(n)))
        assert n.value == 2
        assert lib.pcl_rk_stages(h, 17, C.byref(n)) == L.EINVAL and b"17 stages" in lib.pcl_last_error()
        for bad in (2, -1, 16):
            assert lib.pcl_rk_take(h, bad) == L.EINVAL and b"pcl_rk_take: stage" in lib.pcl_last_error()
            assert lincomb(L, h, 1, 0, [0, bad], [1.0, 1.0]) == L.EINVAL and b"pcl_rk_lincomb: stage" in lib.pcl_last_error()
        assert lincomb(L, h, 1, 0, [0] * 17, [1.0] * 17) == L.EINVAL and b"17 terms" in lib.pcl_last_error()
        assert lincomb(L, h, L.REG_K0 + 1, 0, [0, 1], [1.0, 1.0]) == L.EINVAL and b"D is one of the inputs" in lib.pcl_last_error()
        for Dr, Ar in ((3, 0), (0, 4), (-1, 0), (L.REG_K0, 0), (1, 7)):
            assert lincomb(L, h, Dr, Ar, [1], one) == L.EINVAL and b"must be q, s1 or s2" in lib.pcl_last_error()
        assert lincomb(L, h, 1, 0, [0], [float('nan')]) == L.EINVAL and b"not finite" in lib.pcl_last_error()
        assert lib.pcl_rk_lincomb(h, 1, 0, 1, None, None) == L.EINVAL
        L.check(lib.pcl_rk_stages(h, -1, C.byref(n)))
        assert n.value == 2
        for r, v in regs.items():
            assert np.array_equal(get(L, h, r, shape), v), r
        # and the stage registers still hold their zeros: Q + K_0 + K_1 is Q
        L.check(lincomb(L, h, 2, 0, [0, 1], [1.0, 1.0]))
        assert np.array_equal(get(L, h, 2, shape), regs[0] + 0.0)
        L.check(lib.pcl_rk_stages(h, 0, C.byref(n)))
        assert n.value == 0
    finally:
        lib.pcl_destroy(h)
