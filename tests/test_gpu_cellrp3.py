"""
GPU: user-written Riemann solvers in the dimension-split 3-D step (pyclaw.CellRiemann3D, pcl_cellrp_compile3; DESIGN.md
4.4d).  The library compiles the three passes of its own 3-D sweep kernel around the body, so the built-in solver restated
as a body (apps/problems.py: VC_ACOUSTICS_3D_RP) must give the bits of the frozen oracle -- per sweep and per step, with a
capacity function, on flat stretches where the jump-free shortcut takes the body's speeds, and through the public
interface against the same run with the built-in solver.  Systems the library has no 3-D solver for: homogeneous acoustics
from parameters (the oracle's solver over constant aux arrays), Burgers against a numpy Godunov update on dyadic data
(exact), advection and Euler by the permutation symmetry of the three sweeps (exact), Euler at first order against the
numpy restatement of its Roe formulas (the project's relative gate).  'exact' arithmetic and equalities unless said
otherwise.  Shapes: the smallest that cross every tile seam of the kernel -- 60 cells along a strip, 16 columns across,
4 rows and 240 cells in the x tile.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyclaw_amd as pyclaw
from apps import problems
from oracle import oracle as O
from pyclaw_amd import _lib as L
from test_cellrp3_cpu import euler_roe

PCL_RP_CELL = 100
GATE = 1e-12        # the project's relative gate (tests/test_gpu_cellrp.py: test_fast_mode_is_within_the_projects_gate_of_exact)
D3 = (0.1, 0.07, 0.13)


def stats():
    n, h = C.c_long(), C.c_long()
    L.check(L.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


class Handle3(object):
    """a 3-D PCL_RP_CELL solver handle created around `body` (pcl_create_cellrp), mbc = 2"""

    def __init__(self, body, meqn, mwaves, shape, d, order, mthlim, maux=0, aux=(), mcapa=0, params=(), math=0):
        self.rp = pyclaw.CellRiemann3D(body, meqn, mwaves, params=params, aux=aux, capa=mcapa > 0)
        self.rp.compile(['exact', 'fast', 'strict'][math])
        cfg = L.Config()
        cfg.ndim = 3
        for k in range(3):
            cfg.n[k] = shape[k]
            cfg.d[k] = d[k]
        cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, meqn, mwaves, maux
        for k, v in enumerate([1, order, -1, 0, 0, mcapa, maux]):
            cfg.method[k] = v
        for k, m in enumerate(mthlim):
            cfg.mthlim[k] = m
        for k, v in enumerate(params):
            cfg.rp_params[k] = v
        cfg.rp = PCL_RP_CELL
        cfg.math = math
        self.h = C.c_void_p()
        L.check(L.lib().pcl_create_cellrp(C.byref(cfg), self.rp._rp, C.byref(self.h)))

    def put_aux(self, aux):
        assert aux.flags.f_contiguous
        L.check(L.lib().pcl_put_aux(self.h, L.d(aux)))
        return self

    def _run(self, q0, call):
        lib = L.lib()
        cfl = C.c_double()
        assert q0.flags.f_contiguous
        L.check(lib.pcl_put_q(self.h, L.d(q0), 1))
        L.check(call(lib, C.cast(C.byref(cfl), L.dp)))
        out = np.empty_like(q0, order="F")
        L.check(lib.pcl_get_q(self.h, L.d(out), 1))
        return out, cfl.value

    def sweep(self, q0, ids, dt):
        """one pass over q0 (ghost cells included); returns the new array with ghosts and the Courant number"""
        return self._run(q0, lambda lib, cfl: lib.pcl_sweep(self.h, ids, dt, cfl))

    def step(self, q0, dt):
        return self._run(q0, lambda lib, cfl: lib.pcl_step_hyperbolic(self.h, dt, cfl))

    def close(self):
        L.lib().pcl_destroy(self.h)
        self.h = None


def vc_state(rng, shape, maux=2, mbc=2):
    """q standard normal; aux: impedance in [0.5, 2.5], sound speed in [0.5, 2], then (maux = 3) a capacity function in [0.5, 1.5]"""
    full = tuple(n + 2 * mbc for n in shape)
    q = np.asfortranarray(rng.standard_normal((4,) + full))
    aux = np.empty((maux,) + full, order="F")
    aux[0] = 0.5 + 2.0 * rng.random(full)
    aux[1] = 0.5 + 1.5 * rng.random(full)
    if maux > 2:
        aux[2] = 0.5 + rng.random(full)
    return q, aux


def oracle_sweep(coracle, q, aux, shape, dt, method, mthlim, idir, d=D3):
    want = q.copy("F")
    _, cfl = coracle.step3ds(O.RP_VC_ACOUSTICS_3D, max(shape), 2, shape[0], shape[1], shape[2], q.copy("F"), want, aux,
                             d[0], d[1], d[2], dt, method, np.array(mthlim, dtype=np.int32), idir)
    return want, cfl


def oracle_step(coracle, q, aux, shape, dt, method, mthlim, d=D3):
    """x, y, z in turn; the largest of the three Courant numbers"""
    cur, cfls = q, []
    for idir in (1, 2, 3):
        cur, c = oracle_sweep(coracle, cur, aux, shape, dt, method, mthlim, idir, d)
        cfls.append(c)
    return cur, max(cfls)


SHAPES = [(1, 1, 1), (9, 7, 5), (70, 20, 3), (5, 66, 4), (6, 3, 130), (245, 3, 2)]
SCHEMES = [(2, [4, 4]), (2, [1, 3]), (1, [4, 4])]


# ---- 1. the restated solver against the frozen oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("order,lims", SCHEMES)
def test_restated_solver_sweeps_equal_the_oracle(coracle, shape, order, lims):
    rng = np.random.default_rng(100 * order + shape[0] + lims[0])
    q, aux = vc_state(rng, shape)
    method = np.array([1, order, -1, 0, 0, 0, 2], dtype=np.int32)
    dt = 0.02
    hd = Handle3(problems.VC_ACOUSTICS_3D_RP, 4, 2, shape, D3, order, lims, maux=2, aux=(0, 1)).put_aux(aux)
    try:
        for idir in (1, 2, 3):
            want, cfl_o = oracle_sweep(coracle, q, aux, shape, dt, method, lims, idir)
            got, cfl = hd.sweep(q, idir, dt)
            assert cfl == cfl_o and cfl > 0, (idir, cfl, cfl_o)
            assert np.array_equal(got, want), (idir, np.abs(got - want).max())       # ghost cells included
            assert not np.array_equal(got, q)
    finally:
        hd.close()


@pytest.mark.parametrize("shape", [(70, 20, 3), (6, 3, 130)])
@pytest.mark.parametrize("order,lims", SCHEMES)
def test_restated_solver_step_equals_the_oracle(coracle, shape, order, lims):
    rng = np.random.default_rng(7 * order + shape[1])
    q, aux = vc_state(rng, shape)
    method = np.array([1, order, -1, 0, 0, 0, 2], dtype=np.int32)
    dt = 0.02
    want, cfl_o = oracle_step(coracle, q, aux, shape, dt, method, lims)
    hd = Handle3(problems.VC_ACOUSTICS_3D_RP, 4, 2, shape, D3, order, lims, maux=2, aux=(0, 1)).put_aux(aux)
    try:
        got, cfl = hd.step(q, dt)
    finally:
        hd.close()
    assert cfl == cfl_o and np.array_equal(got, want), np.abs(got - want).max()


# ---- 2. with a capacity function -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 7, 5), (70, 20, 3), (6, 3, 130)])
def test_capacity_function_equals_the_oracle(coracle, shape):
    """the set-up of test_step3ds_capacity_function_equals_oracle (tests/test_gpu_classic3d.py): maux 3, mcapa 3"""
    rng = np.random.default_rng(300 + shape[1])
    q, aux = vc_state(rng, shape, maux=3)
    method = np.array([1, 2, -1, 0, 0, 3, 3], dtype=np.int32)
    lims = [4, 3]
    dt = 0.012
    hd = Handle3(problems.VC_ACOUSTICS_3D_RP, 4, 2, shape, D3, 2, lims, maux=3, aux=(0, 1), mcapa=3).put_aux(aux)
    try:
        for idir in (1, 2, 3):
            want, cfl_o = oracle_sweep(coracle, q, aux, shape, dt, method, lims, idir)
            got, cfl = hd.sweep(q, idir, dt)
            assert cfl == cfl_o and cfl > 0, idir
            assert np.array_equal(got, want) and not np.array_equal(got, q), (idir, np.abs(got - want).max())
            # the capacity function matters: the same sweep without it gives something else
            m0 = method.copy()
            m0[5] = 0
            plain, _ = oracle_sweep(coracle, q, aux, shape, dt, m0, lims, idir)
            assert not np.array_equal(plain, want)
        want, cfl_o = oracle_step(coracle, q, aux, shape, dt, method, lims)
        got, cfl = hd.step(q, dt)
        assert cfl == cfl_o and np.array_equal(got, want)
    finally:
        hd.close()


# ---- 3. flat stretches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idir", [1, 2, 3])
def test_flat_q_inside_noisy_aux_takes_the_speeds_of_the_body(coracle, idir):
    """130 cells along the sweep, q constant from array index 56 on in every line and noisy in front of it, aux noisy
    everywhere: the strip of cells 60..123 of every line is one wavefront without a jump, which takes speeds() -- the body
    again, every interface with its own auxl / auxr.  The largest sound speed sits in that stretch, so the Courant number
    comes out right only through that path."""
    shape = [6, 5, 4]
    shape[idir - 1] = 130
    shape = tuple(shape)
    rng = np.random.default_rng(40 + idir)
    q, aux = vc_state(rng, shape)
    along = [slice(None)] * 4
    along[idir] = slice(56, None)
    for m in range(4):
        idx = list(along)
        idx[0] = m
        q[tuple(idx)] = 0.25 * (m + 1)
    cell = [3, 3, 3]
    cell[idir - 1] = 100
    aux[(1,) + tuple(cell)] = 3.0                   # the rest is below 2
    assert np.unravel_index(np.argmax(aux[1]), aux[1].shape) == tuple(cell) and 60 <= 100 < 124 and 56 <= 60
    method = np.array([1, 2, -1, 0, 0, 0, 2], dtype=np.int32)
    dt = 0.01
    for lims in ([4, 4], [1, 3]):
        want, cfl_o = oracle_sweep(coracle, q, aux, shape, dt, method, lims, idir)
        hd = Handle3(problems.VC_ACOUSTICS_3D_RP, 4, 2, shape, D3, 2, lims, maux=2, aux=(0, 1)).put_aux(aux)
        try:
            got, cfl = hd.sweep(q, idir, dt)
        finally:
            hd.close()
        assert cfl == cfl_o and cfl == pytest.approx(dt / D3[idir - 1] * 3.0, rel=1e-14)
        assert np.array_equal(got, want), np.abs(got - want).max()
        flat = tuple(slice(62, 120) if k == idir else slice(None) for k in range(4))
        assert np.array_equal(got[flat], q[flat])


# ---- 4. a solver from parameters, no aux ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (9, 7, 5), (70, 20, 3), (6, 3, 130)])
def test_homogeneous_acoustics_equals_the_oracles_solver_over_constant_aux(coracle, shape):
    rng = np.random.default_rng(11 + shape[2])
    q, aux = vc_state(rng, shape)
    zz, cc = 1.75, 1.25
    aux[0], aux[1] = zz, cc
    method = np.array([1, 2, -1, 0, 0, 0, 2], dtype=np.int32)
    lims = [4, 4]
    dt = 0.02
    hd = Handle3(problems.ACOUSTICS_3D_RP, 4, 2, shape, D3, 2, lims, maux=0, params=[zz, cc])
    try:
        for idir in (1, 2, 3):
            want, cfl_o = oracle_sweep(coracle, q, aux, shape, dt, method, lims, idir)
            got, cfl = hd.sweep(q, idir, dt)
            assert cfl == cfl_o and cfl > 0 and np.array_equal(got, want), (idir, np.abs(got - want).max())
        want, cfl_o = oracle_step(coracle, q, aux, shape, dt, method, lims)
        got, cfl = hd.step(q, dt)
        assert cfl == cfl_o and np.array_equal(got, want)
    finally:
        hd.close()


# ---- 5. the public interface ---------------------------------------------------------------------------------------------------
def traced(solver):
    """(dt, Courant number) of every hyperbolic step, rejected ones included"""
    log, inner = [], solver.step_hyperbolic

    def step_hyperbolic(solution):
        inner(solution)
        log.append((solver.dt, solver.cfl.get_cached_max()))
    solver.step_hyperbolic = step_hyperbolic
    return log


def small_claw(user, mixed_bcs=False):
    claw = problems.acoustics3D(pyclaw, mx=30, my=6, mz=5, tfinal=0.3, nout=3, run=False, user_rp=user)
    rng = np.random.default_rng(5)
    st = claw.solution.state
    st.q[1:] = 0.1 * rng.standard_normal(st.q[1:].shape)
    st.aux[0] = 1.0 + rng.random(st.aux[0].shape)
    st.aux[1] = 0.5 + rng.random(st.aux[1].shape)
    if mixed_bcs:
        for k in range(3):
            claw.solver.bc_lower[k] = claw.solver.aux_bc_lower[k] = pyclaw.BC.reflecting
            claw.solver.bc_upper[k] = claw.solver.aux_bc_upper[k] = pyclaw.BC.outflow
    return claw


@pytest.mark.parametrize("mixed_bcs", [False, True])
def test_claw_solver_3d_equals_the_built_in_run(mixed_bcs):
    """dt_initial = 0.1 on cells of 1/15: the first step is rejected (Courant number above cfl_max) and retaken -- with the
    same bits, or the logs below would differ"""
    runs = []
    for user in (False, True):
        claw = small_claw(user, mixed_bcs)
        log = traced(claw.solver)
        claw.run()
        runs.append((claw, log))
    (ref, log_ref), (got, log) = runs
    assert log_ref[0][1] > ref.solver.cfl_max and log_ref[1][0] < log_ref[0][0]        # a rejected step, retaken with a smaller dt
    assert log == log_ref and len(log) > 6
    assert got.solver.status['numsteps'] == ref.solver.status['numsteps'] >= 1      # (of the last output interval)
    assert got.solver.status['cflmax'] == ref.solver.status['cflmax']
    assert len(got.frames) == len(ref.frames) == 4
    for f, g in zip(ref.frames, got.frames):
        assert np.array_equal(f.state.q, g.state.q)
    assert not np.array_equal(got.frames[-1].state.q, got.frames[0].state.q)


def homogeneous_claw(user, zz, cc):
    claw = problems.acoustics3D(pyclaw, mx=30, my=6, mz=5, run=False)
    st = claw.solution.state
    st.q[1:] = 0.1 * np.random.default_rng(6).standard_normal(st.q[1:].shape)
    st.aux[0], st.aux[1] = zz, cc
    if user:
        claw.solver.rp = pyclaw.CellRiemann3D(problems.ACOUSTICS_3D_RP, 4, 2, params=[zz, cc])
        claw.solution = pyclaw.Solution(pyclaw.State(st.grid, 4))
        claw.solution.state.q[...] = st.q
    claw.solver.dt_initial = 0.02
    return claw


def test_params_reassigned_mid_run_compile_nothing():
    """impedance and sound speed change behind step 3.  The built-in solver reads them from aux: its run is set up again
    there on the state it has reached, with the aux arrays changed alike."""
    old, new = (1.0, 1.0), (1.5, 1.75)
    claw = homogeneous_claw(False, *old)
    solver, solution = claw.solver, claw.solution
    log_ref = traced(solver)
    solver.setup(solution)
    solver.dt = solver.dt_initial
    for k in range(3):
        solver.evolve_to_time(solution)
    solution.state.aux[0], solution.state.aux[1] = new
    solver.setup(solution)                # (evolve_to_time has brought q back to the host; dt is kept)
    for k in range(3):
        solver.evolve_to_time(solution)
    q_ref = solution.state.q.copy()
    solver.teardown()

    claw = homogeneous_claw(True, *old)
    solver, solution = claw.solver, claw.solution
    solver.rp.compile()                   # whatever this process compiled before: the counts start behind it
    n0 = stats()[0]
    log = traced(solver)
    solver.setup(solution)
    solver.dt = solver.dt_initial
    for k in range(6):
        if k == 3:
            solver.rp.params = new
        solver.evolve_to_time(solution)
    q = solution.state.q.copy()
    solver.teardown()
    assert stats()[0] == n0
    assert len(log) >= 6 and log == log_ref and np.array_equal(q, q_ref)
    assert log[3][1] != log[2][1]


# ---- 6. a system the library lacks, at first order: exact ----------------------------------------------------------------------
def burgers_fluctuations(ql, qr):
    """BURGERS_3D_RP in numpy, any float type"""
    half = ql.dtype.type(0.5)
    wave = qr - ql
    s = half * (ql + qr)
    transonic = (qr > 0) & (ql < 0)
    amdq = np.where(transonic, -half * (ql * ql), np.minimum(s, 0) * wave)
    apdq = np.where(transonic, half * (qr * qr), np.maximum(s, 0) * wave)
    return np.abs(s), amdq, apdq


def godunov_pass3(q, axis, dtd, fluct, mbc=2):
    """first-order update along `axis` (0..2) of q (meqn, I, J, K): the interior cells of every line whose two transverse
    indices lie within one ghost layer of the interior (step3ds.f:110-111), the other cells copied through.  fluct(ql, qr,
    ixy) -> (largest |speed| per interface, amdq, apdq).  Returns the new array and the Courant number over the interfaces
    1..m+1 of the swept lines."""
    qm = np.moveaxis(q, axis + 1, 1)
    m = qm.shape[1] - 2 * mbc
    ql, qr = qm[:, mbc - 1:mbc + m], qm[:, mbc:mbc + m + 1]           # interfaces mbc .. mbc+m: between cells i-1 and i
    smax, amdq, apdq = fluct(ql, qr, axis + 1)
    upd = qm[:, mbc:mbc + m] - dtd * apdq[:, :-1] - dtd * amdq[:, 1:]
    t1, t2 = slice(mbc - 1, qm.shape[2] - mbc + 1), slice(mbc - 1, qm.shape[3] - mbc + 1)
    new = qm.copy()
    new[:, mbc:mbc + m, t1, t2] = upd[:, :, t1, t2]
    return np.moveaxis(new, 1, axis + 1), (dtd * smax[:, t1, t2]).max()


def godunov_step3(q, dtd, fluct):
    cur, cfls = q, []
    for axis in range(3):
        cur, c = godunov_pass3(cur, axis, dtd, fluct)
        cfls.append(c)
    return cur, max(cfls)


@pytest.mark.parametrize("shape", [(7, 5, 3), (61, 18, 5)])
def test_burgers_3d_against_a_numpy_godunov_update(shape):
    """q integer multiples of 1/8 in [-2, 2] of both signs, dt/d = 1/4 in every direction: every product and sum of the
    first-order step is exact in double precision whatever the order of operations, which the long-double recomputation
    below verifies; the comparison with the device is then an equality."""
    rng = np.random.default_rng(shape[0])
    q0 = rng.integers(-16, 17, size=(1,) + tuple(n + 4 for n in shape)).astype(np.float64) / 8.0
    assert (q0 > 0).any() and (q0 < 0).any()

    def fluct1(ql, qr, ixy):
        s, a, b = burgers_fluctuations(ql[0], qr[0])
        return s, a[None], b[None]
    ref, cfl_ref = godunov_step3(q0, 0.25, fluct1)
    refl, cfll = godunov_step3(q0.astype(np.longdouble), np.longdouble(0.25), fluct1)
    assert np.array_equal(ref.astype(np.longdouble), refl) and np.longdouble(cfl_ref) == cfll
    d = 1.0 / 64
    hd = Handle3(problems.BURGERS_3D_RP, 1, 1, shape, (d, d, d), 1, [0])
    try:
        out, cfl = hd.step(np.asfortranarray(q0), 0.25 * d)
    finally:
        hd.close()
    assert np.array_equal(out, ref), np.abs(out - ref).max()
    assert cfl == cfl_ref and not np.array_equal(out, q0)


# ---- 7. permutation symmetry at second order: exact ----------------------------------------------------------------------------
def laid_along(axis, profile, across):
    """profile (meqn, 70) along `axis`, constant across the other two axes, whose cell counts in cyclic order are `across`"""
    cells = [0, 0, 0]
    cells[axis], cells[(axis + 1) % 3], cells[(axis + 2) % 3] = profile.shape[1], across[0], across[1]
    shape = [1, 1, 1]
    shape[axis] = profile.shape[1]
    q = np.empty((profile.shape[0],) + tuple(cells))
    q[...] = profile.reshape((profile.shape[0],) + tuple(shape))
    return q


def profile_of(q, axis):
    """the profile along `axis` of a field that is constant across the other two, which is asserted"""
    qa = np.moveaxis(q, axis + 1, 1)
    assert np.array_equal(qa, np.broadcast_to(qa[:, :, :1, :1], qa.shape))
    return qa[:, :, 0, 0].copy()


def run_five_steps(rp, q0, mwaves):
    solver = pyclaw.ClawSolver3D()
    solver.rp = rp
    solver.dim_split = True
    solver.order = 2
    solver.mwaves = mwaves
    solver.limiters = [4] * mwaves
    for k in range(3):
        solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.outflow
    d = 1.0 / 64
    dims = [pyclaw.Dimension(n, 0.0, q0.shape[k + 1] * d, q0.shape[k + 1]) for k, n in enumerate("xyz")]
    state = pyclaw.State(pyclaw.Grid(dims), q0.shape[0])
    state.q[...] = q0
    solution = pyclaw.Solution(state)
    log = traced(solver)
    solver.dt_initial = 0.2 * d
    solver.setup(solution)
    solver.dt = solver.dt_initial
    for k in range(5):
        solver.evolve_to_time(solution)
    q = solution.state.q.copy()
    solver.teardown()
    return q, log


# cells across the axis the field lies along, in cyclic order behind it: (70, 5, 4), (5, 70, 4) and (5, 4, 70)
ACROSS = {0: (5, 4), 1: (4, 5), 2: (5, 4)}


def test_euler_3d_is_symmetric_under_permutations_of_the_axes():
    """Sod's jump plus a smooth perturbation in density, pressure and the normal velocity along one axis; the other two
    momenta are zero.  (With all three momenta in play the results agree to rounding only: the limiter's dot products sum
    over the components in index order, whatever the body's roles, and a permutation reorders five non-zero terms.  With
    two of them zero the non-zero terms keep their order.)  Every sweep meets the numbers another sweep meets in the other
    two runs, in the roles (normal, next, last) the body gives them, so the three results are one profile, bit for bit.
    The sweeps across the field are the identity on q (every line is constant), but they come before the sweep along it in one run and behind it in another, so their Courant numbers are taken of different states: the step's
    Courant number is the same in the three runs because the sweep along the field sets it, its largest speed being a
    quarter above anything the other two meet (asserted on the initial state; five small steps do not close that gap)."""
    n = 70
    x = (np.arange(n) + 0.5) / n
    rho = np.where(x < 0.5, 1.0, 0.125) + 0.05 * np.sin(6.0 * np.pi * x)
    pres = np.where(x < 0.5, 1.0, 0.1) + 0.02 * np.cos(4.0 * np.pi * x)
    vel = (0.6 + 0.3 * np.sin(2.0 * np.pi * x), 0.0, 0.0)          # normal, next and last in cyclic order
    sound = np.sqrt(1.4 * pres / rho)
    assert (np.abs(vel[0]) + sound).max() > 1.25 * sound.max()
    mom = [rho * v for v in vel]
    energy = pres / 0.4 + 0.5 * rho * sum(v * v for v in vel)
    results = []
    for axis in range(3):
        prof = np.empty((5, n))
        prof[0], prof[4] = rho, energy
        for k in range(3):
            prof[1 + (axis + k) % 3] = mom[k]
        rp = pyclaw.CellRiemann3D(problems.EULER_3D_RP, 5, 3, params=[1.4])
        q0 = laid_along(axis, prof, ACROSS[axis])
        assert q0.shape[1:] == [(70, 5, 4), (5, 70, 4), (5, 4, 70)][axis]
        q, log = run_five_steps(rp, q0, 3)
        out = profile_of(q, axis)
        # back to the roles: density, the three momenta in cyclic order from the axis, energy
        results.append((np.stack([out[0]] + [out[1 + (axis + k) % 3] for k in range(3)] + [out[4]]), log, prof))
    (qx, logx, prof), (qy, logy, _), (qz, logz, _) = results
    assert len(logx) == 5 and logx == logy == logz
    assert np.array_equal(qx, qy) and np.array_equal(qx, qz)
    start = np.stack([prof[0], prof[1], prof[2], prof[3], prof[4]])
    assert not np.array_equal(qx, start) and np.abs(qx - start).max() > 1e-3
    u2 = (qx[1] ** 2 + qx[2] ** 2 + qx[3] ** 2) / qx[0]
    assert qx[0].min() > 0 and (0.4 * (qx[4] - 0.5 * u2)).min() > 0


def test_advection_3d_is_symmetric_under_permutations_of_the_axes():
    """the same with ADVECTION_3D_RP: the velocity along the field's axis is 0.75, the other two are -0.5 and 0.25"""
    n = 70
    x = (np.arange(n) + 0.5) / n
    prof = (np.where(x < 0.5, 1.0, 0.125) + 0.05 * np.sin(6.0 * np.pi * x))[None]
    vel = (0.75, -0.5, 0.25)
    results = []
    for axis in range(3):
        p = [0.0, 0.0, 0.0]
        for k in range(3):
            p[(axis + k) % 3] = vel[k]
        rp = pyclaw.CellRiemann3D(problems.ADVECTION_3D_RP, 1, 1, params=p)
        q, log = run_five_steps(rp, laid_along(axis, prof, ACROSS[axis]), 1)
        results.append((profile_of(q, axis), log))
    (qx, logx), (qy, logy), (qz, logz) = results
    assert len(logx) == 5 and logx == logy == logz
    assert np.array_equal(qx, qy) and np.array_equal(qx, qz)
    assert np.abs(qx - prof).max() > 1e-3 and qx.min() > 0


# ---- 8. Euler at first order against the numpy restatement ---------------------------------------------------------------------
def test_euler_3d_first_order_step_is_the_numpy_roe_update():
    """smooth positive data, one first-order step of the three sweeps.  Not bitwise -- the association of the sums and the
    device's division and square root may differ from numpy's -- so the project's relative gate: 1e-12 of the largest
    value of the reference.  (The restatement is checked on its own in tests/test_cellrp3_cpu.py.)"""
    shape = (61, 18, 5)
    full = tuple(n + 4 for n in shape)
    rng = np.random.default_rng(9)
    X, Y, Z = np.meshgrid(*[np.arange(n) / float(n) for n in full], indexing="ij")
    q0 = np.empty((5,) + full, order="F")
    q0[0] = 1.0 + 0.3 * np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y) + 0.1 * np.sin(2 * np.pi * Z)
    vel = [0.4 * np.sin(2 * np.pi * (X + Y)), -0.3 * np.cos(2 * np.pi * (Y - Z)), 0.2 * np.sin(2 * np.pi * (Z + X))]
    pres = 1.0 + 0.2 * np.cos(2 * np.pi * (X + Y + Z))
    for k in range(3):
        q0[1 + k] = q0[0] * vel[k]
    q0[4] = pres / 0.4 + 0.5 * q0[0] * sum(v * v for v in vel)
    q0 += 1e-3 * rng.standard_normal(q0.shape)

    def fluct(ql, qr, ixy):
        _, s, amdq, apdq = euler_roe(ql, qr, ixy, 1.4)
        return np.abs(s).max(axis=0), amdq, apdq
    dtd = 0.2
    ref, cfl_ref = godunov_step3(q0, dtd, fluct)
    d = 1.0 / 64
    hd = Handle3(problems.EULER_3D_RP, 5, 3, shape, (d, d, d), 1, [0, 0, 0], params=[1.4])
    try:
        out, cfl = hd.step(q0, dtd * d)
    finally:
        hd.close()
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    print("Euler 3-D, first order, device against numpy: max |diff| = %g, largest value %g, Courant numbers %.17g / %.17g"
          % (err, scale, cfl, cfl_ref))
    assert err <= GATE * scale
    assert abs(cfl - cfl_ref) <= GATE * cfl_ref and 0.1 < cfl < 1.0
    assert np.abs(out - q0).max() > 1e-3


# ---- 9. the other arithmetic modes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idir,shape", [(1, (245, 3, 2)), (2, (5, 66, 4)), (3, (6, 3, 130))])
def test_strict_equals_exact_and_fast_is_within_the_projects_gate(coracle, idir, shape):
    rng = np.random.default_rng(17 + idir)
    q, aux = vc_state(rng, shape)
    method = np.array([1, 2, -1, 0, 0, 0, 2], dtype=np.int32)
    lims, dt = [4, 4], 0.02
    want, cfl_o = oracle_sweep(coracle, q, aux, shape, dt, method, lims, idir)
    outs = []
    for math in (0, 1, 2):
        hd = Handle3(problems.VC_ACOUSTICS_3D_RP, 4, 2, shape, D3, 2, lims, maux=2, aux=(0, 1), math=math).put_aux(aux)
        try:
            outs.append(hd.sweep(q, idir, dt))
        finally:
            hd.close()
    (exact, cfl_e), (fast, cfl_f), (strict, cfl_s) = outs
    assert np.array_equal(exact, want) and cfl_e == cfl_o
    assert np.array_equal(strict, exact) and cfl_s == cfl_e
    print("fast against exact: max |diff| = %g, largest value %g" % (np.abs(fast - exact).max(), np.abs(exact).max()))
    assert np.abs(fast - exact).max() <= GATE * np.abs(exact).max()
    assert abs(cfl_f - cfl_e) <= GATE * cfl_e
