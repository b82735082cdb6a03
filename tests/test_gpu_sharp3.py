"""
GPU: SharpClaw in 3-D -- sharp3_kernel (csrc/sharpclaw.hpp) compiled at run time around a user-written Riemann solver
(pyclaw.SharpCellRiemann3D, pcl_cellrp_compile3_sharp) under pyclaw.SharpClawSolver3D.  The device is held to the numpy
restatement of flux1.f90 and of the slice driver in three dimensions (tests/sharp3_reference.py; tests/test_sharp3_cpu.py pins
that glue to the frozen oracle in 2-D) with the oracle's own reconstructions and its rpn3_vc_acoustics: bit for bit in
'exact' mode, the Courant number included.

Shapes: 58 cells are updated per 64-cell strip at order 5 (56 at order 7) and a tile is 16 lines wide, so (59, 17, 5),
(7, 60, 18) and (20, 6, 61) put every axis once one cell past a strip, once past a tile, and once tiny.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sharp3_reference as R
from apps import problems
from oracle import oracle as O
from pyclaw_amd import _lib as L
from pyclaw_amd import rk_tableaus

PCL_RP_CELL = 100
SHAPES = [(59, 17, 5), (7, 60, 18), (20, 6, 61)]
MTHLIM = [4, 2, 1, 3, 5, 1, 1, 1]           # tvd2: one limiter per COMPONENT, every entry of the configuration given
PER, EXT, WALL = R.PERIODIC, R.EXTRAP, R.WALL


# ---- one stage through the C interface --------------------------------------------------------------------------------------
def device_dq(pyclaw, body, meqn, mwaves, q, aux, aux_list, mcapa, d, dt, lim=2, order=5, math='exact', par=(), bc=None,
              mthlim=MTHLIM):
    """One pcl_sharp_dq (bc None: the ghost cells of q as given) or pcl_sharp_bc_dq (bc = 6 types: the device fills them) of a
    3-D solver created with pcl_create_cellrp -> (dq with ghost cells, Courant number)"""
    lib = L.lib()
    mbc = (order + 1) // 2
    rp = pyclaw.SharpCellRiemann3D(body, meqn, mwaves, aux=aux_list, capa=mcapa > 0)
    rp.compile(math, sharp=(lim, order))
    cfg = L.Config()
    cfg.ndim = 3
    for k in range(3):
        cfg.n[k], cfg.d[k] = q.shape[1 + k] - 2 * mbc, d[k]
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.rp = mbc, meqn, mwaves, PCL_RP_CELL
    cfg.maux = 0 if aux is None else aux.shape[0]
    cfg.method[1], cfg.method[5], cfg.method[6] = 2, mcapa, cfg.maux
    for k, m in enumerate(mthlim):
        cfg.mthlim[k] = m
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
        if bc is None:
            L.check(lib.pcl_sharp_dq(h, dt, C.cast(C.byref(cfl), L.dp)))
        else:
            types = np.array(bc, dtype=np.int32)
            L.check(lib.pcl_sharp_bc_dq(h, L.i(types), None, dt, C.cast(C.byref(cfl), L.dp)))
        L.check(lib.pcl_select(h, 3))
        out = np.zeros_like(q)
        L.check(lib.pcl_get_q(h, L.d(out), 1))
    finally:
        lib.pcl_destroy(h)
        rp.release()
    return out, cfl.value


def vc_arrays(rng, shape, mbc, capa):
    """random q = (p, u, v, w) (no zero waves anywhere) and aux = (Z, c[, capa]) varying per cell, ghost cells included"""
    full = tuple(n + 2 * mbc for n in shape)
    q = np.asfortranarray(rng.uniform(-1.0, 1.0, (4,) + full))
    aux = np.asfortranarray(rng.uniform(0.5, 2.0, (3 if capa else 2,) + full))
    return q, aux


def vc_reference(coracle, q, aux, mcapa, mbc, d, dt, lim, order):
    rpn = R.oracle_rpn3(coracle, O.RP_VC_ACOUSTICS_3D, 4, 2, aux.shape[0], mbc)
    return R.dq_reference(rpn, R.reconstruction(coracle, lim, order, mbc, MTHLIM), q, aux, mcapa, mbc, d, dt)


def inner(a, g):
    return a[(slice(None),) + (slice(g, -g),) * (a.ndim - 1)]


# shape 0: periodic on every side; shape 1: extrapolation and walls, mixed; shape 2: the ghost cells as they are uploaded
BCS = [[PER] * 6, [EXT, WALL, WALL, EXT, WALL, WALL], None]


@pytest.mark.parametrize("capa", [False, True], ids=["nocapa", "capa"])
@pytest.mark.parametrize("lim", [1, 2, 3])
@pytest.mark.parametrize("ishape", [0, 1, 2])
def test_dq_and_cfl_of_one_stage(coracle, ishape, lim, capa):
    import pyclaw_amd as pyclaw
    shape, bc, mbc = SHAPES[ishape], BCS[ishape], 3
    rng = np.random.default_rng(1000 * ishape + 10 * lim + capa)
    q, aux = vc_arrays(rng, shape, mbc, capa)
    d, dt = (0.11, 0.07, 0.05), 0.013
    mcapa = 3 if capa else 0
    out, cfl = device_dq(pyclaw, problems.VC_ACOUSTICS_3D_RP, 4, 2, q, aux, (0, 1), mcapa, d, dt, lim=lim, bc=bc)
    if bc is not None:      # the mbc = 3 ghost fill: what the device did to the uploaded ghost cells
        q = R.fill_ghosts(inner(q, mbc), mbc, bc[0::2], bc[1::2])
    ref, cfl_ref = vc_reference(coracle, q, aux, mcapa, mbc, d, dt, lim, 5)
    print("max |device - reference| = %g of %g, cfl %r / %r" % (np.abs(inner(out, mbc) - inner(ref, mbc)).max(),
                                                                np.abs(inner(ref, mbc)).max(), cfl, cfl_ref))
    assert np.abs(inner(ref, mbc)).max() > 1e-3
    assert cfl == cfl_ref
    assert np.array_equal(inner(out, mbc), inner(ref, mbc))


@pytest.mark.parametrize("capa", [False, True], ids=["nocapa", "capa"])
def test_weno_order_7(coracle, capa):
    """mbc = 4, 56 updated cells per strip: (53, 17, 5) is 56 + 1 - 4 cells along x, one strip plus one cell"""
    import pyclaw_amd as pyclaw
    shape, mbc = (53, 17, 5), 4
    rng = np.random.default_rng(7 + capa)
    q, aux = vc_arrays(rng, shape, mbc, capa)
    d, dt = (0.11, 0.07, 0.05), 0.013
    mcapa = 3 if capa else 0
    out, cfl = device_dq(pyclaw, problems.VC_ACOUSTICS_3D_RP, 4, 2, q, aux, (0, 1), mcapa, d, dt, lim=2, order=7, bc=[PER] * 6)
    q = R.fill_ghosts(inner(q, mbc), mbc, [PER] * 3, [PER] * 3)
    ref, cfl_ref = vc_reference(coracle, q, aux, mcapa, mbc, d, dt, 2, 7)
    assert cfl == cfl_ref
    assert np.array_equal(inner(out, mbc), inner(ref, mbc)), np.abs(inner(out, mbc) - inner(ref, mbc)).max()
    # the same state on a y-long and a z-long block: one strip plus one cell along those axes too
    for perm in ((1, 0, 2), (2, 1, 0)):
        qp = np.asfortranarray(np.transpose(q, (0,) + tuple(1 + p for p in perm)))
        ap = np.asfortranarray(np.transpose(aux, (0,) + tuple(1 + p for p in perm)))
        out, cfl = device_dq(pyclaw, problems.VC_ACOUSTICS_3D_RP, 4, 2, qp, ap, (0, 1), mcapa, d, dt, lim=2, order=7)
        ref, cfl_ref = vc_reference(coracle, qp, ap, mcapa, mbc, d, dt, 2, 7)
        assert cfl == cfl_ref and np.array_equal(inner(out, mbc), inner(ref, mbc))


# ---- 'strict' and 'fast' ----------------------------------------------------------------------------------------------------
def test_strict_equals_exact_and_fast_is_close(coracle):
    """fast mode at the tolerance tests/test_gpu_sharpclaw.py holds it to: 1e-12 of the largest value"""
    import pyclaw_amd as pyclaw
    shape, mbc = SHAPES[0], 3
    rng = np.random.default_rng(31)
    q, aux = vc_arrays(rng, shape, mbc, True)
    d, dt = (0.11, 0.07, 0.05), 0.013
    res = {m: device_dq(pyclaw, problems.VC_ACOUSTICS_3D_RP, 4, 2, q, aux, (0, 1), 3, d, dt, lim=2, math=m)
           for m in ('exact', 'strict', 'fast')}
    ref, cfl_ref = vc_reference(coracle, q, aux, 3, mbc, d, dt, 2, 5)
    assert res['exact'][1] == cfl_ref and np.array_equal(inner(res['exact'][0], mbc), inner(ref, mbc))
    assert res['strict'][1] == res['exact'][1] and np.array_equal(res['strict'][0], res['exact'][0])
    err = np.abs(inner(res['fast'][0], mbc) - inner(ref, mbc)).max()
    print("fast: max |device - reference| = %g of %g" % (err, np.abs(ref).max()))
    assert err < 1e-12 * np.abs(inner(ref, mbc)).max()
    assert abs(res['fast'][1] - cfl_ref) < 1e-12 * cfl_ref


# ---- axis checks without any oracle ------------------------------------------------------------------------------------------
def test_a_state_varying_along_one_axis_gives_the_same_line_along_x_y_and_z():
    """q and aux are functions of one coordinate; along x, y and z in turn, with the velocity components permuted with the
    axes, the line of dq is the same bit for bit: DIR 2 and DIR 3 (tile transposed and swizzled, aux staged in LDS) against
    DIR 1.  tvd2, because the statement is exact only there: on a constant line tvd2 returns ql = qr = q, so the two
    transverse passes add signed zeros, whereas the WENO forms, whose float32-rounded coefficients do not sum to 1, leave
    ql != qr on constant data and with them transverse increments of rounding size that are summed in another order (x,
    y, z) on each orientation."""
    import pyclaw_amd as pyclaw
    n, mbc, across = 61, 3, (5, 6)
    rng = np.random.default_rng(5)
    N = n + 2 * mbc
    prof_q, prof_a = rng.uniform(-1.0, 1.0, (4, N)), rng.uniform(0.5, 2.0, (3, N))
    lines = []
    for axis in range(3):
        shape = [0, 0, 0]
        shape[axis], shape[(axis + 1) % 3], shape[(axis + 2) % 3] = N, across[0] + 2 * mbc, across[1] + 2 * mbc
        idx = [None, None, None]
        idx[axis] = slice(None)
        q = np.zeros([4] + shape, order="F")
        aux = np.zeros([3] + shape, order="F")
        q[0] = prof_q[0][tuple(idx)]
        for k in range(3):          # (u, v, w) of the profile are the velocities along axis, axis + 1, axis + 2
            q[1 + (axis + k) % 3] = prof_q[1 + k][tuple(idx)]
        for k in range(3):
            aux[k] = prof_a[k][tuple(idx)]
        # (one limiter for the three velocity components: they change places with the orientation)
        out, cfl = device_dq(pyclaw, problems.VC_ACOUSTICS_3D_RP, 4, 2, q, aux, (0, 1), 3, (0.1, 0.1, 0.1), 0.02, lim=1,
                             mthlim=[4, 2, 2, 2, 1, 1, 1, 1])
        out = np.moveaxis(out, 1 + axis, 1)
        # every line of the block is the same line
        assert all(np.array_equal(out[:, :, mbc, mbc], out[:, :, j, k]) for j in range(mbc, out.shape[2] - mbc)
                   for k in range(mbc, out.shape[3] - mbc))
        line = out[:, mbc:-mbc, mbc, mbc]
        lines.append((np.stack([line[0]] + [line[1 + (axis + k) % 3] for k in range(3)]), cfl))
    assert np.abs(lines[0][0][:2]).min() > 0 and not lines[0][0][2:].any()
    for line, cfl in lines[1:]:
        assert cfl == lines[0][1]
        assert np.array_equal(line, lines[0][0])


@pytest.mark.parametrize("lim", [2, 3])
def test_swapping_x_and_y_of_a_state_transposes_the_result(lim):
    import pyclaw_amd as pyclaw
    shape, mbc = (20, 61, 6), 3
    rng = np.random.default_rng(77 + lim)
    q, aux = vc_arrays(rng, shape, mbc, True)
    d, dt = (0.11, 0.07, 0.05), 0.013
    out, cfl = device_dq(pyclaw, problems.VC_ACOUSTICS_3D_RP, 4, 2, q, aux, (0, 1), 3, d, dt, lim=lim)
    qs = np.asfortranarray(np.transpose(q, (0, 2, 1, 3))[[0, 2, 1, 3]])
    auxs = np.asfortranarray(np.transpose(aux, (0, 2, 1, 3)))
    outs, cfls = device_dq(pyclaw, problems.VC_ACOUSTICS_3D_RP, 4, 2, qs, auxs, (0, 1), 3, (d[1], d[0], d[2]), dt, lim=lim)
    assert cfl == cfls and np.abs(inner(out, mbc)).max() > 1e-3
    assert np.array_equal(np.transpose(outs, (0, 2, 1, 3))[[0, 2, 1, 3]], out)


# ---- whole steps under the Python solver --------------------------------------------------------------------------------------
STEP_SHAPE = (20, 19, 18)
STEP_BCS = ([PER, EXT, WALL], [PER, EXT, WALL])


def vc_claw(pyclaw, ti, shape=STEP_SHAPE, capa=False, seed=3, math='exact'):
    claw = problems.acoustics3D(pyclaw, mx=shape[0], my=shape[1], mz=shape[2], run=False, solver_type='sharpclaw',
                                time_integrator=ti, math=math)
    solver, state = claw.solver, claw.solution.state
    rng = np.random.default_rng(seed)
    if capa:
        grid = state.grid
        state2 = pyclaw.State(grid, 4, 3)
        state2.mcapa = 2
        claw.solution = pyclaw.Solution(state2)
        state = state2
        solver.rp = pyclaw.SharpCellRiemann3D(problems.VC_ACOUSTICS_3D_RP, 4, 2, aux=(0, 1), capa=True)
    # smooth enough for a stable run, every cell different, aux varying per cell
    X, Y, Z = state.grid._c_center
    state.q[0] = np.exp(-8.0 * (X ** 2 + Y ** 2 + Z ** 2)) + 0.01 * rng.uniform(-1.0, 1.0, shape)
    state.q[1:] = 0.01 * rng.uniform(-1.0, 1.0, (3,) + shape)
    state.aux[...] = rng.uniform(0.8, 1.25, state.aux.shape)
    for k in range(3):
        solver.bc_lower[k], solver.bc_upper[k] = STEP_BCS[0][k], STEP_BCS[1][k]
        solver.aux_bc_lower[k], solver.aux_bc_upper[k] = STEP_BCS[0][k], STEP_BCS[1][k]
    return claw


def device_steps(claw, nsteps, dt0, cfl_max, cfl_desired, resident=False):
    """nsteps accepted steps with the solver's own step-size control -> q, t, [(dt, cfl) of every stage, rejected ones too]"""
    solver, solution = claw.solver, claw.solution
    solver.cfl_max, solver.cfl_desired = cfl_max, cfl_desired
    solver.dt_variable = True
    solver.dt_initial = dt0
    solver.setup(solution)
    seen = []
    solver.cfl._reduce = lambda v: (seen.append((solver.dt, v)), v)[1]
    solver.dt = dt0
    try:
        for n in range(nsteps):
            solver.evolve_to_time(solution)
    finally:
        solver.teardown()
    return solution.state.q.copy('F'), solution.t, seen


def reference_steps(coracle, claw, ti, nsteps, dt0, cfl_max, cfl_desired, mcapa=0):
    state = claw.solution.state
    mbc = 3
    q = state.q.copy('F')
    auxb = R.fill_ghosts(state.aux, mbc, STEP_BCS[0], STEP_BCS[1], is_aux=True)
    d = tuple(float(x) for x in state.grid.d)
    rpn = R.oracle_rpn3(coracle, O.RP_VC_ACOUSTICS_3D, 4, 2, auxb.shape[0], mbc)
    recon = R.reconstruction(coracle, 2, 5, mbc)
    t, dt, seen, nrej, done = 0.0, dt0, [], 0, 0
    while done < nsteps:
        def dq(y):
            qb = R.fill_ghosts(y, mbc, STEP_BCS[0], STEP_BCS[1])
            D, c = R.dq_reference(rpn, recon, qb, auxb, mcapa, mbc, d, dt)
            return inner(D, mbc), c
        with np.errstate(all="ignore"):
            if ti == 'SSP104':
                qn, cfls = R.ssp104(q, dq)
            elif ti == 'SSP33':
                qn, cfls = R.ssp33(q, dq)
            else:
                tab = rk_tableaus.TABLEAUS[ti]
                a, b, c = rk_tableaus.validate(tab['a'], tab['b'], tab['c'])
                qn, cfls = R.tableau(q, dq, a, b, c)
        over = [k for k, c in enumerate(cfls) if c > cfl_max]
        if over:                    # the step ends at the first stage over cfl_max, q is as it was
            cfls = cfls[:over[0] + 1]
            nrej += 1
        else:
            q, t, done = qn, t + dt, done + 1
        seen += [(dt, c) for c in cfls]
        if cfls[-1] > 0.0:
            dt = min(1e99, dt * cfl_desired / cfls[-1])
    return q, t, seen, nrej


@pytest.mark.parametrize("ti,cfl_max,cfl_desired", [('SSP104', 2.5, 2.45), ('SSP33', 0.5, 0.45), ('RK44', 0.5, 0.45)])
def test_three_steps_equal_the_restated_scheme(coracle, ti, cfl_max, cfl_desired):
    """(20, 19, 18), periodic in x, extrapolation in y, walls in z; the first step is far too long and is rejected, which must
    leave q as it was: q, every dt and every stage's Courant number are those of the numpy restatement"""
    import pyclaw_amd as pyclaw
    dt0 = 0.5
    claw = vc_claw(pyclaw, ti)
    want, t_want, seen_want, nrej = reference_steps(coracle, claw, ti, 3, dt0, cfl_max, cfl_desired)
    q0 = claw.solution.state.q.copy('F')
    got, t, seen = device_steps(claw, 3, dt0, cfl_max, cfl_desired)
    print("%s: %d stages, %d rejected steps, max |device - reference| = %g" % (ti, len(seen), nrej, np.abs(got - want).max()))
    assert nrej >= 1 and np.abs(want - q0).max() > 1e-3
    assert seen == seen_want
    assert t == t_want
    assert np.array_equal(got, want)


def test_resident_mode_equals_the_plain_run():
    import pyclaw_amd as pyclaw
    runs = []
    for resident in (False, True):
        claw = vc_claw(pyclaw, 'SSP104', shape=(20, 6, 17), capa=True)
        solver, solution = claw.solver, claw.solution
        solver.dt_initial = 0.01
        solver.setup(solution)
        try:
            if resident:
                solver.begin_resident(solution)
            solver.evolve_to_time(solution, 0.03)
            solver.evolve_to_time(solution, 0.06)
            if resident:
                solver.end_resident(solution)
        finally:
            solver.teardown()
        runs.append((solution.state.q.copy('F'), solution.t, solver.status['numsteps']))
    assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2] and runs[0][2] >= 1
    assert np.array_equal(runs[0][0], runs[1][0])


def test_a_pointwise_cell_dq_source_equals_its_numpy_callback():
    """dq_src as a CellDqSource runs as a pass of its own behind the three directional passes; the same source as a Python
    callback goes through the host"""
    import pyclaw_amd as pyclaw

    def callback(solver, state, dt):
        dq = np.zeros(state.q.shape, order='F')
        dq[0] = dt * (-0.5) * state.q[0]
        dq[3] = dt * 0.25 * state.q[0]
        return dq
    runs = []
    for src in (pyclaw.CellDqSource("dq[0] = c.dt * p[0] * q[0];\ndq[3] = c.dt * p[1] * q[0];\n", params=[-0.5, 0.25]), callback):
        claw = vc_claw(pyclaw, 'SSP33', shape=(20, 6, 17))
        claw.solver.dq_src = src
        claw.solver.cfl_max, claw.solver.cfl_desired = 0.5, 0.45
        claw.solver.dt_initial = 0.005
        claw.solver.setup(claw.solution)
        try:
            claw.solver.evolve_to_time(claw.solution, 0.02)
        finally:
            claw.solver.teardown()
        runs.append(claw.solution.state.q.copy('F'))
    plain = vc_claw(pyclaw, 'SSP33', shape=(20, 6, 17))
    plain.solver.cfl_max, plain.solver.cfl_desired = 0.5, 0.45
    plain.solver.dt_initial = 0.005
    plain.solver.setup(plain.solution)
    try:
        plain.solver.evolve_to_time(plain.solution, 0.02)
    finally:
        plain.solver.teardown()
    assert np.abs(runs[0] - plain.solution.state.q).max() > 1e-4        # the source did something
    assert np.array_equal(runs[0], runs[1])


# ---- a solver with no oracle: dimension consistency ---------------------------------------------------------------------------
def test_euler_uniform_in_z_equals_the_2d_run_plane_by_plane():
    """EULER_3D_RP on (64, 6, 4), Sod's jump along x and along y, uniform in z, two SSP104 steps: every z plane equals the
    run of the same body as a 2-D CellRiemann(sharpclaw=True), np.array_equal (signed zeros compare equal).
    tvd2 (lim_type 1): there a constant line reconstructs to ql = qr = q exactly, so the z pass adds signed zeros and the
    statement is exact.  It is not for the WENO forms: their float32-rounded coefficients do not sum to 1, ql != qr on a
    constant line, and the z pass leaves increments of rounding size in the z momentum -- the numpy restatement of the scheme
    itself (tests/sharp3_reference.py with the Roe formulas of tests/test_cellrp3_cpu.py, lim_type 2, a 24 x 6 x 4 block)
    differs from its own 2-D run by 1.2e-33 in that component and in no other."""
    import pyclaw_amd as pyclaw
    gamma = 1.4
    results = {}
    for ndim in (2, 3):
        shape = (64, 6, 4)[:ndim]
        dims = [pyclaw.Dimension(n, 0.0, shape[k] / 64.0, shape[k]) for k, n in enumerate("xyz"[:ndim])]
        state = pyclaw.State(pyclaw.Grid(dims), 5)
        state.grid.compute_c_center()
        X, Y = state.grid._c_center[0], state.grid._c_center[1]
        left = (X < 0.5) & (Y < 3.0 / 64.0)
        state.q[0] = np.where(left, 1.0, 0.125)
        state.q[1:4] = 0.0
        state.q[4] = np.where(left, 1.0, 0.1) / (gamma - 1.0)
        if ndim == 3:
            solver = pyclaw.SharpClawSolver3D()
            solver.rp = pyclaw.SharpCellRiemann3D(problems.EULER_3D_RP, 5, 3, params=[gamma])
        else:
            solver = pyclaw.SharpClawSolver2D()
            solver.rp = pyclaw.CellRiemann(problems.EULER_3D_RP, 5, 3, 2, params=[gamma], sharpclaw=True)
        solver.mwaves, solver.lim_type, solver.limiters = 3, 1, [4, 4, 4]
        for k in range(ndim):
            solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.outflow
        solver.dt_variable = False
        solution = pyclaw.Solution(state)
        solver.setup(solution)
        solver.dt = 0.4 / 64.0
        try:
            solver.evolve_to_time(solution)
            solver.evolve_to_time(solution)
        finally:
            solver.teardown()
        results[ndim] = solution.state.q.copy('F')
    q2, q3 = results[2], results[3]
    assert np.abs(q2[1]).max() > 1e-3 and np.abs(q2[2]).max() > 1e-3 and np.isfinite(q3).all()
    for k in range(4):
        assert np.array_equal(q3[:, :, :, k], q2), (k, np.abs(q3[:, :, :, k] - q2).max())
