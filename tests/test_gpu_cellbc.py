"""
GPU: custom boundary conditions as cell functions (pyclaw.CellBC) -- user-written C++ per ghost cell, compiled at setup()
and run on the resident arrays -- against the Python callbacks they stand in for and against the library's built-in
fills, never against themselves.  Every comparison is bit for bit in 'exact' mode; 'fast' is held to the gate
tests/test_gpu_cellfn.py uses for its 'fast' run.

Bodies used for bit comparisons contain + - * / and comparisons only.  The number of distinct bodies is kept small:
each is one run-time compile per (meqn, maux, ndim, math).
"""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from apps import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12                      # tests/test_gpu_cellfn.py::test_shockbubble_cell_source_fast (the project's 'fast' gate)

EXTRAP = "for (int m = 0; m < MEQN; m++) q[m] = (1.0 + 0.5 * c.g) * (2.0 * qin(m, 0) - qin(m, 1));"
OUTFLOW = "for (int m = 0; m < MEQN; m++) q[m] = qin(m, 0);"
MIRROR = "for (int m = 0; m < MEQN; m++) q[m] = qin(m, c.g);\nq[c.idim + 1] = -q[c.idim + 1];"
# x: the constant state p[0 .. MEQN-1]; any other dimension: the solid wall
CONST_OR_MIRROR = ("if (c.idim == 0) { for (int m = 0; m < MEQN; m++) q[m] = p[m]; }\n"
                   "else { for (int m = 0; m < MEQN; m++) q[m] = qin(m, c.g); q[c.idim + 1] = -q[c.idim + 1]; }")
INFLOW = "q[0] = p[0] + p[1] * c.t * (1.0 - c.t);\nfor (int m = 1; m < MEQN; m++) q[m] = 0.0;"
# component m := entry (p[0] + m) of (c.i[], c.x[], c.g, c.side)
STAMP = ("double v[2 * NDIM + 2];\n"
         "for (int k = 0; k < NDIM; k++) { v[k] = c.i[k]; v[NDIM + k] = c.x[k]; }\n"
         "v[2 * NDIM] = c.g; v[2 * NDIM + 1] = c.side;\n"
         "for (int m = 0; m < MEQN; m++) q[m] = v[((int)p[0] + m) % (2 * NDIM + 2)];")
CLAMP = "q[0] = qin(0, (int)p[0]);"


def lib():
    from pyclaw_amd import _lib
    return _lib, _lib.lib()


def compiles():
    _lib, L = lib()
    n, h = ctypes.c_long(), ctypes.c_long()
    _lib.check(L.pcl_cellfn_stats(ctypes.byref(n), ctypes.byref(h)))
    return n.value


def inflow_state():
    rinf, vinf, einf = problems.shock_state()
    return [rinf, rinf * vinf, 0., einf, 0.]


def put_ghosted(solver, up):
    _lib, L = lib()
    _lib.check(L.pcl_put_q(solver._h, _lib.d(up), 1))


def get_ghosted(solver):
    _lib, L = lib()
    back = np.empty(solver.qbc.shape, order='F')
    _lib.check(L.pcl_get_q(solver._h, _lib.d(back), 1))
    return back


def all_custom(solver, lower, upper):
    for k in range(solver.ndim):
        solver.bc_lower[k] = solver.bc_upper[k] = 0        # BC.custom
    solver.user_bc_lower, solver.user_bc_upper = lower, upper


def filled_frame(claw, lower, upper, seed=7):
    """all sides custom; upload a random ghosted array, apply_q_bcs, read the ghosted array back: (uploaded, read back)"""
    solver, state = claw.solver, claw.solution.state
    all_custom(solver, lower, upper)
    solver.setup(claw.solution)
    solver._push(state)
    up = np.asfortranarray(np.random.default_rng(seed).standard_normal(solver.qbc.shape))
    put_ghosted(solver, up)
    solver.apply_q_bcs(state)
    back = get_ghosted(solver)
    solver.teardown()
    return up, back


def interior(a, mbc):
    return a[(slice(None),) + (slice(mbc, -mbc),) * (a.ndim - 1)]


# ---- 1: the ghost frame after one fill ------------------------------------------------------------------------------------
def extrap_lower(state, dim, t, qbc, mbc):
    a = np.moveaxis(qbc, state.grid.dimensions.index(dim) + 1, 1)
    for g in range(mbc):
        a[:, mbc - 1 - g] = (1.0 + 0.5 * g) * (2.0 * a[:, mbc] - a[:, mbc + 1])


def extrap_upper(state, dim, t, qbc, mbc):
    a = np.moveaxis(qbc, state.grid.dimensions.index(dim) + 1, 1)
    for g in range(mbc):
        a[:, -mbc + g] = (1.0 + 0.5 * g) * (2.0 * a[:, -mbc - 1] - a[:, -mbc - 2])


@pytest.mark.parametrize("mbc", [2, 3])
def test_ghost_frame_after_one_fill(mbc):
    """37 x 21 Euler, every side custom with one linear-extrapolation body: the whole ghost frame, corners included,
    equals what the numpy callbacks leave (the y fill reads x-filled ghosts, over the full ghosted width); the interior
    is untouched.  mbc 3 is the SharpClaw solver's."""
    import pyclaw_amd as pyclaw
    kind = {'solver_type': 'sharpclaw', 'time_integrator': 'SSP33'} if mbc == 3 else {}

    def claw():
        return problems.shockbubble(pyclaw, mx=37, my=21, device_callbacks=True, run=False, **kind)

    up, want = filled_frame(claw(), extrap_lower, extrap_upper)
    bc = pyclaw.CellBC(EXTRAP)
    up2, got = filled_frame(claw(), bc, bc)
    assert got.shape == (5, 37 + 2 * mbc, 21 + 2 * mbc) and np.array_equal(up, up2)
    print("frame, mbc %d: max |cell - numpy| = %g" % (mbc, np.abs(got - want).max()))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(interior(got, mbc).view(np.uint64), interior(up, mbc).view(np.uint64))
    ghosts = np.ones(up.shape, dtype=bool)
    interior(ghosts, mbc)[...] = False
    assert not np.any(got[ghosts] == up[ghosts])               # every ghost cell was written


# ---- 2: equals the built-in fills -----------------------------------------------------------------------------------------
def ten_steps(claw):
    solver, solution = claw.solver, claw.solution
    solver.setup(solution)
    solver.dt = solver.dt_initial
    for _ in range(10):
        solver.evolve_to_time(solution)
    spec = solver._device_bc_spec(solution.state)
    solver.teardown()
    return solution.state.q.copy('F'), spec


@pytest.fixture(scope="module")
def sb_builtin():
    """10 steps of the 160 x 40 shock-bubble with the built-in fills (pcl_bc_step: ghosts filled inside the x pass)"""
    import pyclaw_amd as pyclaw
    q, spec = ten_steps(problems.shockbubble(pyclaw, device_callbacks=True, run=False))
    assert spec is not None
    return q


@pytest.mark.parametrize("case", ["outflow", "reflecting", "constant"])
def test_equals_builtin_fills_shockbubble(sb_builtin, case):
    import pyclaw_amd as pyclaw
    claw = problems.shockbubble(pyclaw, device_callbacks=True, run=False)
    solver = claw.solver
    if case == "outflow":               # both upper sides of the set-up are BC.outflow
        solver.bc_upper[0] = solver.bc_upper[1] = pyclaw.BC.custom
        solver.user_bc_upper = pyclaw.CellBC(OUTFLOW)
    elif case == "reflecting":          # the lower y side is BC.reflecting; the same object restates the inflow in x
        solver.bc_lower[1] = pyclaw.BC.custom
        solver.user_bc_lower = pyclaw.CellBC(CONST_OR_MIRROR, params=inflow_state())
    else:
        solver.user_bc_lower = pyclaw.CellBC(CONST_OR_MIRROR, params=inflow_state(), dims=[0])
    q, spec = ten_steps(claw)
    assert spec is None                 # apply_q_bcs + pcl_step_hyperbolic, not pcl_bc_step
    print("shock-bubble, %s: max |cell - built-in| = %g" % (case, np.abs(q - sb_builtin).max()))
    assert np.array_equal(q, sb_builtin)


def test_equals_builtin_fills_unsplit_step():
    """the unsplit classic step (transverse solves read the corner ghost cells), every side of the set-up restated"""
    import pyclaw_amd as pyclaw

    def claw():
        return problems.shockbubble(pyclaw, mx=67, my=23, dim_split=False, device_callbacks=True, run=False)

    want, spec = ten_steps(claw())
    cell = claw()
    solver = cell.solver
    all_custom(solver, pyclaw.CellBC(CONST_OR_MIRROR, params=inflow_state()), pyclaw.CellBC(OUTFLOW))
    got, spec_cell = ten_steps(cell)
    assert spec is not None and spec_cell is None
    print("unsplit shock-bubble: max |cell - built-in| = %g" % np.abs(got - want).max())
    assert np.array_equal(got, want)


def test_equals_builtin_reflecting_acoustics_box():
    import pyclaw_amd as pyclaw

    def run(bc):
        claw = problems.acoustics2D(pyclaw, mx=37, my=21, run=False)
        solver = claw.solver
        for k in range(2):
            solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.custom if bc else pyclaw.BC.reflecting
        solver.user_bc_lower = solver.user_bc_upper = bc
        return ten_steps(claw)

    want, spec = run(None)
    got, spec_cell = run(pyclaw.CellBC(MIRROR))
    assert spec is not None and spec_cell is None
    print("acoustics box: max |cell - built-in| = %g" % np.abs(got - want).max())
    assert np.array_equal(got, want)


# ---- 3: time-dependent inflow, classic and SharpClaw ------------------------------------------------------------------------
def advection_1d(pyclaw, mx=50):
    solver = pyclaw.ClawSolver1D()
    solver.rp = pyclaw.riemann.rp_advection_1d
    solver.mwaves = 1
    solver.bc_lower[0] = pyclaw.BC.custom
    solver.bc_upper[0] = pyclaw.BC.outflow
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.5, 1.75, mx)), 1)
    state.aux_global['u'] = 1.
    xc = state.grid.x.center
    state.q[0, :] = np.exp(-100 * (xc - 1.0) ** 2) + 0.25
    solver.dt_initial = 0.8 * state.grid.d[0]
    claw = pyclaw.Controller()
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    return claw


def acoustics_sharp(pyclaw):
    claw = problems.acoustics2D(pyclaw, mx=24, my=18, solver_type='sharpclaw', time_integrator='SSP33', run=False)
    claw.solver.bc_lower[0] = pyclaw.BC.custom
    return claw


def acoustics_1d_sharp(pyclaw, mx=50):
    solver = pyclaw.SharpClawSolver1D()
    solver.lim_type, solver.time_integrator, solver.weno_order = 2, 'SSP33', 5
    solver.rp = pyclaw.riemann.rp_acoustics_1d
    solver.mwaves = 2
    solver.bc_lower[0] = pyclaw.BC.custom
    solver.bc_upper[0] = pyclaw.BC.outflow
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx)), 2)
    state.aux_global.update({'rho': 1.0, 'bulk': 1.0, 'zz': 1.0, 'cc': 1.0})
    xc = state.grid.x.center
    state.q[0, :] = np.exp(-100 * (xc - 0.75) ** 2)
    state.q[1, :] = 0.
    solver.dt_initial = 0.1 * state.grid.d[0]
    claw = pyclaw.Controller()
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    return claw


@pytest.mark.parametrize("which", ["classic_1d", "sharpclaw_1d", "sharpclaw_2d"])
def test_time_dependent_inflow(which):
    """Lower-x value p[0] + p[1] t (1 - t), t = state.t (the stage time in SharpClaw), against the Python callback; the
    parameters are reassigned after 5 of the 10 steps, and nothing is compiled again.  Classic 1-D advection on 50 cells,
    SharpClaw SSP33 1-D acoustics on 50 cells and 2-D acoustics on 24 x 18 (mbc 3)."""
    import pyclaw_amd as pyclaw
    make = {"classic_1d": advection_1d, "sharpclaw_1d": acoustics_1d_sharp, "sharpclaw_2d": acoustics_sharp}[which]
    coef = {}
    seen = []

    def python_bc(state, dim, t, qbc, mbc):
        assert t == state.t
        seen.append(t)
        a, b = coef['p']
        qbc[0, :mbc, ...] = a + b * state.t * (1.0 - state.t)
        qbc[1:, :mbc, ...] = 0.0

    def run(bc, set_p):
        claw = make(pyclaw)
        solver, solution = claw.solver, claw.solution
        assert solver.mbc == (2 if which == "classic_1d" else 3)
        solver.user_bc_lower = bc
        set_p((0.5, 2.0))
        solver.setup(solution)
        solver.dt = solver.dt_initial
        n0 = compiles()
        for n in range(10):
            if n == 5:
                set_p((0.75, -3.0))
            solver.evolve_to_time(solution)
        assert compiles() == n0
        assert solution.t > 0.0
        solver.teardown()
        return solution.state.q.copy('F'), solution.t

    want, t_want = run(python_bc, lambda p: coef.__setitem__('p', p))
    cell = pyclaw.CellBC(INFLOW)
    got, t_got = run(cell, lambda p: setattr(cell, 'params', p))
    assert t_got == t_want
    if which != "classic_1d":
        assert len(set(seen)) > 10                 # the callback saw stage times, not only step times
    print("inflow %s: max |cell - python| = %g at t = %g" % (which, np.abs(got - want).max(), t_got))
    assert np.array_equal(got, want)
    frozen, _ = run(python_bc, lambda p: coef.__setitem__('p', (0.5, 2.0)))
    assert not np.array_equal(frozen, want)        # the reassigned parameters are what the result shows


# ---- 4: index and coordinate stamps ---------------------------------------------------------------------------------------
def stamp_claw(pyclaw, ndim):
    if ndim == 1:
        return advection_1d(pyclaw, mx=50)
    if ndim == 2:
        return problems.acoustics2D(pyclaw, mx=37, my=21, run=False)
    return problems.acoustics3D(pyclaw, test='hom', mx=9, my=7, mz=6, run=False)


def stamp_values(state, mbc):
    """entries (c.i[], c.x[]) over the ghosted index range, as arrays that broadcast over the ghosted block"""
    dims = state.grid.dimensions
    nd = len(dims)
    out = []
    for k, dim in enumerate(dims):
        gi = np.arange(-mbc, dim.n + mbc)
        shape = [1] * nd
        shape[k] = len(gi)
        out.append((gi.astype(np.float64).reshape(shape), (dim.lower + (gi + 0.5) * dim.d).reshape(shape)))
    return [o[0] for o in out] + [o[1] for o in out]


def stamp_side(want, state, mbc, idim, side, first):
    """what one launch of STAMP with p[0] = first leaves in `want` (ghosted, meqn first)"""
    nd = want.ndim - 1
    meqn = want.shape[0]
    ent = stamp_values(state, mbc)
    sl = [slice(None)] * nd
    sl[idim] = slice(0, mbc) if side == 0 else slice(-mbc, None)
    box = want[(slice(None),) + tuple(sl)]
    layer_shape = [1] * nd
    layer_shape[idim] = mbc
    layer = (np.arange(mbc - 1, -1, -1.0) if side == 0 else np.arange(0.0, mbc)).reshape(layer_shape)
    for m in range(meqn):
        e = (first + m) % (2 * nd + 2)
        if e < 2 * nd:
            v = ent[e][tuple(sl[k] if k == (e % nd) else slice(None) for k in range(nd))]
        elif e == 2 * nd:
            v = layer
        else:
            v = float(side)
        box[m] = np.broadcast_to(v, box[m].shape)


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_index_and_coordinate_stamps(ndim):
    """c.i (negative and >= n), c.x, c.g and c.side of every ghost cell of every side, in the order apply_q_bcs fills
    them (a later dimension's launch overwrites the corners), against numpy's cell centres extended into the ghosts."""
    import pyclaw_amd as pyclaw
    claw = stamp_claw(pyclaw, ndim)
    solver, state = claw.solver, claw.solution.state
    bc = pyclaw.CellBC(STAMP, params=[0])
    all_custom(solver, bc, bc)
    solver.setup(claw.solution)
    solver._push(state)
    mbc, meqn = solver.mbc, state.meqn
    up = np.asfortranarray(np.random.default_rng(11).standard_normal(solver.qbc.shape))
    n0 = compiles()
    for first in range(0, 2 * ndim + 2, meqn):
        put_ghosted(solver, up)
        bc.params = [first]
        solver.apply_q_bcs(state)
        got = get_ghosted(solver)
        want = up.copy('F')
        for idim in range(ndim):
            for side in (0, 1):
                stamp_side(want, state, mbc, idim, side, first)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (ndim, first)
    assert compiles() == n0
    solver.teardown()


def test_periodic_side_beside_a_custom_one_is_not_written():
    """x custom, y periodic: the two x launches write the x ghost columns over the whole ghosted height and nothing else."""
    import pyclaw_amd as pyclaw
    claw = stamp_claw(pyclaw, 2)
    solver, state = claw.solver, claw.solution.state
    bc = pyclaw.CellBC(STAMP, params=[0])
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.custom
    solver.bc_lower[1] = solver.bc_upper[1] = pyclaw.BC.periodic
    solver.user_bc_lower = solver.user_bc_upper = bc
    solver.setup(claw.solution)
    solver._push(state)
    mbc = solver.mbc
    up = np.asfortranarray(np.random.default_rng(12).standard_normal(solver.qbc.shape))
    put_ghosted(solver, up)
    dim = state.grid.dimensions[0]
    solver._custom_bc(state, dim, 0, 0, bc)
    solver._custom_bc(state, dim, 0, 1, bc)
    got = get_ghosted(solver)
    want = up.copy('F')
    stamp_side(want, state, mbc, 0, 0, 0)
    stamp_side(want, state, mbc, 0, 1, 0)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.array_equal(got[:, mbc:-mbc, :mbc].view(np.uint64), up[:, mbc:-mbc, :mbc].view(np.uint64))
    assert np.array_equal(got[:, mbc:-mbc, -mbc:].view(np.uint64), up[:, mbc:-mbc, -mbc:].view(np.uint64))
    # a CellBC restricted to y leaves the x sides alone altogether
    put_ghosted(solver, up)
    only_y = pyclaw.CellBC(STAMP, params=[0], dims=[1])
    solver._custom_bc(state, dim, 0, 0, only_y)
    assert np.array_equal(get_ghosted(solver).view(np.uint64), up.view(np.uint64))
    solver.teardown()


# ---- 5: clamping ------------------------------------------------------------------------------------------------------------
def test_inward_reads_are_clamped():
    """qin(0, 1000000) and qin(0, -5): the last and the first interior cell of the line, counted from the side"""
    import pyclaw_amd as pyclaw
    claw = advection_1d(pyclaw, mx=50)
    solver, state = claw.solver, claw.solution.state
    bc = pyclaw.CellBC(CLAMP, params=[0])
    all_custom(solver, bc, bc)
    solver.setup(claw.solution)
    solver._push(state)
    mbc = solver.mbc
    up = np.asfortranarray(np.random.default_rng(13).standard_normal(solver.qbc.shape))
    first, last = up[0, mbc], up[0, -mbc - 1]
    for r, lower, upper in ((1000000, last, first), (-5, first, last), (0, first, last), (49, last, first),
                            (50, last, first), (1, up[0, mbc + 1], up[0, -mbc - 2])):
        put_ghosted(solver, up)
        bc.params = [r]
        solver.apply_q_bcs(state)
        got = get_ghosted(solver)
        assert np.all(got[0, :mbc] == lower) and np.all(got[0, -mbc:] == upper), r
        assert np.array_equal(got[0, mbc:-mbc], up[0, mbc:-mbc])
    solver.teardown()


# ---- 6: bookkeeping in resident mode, 8: fast math ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sb_gold(golden_dir):
    return np.loadtxt(os.path.join(golden_dir, "sb_density"))


def sb_inflow_run(pyclaw, math='exact'):
    """the shock-bubble regression in resident mode, its inflow state restated as a CellBC: (density, steps, enqueued ahead)"""
    _lib, L = lib()
    claw = problems.shockbubble(pyclaw, device_callbacks=True, math=math, run=False)
    solver, solution = claw.solver, claw.solution
    solver.user_bc_lower = pyclaw.CellBC(CONST_OR_MIRROR, params=inflow_state())
    solver.setup(solution)
    solver.dt = solver.dt_initial
    solver.begin_resident(solution)
    solver.evolve_to_time(solution, claw.tfinal)
    a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(L.pcl_step_ahead_stats(solver._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    solver.end_resident(solution)
    steps = solver.status['numsteps']
    solver.teardown()
    return solution.state.q[0].copy(), steps, a.value


@pytest.fixture(scope="module")
def sb_exact():
    import pyclaw_amd as pyclaw
    return sb_inflow_run(pyclaw)


def test_resident_run_takes_no_step_ahead_and_meets_the_golden(sb_exact, sb_gold):
    dens, steps, enqueued = sb_exact
    print("resident CellBC run: steps %d, enqueued ahead %d, max |density - golden| = %g"
          % (steps, enqueued, np.abs(dens - sb_gold).max()))
    assert steps == 170
    assert enqueued == 0
    assert np.max(np.abs(dens - sb_gold)) < 1e-12


def test_fast_math_agrees_with_exact(sb_exact):
    import pyclaw_amd as pyclaw
    exact = sb_exact[0]
    dens, steps, _ = sb_inflow_run(pyclaw, math='fast')
    print("fast: steps %d, max rel. difference to exact %g" % (steps, np.max(np.abs(dens - exact) / np.abs(exact))))
    assert steps == 170
    assert np.max(np.abs(dens - exact) / np.abs(exact)) < RTOL


# ---- 7: two ranks on one GPU ------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_cut_in_y(tmp_path):
    """24 x 18 acoustics cut in y: the lower x side (both ranks own a part of it) stamps the GLOBAL c.i[1] into the
    pressure, the upper y side (the second rank's alone) extrapolates; 8 steps, against the single block, bit for bit."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import cellbc_mp_worker as W
    finally:
        sys.path.pop(0)
    q = W.run_case()[0]["q"]
    assert len(np.unique(q[0, 0, :])) > 9              # the stamp reached the interior, row by row
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, q=q)
    port = free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port), "PCL_HALO_TRANSPORT": "host", "PCL_FORCE_DEVICE": "0",
                    "PCL_PROC_GRID": "1x2", "TORCHELASTIC_RUN_ID": "cb%d" % port})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "cellbc_mp_worker.py"), ref],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=120)
            outs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    codes = [p.returncode for p in procs]
    assert codes == [0, 0], "exit codes %s\n%s" % (codes, "\n----\n".join(o[-1500:] for o in outs))
    assert "cut in y: True" in outs[0] and "bit-identical: True" in outs[0], outs[0][-1500:]
