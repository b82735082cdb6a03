"""
GPU: cell functions that read neighbour cells (``reach > 0``: qn / auxn) as start_step, step_src and dq_src, each against
the numpy callback it stands in for.  The numpy twins (apps/problems.py) form the right-hand side from a padded copy of
the OLD interior -- np.pad in the mode of each side's boundary condition, x first -- and then assign.  Every comparison is
bit for bit in 'exact' mode; 'fast' is held to the project's gate.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from apps import problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12                      # the project's gate for PCL_MATH_FAST (tests/test_gpu_apps.py)
NU = 0.01


def advection_1d(pyclaw, mx=300, meqn_two=False):
    """periodic 1-D problem: advection (meqn 1) or acoustics (meqn 2)"""
    solver = pyclaw.ClawSolver1D()
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx)), 2 if meqn_two else 1)
    xc = state.grid.x.center
    if meqn_two:
        solver.rp = pyclaw.riemann.rp_acoustics_1d
        solver.mwaves = 2
        solver.limiters = [4, 4]
        state.aux_global.update(rho=1.0, bulk=1.0, zz=1.0, cc=1.0)
        state.q[1, :] = 0.3 * np.sin(2 * np.pi * xc) + 0.01 * xc
    else:
        solver.rp = pyclaw.riemann.rp_advection_1d
        solver.mwaves = 1
        state.aux_global['u'] = 1.
    state.q[0, :] = np.exp(-100 * (xc - 0.75) ** 2) + 0.25 * xc
    return solver, pyclaw.Solution(state)


# ---- 1: the snapshot, across lanes, wavefronts and workgroups ---------------------------------------------------------
def test_shift_1d_crosses_workgroups():
    """mx = 300: lanes 255 | 256 sit in different workgroups, the last workgroup holds 44 lanes.  Every cell takes its
    left neighbour's OLD value: a launch that read q in place would hand some lanes a value already shifted."""
    import pyclaw_amd as pyclaw

    def hook(solver, solution):
        q = solution.state.q
        q[0] = np.roll(q[0], 1)

    def run(start_step):
        solver, solution = advection_1d(pyclaw)
        solver.start_step = start_step
        return problems.fixed_steps(solver, solution, 5, 0.8 / 300)

    ref, cell = run(hook), run(pyclaw.CellStartStep("q[0] = qn(0, -1);", reach=1))
    print("1-D shift: max |cell - numpy| = %g" % np.abs(cell - ref).max())
    assert np.array_equal(cell, ref)
    plain = run(None)
    assert not np.array_equal(plain, ref)


def test_shift_2d_in_y_every_row_another_workgroup():
    import pyclaw_amd as pyclaw

    def hook(solver, solution):
        q = solution.state.q
        q[0] = np.roll(q[0], 1, axis=1)

    def run(start_step):
        solver, solution = problems.advection2D(pyclaw, 37, 21)
        solver.start_step = start_step
        return problems.fixed_steps(solver, solution, 5, 0.4 / 37)

    ref, cell = run(hook), run(pyclaw.CellStartStep("q[0] = qn(0, 0, -1);", reach=1))
    print("2-D shift in y: max |cell - numpy| = %g" % np.abs(cell - ref).max())
    assert np.array_equal(cell, ref)
    assert not np.array_equal(run(None), ref)


# ---- 2: corners ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y", ["periodic", "extrapolation"])
def test_diagonal_neighbours_read_the_corner_ghost_cells(y):
    import pyclaw_amd as pyclaw
    bc_y, modes = (None, ['wrap', 'wrap']) if y == "periodic" else (pyclaw.BC.outflow, ['wrap', 'edge'])

    def run(start_step):
        solver, solution = problems.advection2D(pyclaw, 37, 21, bc_y=bc_y)
        solver.start_step = start_step
        return problems.fixed_steps(solver, solution, 4, 0.4 / 37)

    ref = run(problems.diagonal_mean_hook(modes))
    cell = run(pyclaw.CellStartStep(problems.DIAGONAL_MEAN_CELL_HOOK, reach=1))
    print("corners, y %s: max |cell - numpy| = %g" % (y, np.abs(cell - ref).max()))
    assert np.array_equal(cell, ref)
    if y == "periodic":        # np.roll on both axes is the same thing there
        def rolled(solver, solution):
            q = solution.state.q
            r = lambda a, b: np.roll(np.roll(q[0], -a, axis=0), -b, axis=1)
            q[0] = 0.25 * (r(1, 1) + r(-1, 1) + r(1, -1) + r(-1, -1))
        assert np.array_equal(run(rolled), ref)


# ---- 3, 11: a Godunov-split source on the classic solver ---------------------------------------------------------------
def acoustics_diffusion(pyclaw, src, math='exact'):
    claw = problems.acoustics2D(pyclaw, mx=37, my=21, tfinal=0.05, nout=1, run=False, math=math)
    claw.solver.step_src = src
    claw.run()
    return claw


@pytest.fixture(scope="module")
def acoustics_diffusion_exact():
    import pyclaw_amd as pyclaw
    return acoustics_diffusion(pyclaw, pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC, params=[NU, 0], reach=1))


def test_diffusion_source_godunov(acoustics_diffusion_exact):
    import pyclaw_amd as pyclaw
    cell = acoustics_diffusion_exact
    ref = acoustics_diffusion(pyclaw, problems.diffusion_src(NU, ['edge', 'edge']))
    plain = acoustics_diffusion(pyclaw, None)
    q, want = cell.frames[1].state.q, ref.frames[1].state.q
    print("diffusion source: steps %d (numpy %d), max |cell - numpy| = %g"
          % (cell.solver.status['numsteps'], ref.solver.status['numsteps'], np.abs(q - want).max()))
    assert cell.solver.status['numsteps'] == ref.solver.status['numsteps'] >= 2
    assert np.array_equal(q, want)
    assert not np.array_equal(plain.frames[1].state.q, want)


def test_diffusion_source_fast(acoustics_diffusion_exact):
    """'fast' contracts the body's multiply-adds (and the sweeps'): held to 1e-12 of the largest |q| of the exact run --
    the fields cross zero, so a cell-wise relative difference has no meaning here (as in tests/test_gpu_cellfn.py's
    p-system test)."""
    import pyclaw_amd as pyclaw
    exact = acoustics_diffusion_exact
    fast = acoustics_diffusion(pyclaw, pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC, params=[NU, 0], reach=1), math='fast')
    q, want = fast.frames[1].state.q, exact.frames[1].state.q
    err = np.abs(q - want).max() / np.abs(want).max()
    print("fast: steps %d, max |fast - exact| / max |exact| = %g" % (fast.solver.status['numsteps'], err))
    assert fast.solver.status['numsteps'] == exact.solver.status['numsteps']
    assert err < RTOL


# ---- 4: Strang splitting and a rejected step ----------------------------------------------------------------------------
def test_strang_diffusion_source_with_a_rejected_step():
    """The 40 x 10 shock-bubble with dt_initial = 0.05 (the configuration of tests/test_gpu_cellfn.py's Strang test) and
    diffusion of the density alone as the source: custom inflow (a Python callback), extrapolation, a wall and
    extrapolation again around the block.  Strang calls the source twice in an accepted step and once in a rejected one."""
    import pyclaw_amd as pyclaw
    rinf, vinf, einf = problems.shock_state()
    modes = [([rinf, rinf * vinf, 0., einf, 0.], 'edge'), ('wall', 'edge')]
    nu = 0.001

    def run(src):
        claw = problems.shockbubble(pyclaw, mx=40, my=10, tfinal=0.02, run=False, dt_initial=0.05)
        claw.solver.src_split = 2
        claw.solver.step_src = src
        claw.run()
        return claw

    calls = []
    ref = run(problems.diffusion_src(nu, modes, ncomp=1, calls=calls))
    cell = run(pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC, params=[nu, 1], reach=1))
    steps = ref.solver.status['numsteps']
    rejected = len(calls) - 2 * steps
    q, want = cell.frames[1].state.q, ref.frames[1].state.q
    print("strang: steps %d (numpy %d), rejected %d, max |cell - numpy| = %g"
          % (cell.solver.status['numsteps'], steps, rejected, np.abs(q - want).max()))
    assert rejected >= 1
    assert cell.solver.status['numsteps'] == steps
    assert np.array_equal(q, want)
    assert not np.array_equal(run(None).frames[1].state.q, want)


# ---- 5: SharpClaw ------------------------------------------------------------------------------------------------------
def sharp_1d(pyclaw, mx=300):
    solver = pyclaw.SharpClawSolver1D()
    solver.time_integrator = 'SSP33'
    solver.rp = pyclaw.riemann.rp_acoustics_1d
    solver.mwaves = 2
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx)), 2)
    state.aux_global.update(rho=1.0, bulk=1.0, zz=1.0, cc=1.0)
    xc = state.grid.x.center
    state.q[0, :] = np.exp(-100 * (xc - 0.75) ** 2)
    state.q[1, :] = 0.1 * np.sin(2 * np.pi * xc)
    solver.dt_initial = 0.5 / mx
    claw = pyclaw.Controller()
    claw.keep_copy = True
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    claw.tfinal, claw.nout = 0.01, 1
    return claw


def sharp_claw(pyclaw, ndim):
    if ndim == 1:
        return sharp_1d(pyclaw), ['wrap']
    return problems.acoustics2D(pyclaw, mx=37, my=21, tfinal=0.03, nout=1, solver_type='sharpclaw', time_integrator='SSP33',
                                run=False), ['edge', 'edge']


@pytest.mark.parametrize("ndim", [1, 2])
def test_sharpclaw_laplacian_dq_source(ndim):
    import pyclaw_amd as pyclaw
    nu = 1e-4 if ndim == 1 else NU

    def run(make):
        claw, modes = sharp_claw(pyclaw, ndim)
        claw.solver.dq_src = make(modes)
        claw.run()
        assert claw.solver.mbc == 3
        return claw

    ref = run(lambda modes: problems.laplacian4_dq_src(nu, modes))
    cell = run(lambda modes: pyclaw.CellDqSource(problems.LAPLACIAN4_DQ_CELL_SRC, params=[nu], reach=2))
    plain = run(lambda modes: None)
    q, want = cell.frames[1].state.q, ref.frames[1].state.q
    print("SharpClaw %d-D dq_src: steps %d (numpy %d), max |cell - numpy| = %g"
          % (ndim, cell.solver.status['numsteps'], ref.solver.status['numsteps'], np.abs(q - want).max()))
    assert cell.solver.status['numsteps'] == ref.solver.status['numsteps'] > 1
    assert np.array_equal(q, want)
    assert not np.array_equal(plain.frames[1].state.q, want)


@pytest.mark.parametrize("ndim", [1, 2])
def test_sharpclaw_smoothing_start_step(ndim):
    import pyclaw_amd as pyclaw
    body = "q[0] = 0.25 * qn(0, -1) + 0.5 * qn(0, 0) + 0.25 * qn(0, 1);"

    def run(make):
        claw, modes = sharp_claw(pyclaw, ndim)
        claw.solver.start_step = make(modes)
        claw.run()
        return claw

    def python_hook(modes):
        def start_step(solver, solution):
            q = solution.state.q
            qb = problems.pad_like_bcs(q, 1, modes)
            zero = (0,) * (ndim - 1)
            sh = lambda o: problems.shifted(qb, 1, (o,) + zero)[0]
            q[0] = 0.25 * sh(-1) + 0.5 * sh(0) + 0.25 * sh(1)
        return start_step

    ref = run(python_hook)
    cell = run(lambda modes: pyclaw.CellStartStep(body, reach=1))
    q, want = cell.frames[1].state.q, ref.frames[1].state.q
    print("SharpClaw %d-D start_step: steps %d, max |cell - numpy| = %g"
          % (ndim, cell.solver.status['numsteps'], np.abs(q - want).max()))
    assert cell.solver.status['numsteps'] == ref.solver.status['numsteps'] > 1
    assert np.array_equal(q, want)


# ---- 6: 3-D ---------------------------------------------------------------------------------------------------------------
def test_diffusion_source_3d():
    import pyclaw_amd as pyclaw

    def run(src):
        claw = problems.acoustics3D(pyclaw, test='hom', mx=9, my=7, mz=5, run=False, tfinal=0.3, nout=1)
        # (the problem's own data vary in x alone: give the other two directions something to diffuse)
        X, Y, Z = claw.solution.state.grid._c_center
        claw.solution.state.q[1] = 0.1 * np.sin(np.pi * Y) + 0.05 * np.cos(np.pi * Z) * X
        claw.solver.step_src = src
        claw.run()
        return claw

    ref = run(problems.diffusion_src(NU, ['wrap'] * 3))
    cell = run(pyclaw.CellSource(problems.DIFFUSION_3D_CELL_SRC, params=[NU, 0], reach=1))
    q, want = cell.frames[1].state.q, ref.frames[1].state.q
    print("3-D diffusion source: steps %d, max |cell - numpy| = %g" % (cell.solver.status['numsteps'], np.abs(q - want).max()))
    assert cell.solver.mbc == 2
    assert cell.solver.status['numsteps'] == ref.solver.status['numsteps'] >= 2
    assert np.array_equal(q, want)
    assert not np.array_equal(run(None).frames[1].state.q, want)


# ---- 7: aux neighbours -------------------------------------------------------------------------------------------------
def test_aux_gradient_source():
    import pyclaw_amd as pyclaw
    g = 0.5

    def run(src):
        claw = problems.vc_acoustics2D(pyclaw, mx=37, my=21, tfinal=0.05, nout=1, run=False)
        claw.solver.step_src = src
        claw.run()
        return claw

    ref = run(problems.aux_gradient_src(g))
    cell = run(pyclaw.CellSource(problems.AUX_GRADIENT_CELL_SRC, params=[g], reach=1))
    q, want = cell.frames[1].state.q, ref.frames[1].state.q
    print("aux gradient: steps %d, max |cell - numpy| = %g" % (cell.solver.status['numsteps'], np.abs(q - want).max()))
    assert cell.solver.status['numsteps'] == ref.solver.status['numsteps'] >= 2
    assert np.array_equal(q, want)
    assert not np.array_equal(run(None).frames[1].state.q, want)


# ---- 8: the clamps ------------------------------------------------------------------------------------------------------
def test_offsets_and_components_are_clamped():
    """mbc = 2, reach = 1: an offset of 2 and a component MEQN, both run-time values taken from p[], read what offset 1
    and component MEQN - 1 read.  Unclamped, the offset would land in the second ghost layer -- inside the block, other
    numbers."""
    import pyclaw_amd as pyclaw

    def hook(solver, solution):
        q = solution.state.q
        q[0] = np.roll(q[0], -1) + np.roll(q[1], -1)

    def run(start_step):
        solver, solution = advection_1d(pyclaw, meqn_two=True)
        solver.start_step = start_step
        q = problems.fixed_steps(solver, solution, 3, 0.4 / 300)
        assert solver.mbc == 2
        return q

    ref = run(hook)
    cell = run(pyclaw.CellStartStep("q[0] = qn(0, (int)p[0]) + qn((int)p[1], 1);", params=[2, 2], reach=1))
    honest = run(pyclaw.CellStartStep("q[0] = qn(0, 1) + qn(1, 1);", reach=1))
    low = run(pyclaw.CellStartStep("q[0] = qn(0, -(int)p[0]) + qn(-(int)p[1], -1);", params=[7, 3], reach=1))

    def low_hook(solver, solution):
        q = solution.state.q
        q[0] = np.roll(q[0], 1) + np.roll(q[0], 1)

    print("clamp: max |cell - numpy| = %g" % np.abs(cell - ref).max())
    assert np.array_equal(cell, ref) and np.array_equal(honest, ref)
    assert np.array_equal(low, run(low_hook))


# ---- 9: untouched storage ----------------------------------------------------------------------------------------------
def test_ghost_frame_and_unassigned_components_are_left_alone():
    """One launch on a random ghosted array: the ghost frame afterwards is the frame apply_q_bcs produced, bit for bit, the
    components the body does not assign keep their bits, and the assigned one is the numpy stencil over that frame --
    random ghost values, so a read that missed its ghost cell shows."""
    import pyclaw_amd as pyclaw
    from pyclaw_amd import _lib
    claw = problems.acoustics2D(pyclaw, mx=37, my=21, run=False)
    solver, state = claw.solver, claw.solution.state
    solver.setup(claw.solution)
    solver._push(state)
    L = _lib.lib()
    up = np.asfortranarray(np.random.default_rng(5).standard_normal(solver.qbc.shape))
    _lib.check(L.pcl_put_q(solver._h, _lib.d(up), 1))
    solver.apply_q_bcs(state)
    framed = np.empty(up.shape, order='F')
    _lib.check(L.pcl_get_q(solver._h, _lib.d(framed), 1))
    _lib.check(L.pcl_put_q(solver._h, _lib.d(up), 1))
    pyclaw.CellSource("q[0] = qn(0, 1, 0) - qn(0, 0, -1) + 2.0 * qn(2, -1, 1);", reach=1).apply(solver, state, 0.0)
    back = np.empty(up.shape, order='F')
    _lib.check(L.pcl_get_q(solver._h, _lib.d(back), 1))
    solver.teardown()
    mbc = solver.mbc
    inner = (slice(None), slice(mbc, -mbc), slice(mbc, -mbc))
    assert np.array_equal(framed[inner], up[inner]) and not np.array_equal(framed, up)
    ghosts = np.ones(up.shape, dtype=bool)
    ghosts[inner] = False
    assert np.array_equal(back[ghosts].view(np.uint64), framed[ghosts].view(np.uint64))
    assert np.array_equal(back[1:].view(np.uint64), framed[1:].view(np.uint64))
    sh = lambda m, a, b: framed[m, mbc + a:framed.shape[1] - mbc + a, mbc + b:framed.shape[2] - mbc + b]
    assert np.array_equal(back[inner][0], sh(0, 1, 0) - sh(0, 0, -1) + 2.0 * sh(2, -1, 1))


# ---- 10: two ranks on one GPU -------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(case, ref_file, nranks=2):
    port = free_port()
    procs = []
    for r in range(nranks):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(nranks), "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port), "PCL_HALO_TRANSPORT": "host", "PCL_FORCE_DEVICE": "0",
                    "PCL_PROC_GRID": "%dx1" % nranks, "TORCHELASTIC_RUN_ID": "cr%d" % port})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "cellfn_reach_mp_worker.py"), case, ref_file],
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
    assert codes == [0] * nranks, "exit codes %s\n%s" % (codes, "\n----\n".join(o[-1500:] for o in outs))
    assert "bit-identical: True" in outs[0], outs[0][-1500:]


def test_two_ranks_diagonal_hook_and_diffusion_source(tmp_path):
    """40 x 24, periodic, cut in x: the diagonal body reads the corner ghost cells next to the neighbour block, the source
    the columns next to it -- both filled by the halo exchange of the apply_q_bcs in front of the launch."""
    import pyclaw_amd as pyclaw
    solver, solution = problems.advection2D(pyclaw, 40, 24)
    solver.start_step = pyclaw.CellStartStep(problems.DIAGONAL_MEAN_CELL_HOOK, reach=1)
    solver.step_src = pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC, params=[NU, 0], reach=1)
    q = problems.fixed_steps(solver, solution, 4, 0.01)
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, q=q, nu=NU, dt=0.01, nsteps=4)
    launch("advection", ref)


# ---- the library's own check behind the Python one ----------------------------------------------------------------------
def test_library_refuses_a_reach_beyond_mbc():
    import ctypes as C
    import pyclaw_amd as pyclaw
    from pyclaw_amd import _lib
    solver, solution = advection_1d(pyclaw, mx=40)
    solver.setup(solution)
    solver._push(solution.state)
    L = _lib.lib()
    fn = C.c_void_p()
    _lib.check(L.pcl_cellfn_compile_reach(1, b"q[0] = qn(0, 3);", b"", 1, 0, 1, 0, 0, 3, C.byref(fn), None))
    rc = L.pcl_cellfn_apply(solver._h, fn, 0.0, 0.0, None, 0)
    msg = L.pcl_last_error().decode()
    L.pcl_cellfn_release(fn)
    solver._pull(solution.state)
    solver.teardown()
    assert rc == _lib.EINVAL and "reads 3 cells away" in msg and "mbc = 2" in msg
