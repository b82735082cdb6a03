"""
GPU: cell functions -- user-written per-cell C++ compiled at setup() and run on the resident arrays -- as step_src
(CellSource), dq_src (CellDqSource) and start_step (CellStartStep, with and without writes_aux), against the reference's
golden file, the oracle replay and the Python callbacks they stand in for.  Every comparison is bit for bit in 'exact'
mode; 'fast' is held to the gate of tests/test_gpu_apps.py.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import driver as D
from oracle import oracle as O
from apps import problems
from apps import psystem as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12                      # the project's gate for PCL_MATH_FAST (tests/test_gpu_apps.py)
NOOP = "(void)c;"                 # a start_step body that leaves q alone


def euler_cell_source(pyclaw):
    return pyclaw.CellSource(problems.EULER_RAD_CELL_SRC, params=[problems.gamma1, 2])


@pytest.fixture(scope="module")
def sb_gold(golden_dir):
    return np.loadtxt(os.path.join(golden_dir, "sb_density"))


# ---- 5: shock-bubble against the reference golden ----------------------------------------------------------------------
def test_shockbubble_cell_source_golden(sb_gold, monkeypatch):
    import pyclaw_amd as pyclaw
    claw = problems.shockbubble(pyclaw, run=False)
    claw.solver.step_src = euler_cell_source(pyclaw)
    claw.run()
    q = claw.frames[claw.nout].state.q
    print("cell source: steps %d, max |density - golden| = %g" % (claw.solver.status['numsteps'], np.abs(q[0] - sb_gold).max()))
    assert claw.solver.status['numsteps'] == 170
    assert np.array_equal(q[0], sb_gold)
    # the built-in source as a kernel of its own (not fused into the y pass): the same q
    monkeypatch.setenv("PCL_FUSE_SRC", "0")
    ref = problems.shockbubble(pyclaw, run=False)
    ref.solver.step_src = pyclaw.EulerRadialSource(problems.gamma1, 2)
    ref.run()
    assert not ref.solver._src_fused
    assert np.array_equal(q, ref.frames[ref.nout].state.q)


# ---- 6: Strang splitting, a start_step hook and a rejected step ---------------------------------------------------------
def test_strang_cell_source_and_cell_start_step(coracle):
    import pyclaw_amd as pyclaw
    claw = problems.shockbubble(pyclaw, mx=40, my=10, tfinal=0.02, run=False, dt_initial=0.05)
    claw.solver.src_split = 2
    claw.solver.step_src = euler_cell_source(pyclaw)
    claw.solver.start_step = pyclaw.CellStartStep(NOOP)
    claw.run()
    assert claw.solver._pre_step_modifies_q()
    p = D.shockbubble_problem(mx=40, my=10, dt_initial=0.05)
    p.src_split = 2
    st = D.run(p, coracle, 0.02, 1)[-1]
    print("strang: steps %d (replay %d), rejected in the replay %d" % (claw.solver.status['numsteps'], st['numsteps'], p.nrejected))
    assert p.nrejected >= 1
    assert claw.solver.status['numsteps'] == st['numsteps']
    assert np.array_equal(claw.frames[1].state.q, p.q)


# ---- 7: SharpClaw dq_src -----------------------------------------------------------------------------------------------
def test_sharpclaw_cell_dq_source():
    import pyclaw_amd as pyclaw

    def run(dq_src):
        claw = problems.shockbubble(pyclaw, mx=40, my=10, tfinal=0.01, solver_type='sharpclaw', time_integrator='SSP33',
                                    run=False)
        if dq_src is not None:
            claw.solver.dq_src = dq_src
        claw.run()
        return claw

    python = run(None)                          # problems.dq_euler_radial, through the host
    assert python.solver.dq_src is problems.dq_euler_radial and python.solver.weno_order == 5
    cell = run(pyclaw.CellDqSource(problems.DQ_EULER_RAD_CELL_SRC, params=[problems.gamma1, 2]))
    builtin = run(pyclaw.EulerRadialDqSource(problems.gamma1, 2))
    assert not cell.solver._dq_src_fused
    assert cell.solver.status['numsteps'] == python.solver.status['numsteps'] == builtin.solver.status['numsteps'] > 0
    print("dq_src: steps %d, max |cell - python| = %g, max |cell - built-in| = %g"
          % (cell.solver.status['numsteps'], np.abs(cell.frames[1].state.q - python.frames[1].state.q).max(),
             np.abs(cell.frames[1].state.q - builtin.frames[1].state.q).max()))
    assert np.array_equal(cell.frames[1].state.q, python.frames[1].state.q)
    assert np.array_equal(cell.frames[1].state.q, builtin.frames[1].state.q)


def test_sharpclaw_cell_start_step():
    """a before-step hook that changes q, on the SharpClaw solver: the cell function against the Python hook"""
    import pyclaw_amd as pyclaw

    def python_hook(solver, solution):
        q = solution.state.q
        q[0] = q[0] - solver.dt * 0.5 * q[0]

    def run(hook):
        claw = problems.acoustics2D(pyclaw, mx=37, my=21, tfinal=0.03, nout=1, solver_type='sharpclaw',
                                    time_integrator='SSP33', run=False)
        claw.solver.start_step = hook
        claw.run()
        return claw

    ref = run(python_hook)
    cell = run(pyclaw.CellStartStep("q[0] = q[0] - c.dt * p[0] * q[0];", params=[0.5]))
    plain = problems.acoustics2D(pyclaw, mx=37, my=21, tfinal=0.03, nout=1, solver_type='sharpclaw', time_integrator='SSP33')
    assert cell.solver.status['numsteps'] == ref.solver.status['numsteps'] > 1
    print("SharpClaw start_step: steps %d, max |cell - python| = %g"
          % (cell.solver.status['numsteps'], np.abs(cell.frames[1].state.q - ref.frames[1].state.q).max()))
    assert np.array_equal(cell.frames[1].state.q, ref.frames[1].state.q)
    assert not np.array_equal(plain.frames[1].state.q, ref.frames[1].state.q)


# ---- 8: coordinates, parameters, a last wavefront that is not full -------------------------------------------------------
def test_coordinates_and_params_1d():
    import pyclaw_amd as pyclaw
    mx = 67

    def run(make_src, set_rate):
        solver = pyclaw.ClawSolver1D()
        solver.rp = pyclaw.riemann.rp_advection_1d
        solver.mwaves = 1
        solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
        solver.dt_variable = False
        state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.5, 1.75, mx)), 1)
        state.aux_global['u'] = 1.
        xc = state.grid.x.center
        state.q[0, :] = np.exp(-100 * (xc - 1.0) ** 2) + 0.25
        solution = pyclaw.Solution(state)
        solver.step_src = make_src(state)
        solver.setup(solution)
        solver.dt = 0.8 * state.grid.d[0]
        for n in range(5):
            if n == 2:
                set_rate(solver, 0.75)
            solver.evolve_to_time(solution)
        solver.teardown()
        return solution.state.q.copy()

    rate = [0.3]

    def numpy_src(state):
        rate[0] = 0.3
        return lambda solver, st, dt: st.q.__setitem__(0, st.q[0] - dt * rate[0] * st.grid.x.center * st.q[0])

    ref = run(numpy_src, lambda solver, v: rate.__setitem__(0, v))
    cell = run(lambda state: pyclaw.CellSource("q[0] = q[0] - c.dt * p[0] * c.x[0] * q[0];", params=[0.3]),
               lambda solver, v: setattr(solver.step_src, 'params', [v]))
    print("1-D coordinates: max |cell - numpy| = %g" % np.abs(cell - ref).max())
    assert np.array_equal(cell, ref)
    unchanged = run(numpy_src, lambda solver, v: None)
    assert not np.array_equal(unchanged, ref)          # the reassigned parameter is what the result shows


# ---- 9: index stamps, untouched ghost cells ---------------------------------------------------------------------------
STAMP = {2: "for (int m = 0; m < MEQN; m++) q[m] = c.i[0] + 1000.0 * c.i[1] + 0.25 * m;",
         3: "for (int m = 0; m < MEQN; m++) q[m] = c.i[0] + 1000.0 * c.i[1] + 1e6 * c.i[2] + 0.25 * m;"}


def stamp_run(pyclaw, claw, seed=3):
    """upload a random ghosted array, stamp the interior, read the ghosted array back: (uploaded, read back)"""
    from pyclaw_amd import _lib
    solver, state = claw.solver, claw.solution.state
    solver.setup(claw.solution)
    solver._push(state)
    up = np.asfortranarray(np.random.default_rng(seed).standard_normal(solver.qbc.shape))
    _lib.check(_lib.lib().pcl_put_q(solver._h, _lib.d(up), 1))
    pyclaw.CellSource(STAMP[solver.ndim]).apply(solver, state, 0.0)
    back = np.empty(up.shape, order='F')
    _lib.check(_lib.lib().pcl_get_q(solver._h, _lib.d(back), 1))
    solver.teardown()
    return up, back


@pytest.mark.parametrize("ndim", [2, 3])
def test_index_stamps_and_untouched_ghosts(ndim):
    import pyclaw_amd as pyclaw
    if ndim == 2:
        claw = problems.acoustics2D(pyclaw, mx=65, my=3, run=False)
    else:
        claw = problems.acoustics3D(pyclaw, test='hom', mx=9, my=5, mz=4, run=False)
    meqn = claw.solution.state.meqn
    assert meqn == (3 if ndim == 2 else 4)
    up, back = stamp_run(pyclaw, claw)
    mbc = claw.solver.mbc
    inner = (slice(None),) + (slice(mbc, -mbc),) * ndim
    idx = np.meshgrid(*[np.arange(n) for n in claw.solution.state.grid.ng], indexing="ij")
    want = idx[0] + 1000.0 * idx[1] + (1e6 * idx[2] if ndim == 3 else 0.0)
    for m in range(meqn):
        assert np.array_equal(back[inner][m], want + 0.25 * m)
    ghosts = np.ones(up.shape, dtype=bool)
    ghosts[inner] = False
    assert np.array_equal(back[ghosts].view(np.uint64), up[ghosts].view(np.uint64))


# ---- 10: fast mode -----------------------------------------------------------------------------------------------------
def test_shockbubble_cell_source_fast(sb_gold):
    import pyclaw_amd as pyclaw
    claw = problems.shockbubble(pyclaw, math='fast', run=False)
    claw.solver.step_src = euler_cell_source(pyclaw)
    claw.run()
    dens = claw.frames[claw.nout].state.q[0]
    print("fast: steps %d, max rel. difference to the golden %g"
          % (claw.solver.status['numsteps'], np.max(np.abs(dens - sb_gold) / np.abs(sb_gold))))
    assert claw.solver.status['numsteps'] == 170
    assert np.max(np.abs(dens - sb_gold) / np.abs(sb_gold)) < RTOL


# ---- 11: time-dependent aux on one block --------------------------------------------------------------------------------
NSTEPS = 8


def psystem_claw(pyclaw, bc, hook=True, linearity=1):
    # the exponential law with a smaller pulse: its sound speed grows with the strain, and the step length is fixed
    claw = PS.psystem2D(pyclaw, solver_type='classic_unsplit', mx=24, my=20, linearity=linearity, bc=bc,
                        upper=(4.25, 4.25), amplitude=10.0 if linearity == 1 else 1.0, run=False)
    solver = claw.solver
    if not hook:
        solver.start_step = None
    solver.dt_variable = False
    claw.tfinal, claw.nout = NSTEPS * solver.dt_initial, 1
    return claw


def psystem_run(claw):
    """NSTEPS fixed steps: (q, state.aux as the host sees it afterwards, the resident aux WITH its ghost cells)"""
    from pyclaw_amd import _lib
    solver, solution = claw.solver, claw.solution
    solver.setup(solution)
    solver.dt = solver.dt_initial
    solver.evolve_to_time(solution, claw.tfinal)
    assert solver.status['numsteps'] == NSTEPS
    auxbc = np.empty(solver.auxbc.shape, order='F')
    _lib.check(_lib.lib().pcl_get_aux(solver._h, _lib.d(auxbc)))
    solver.teardown()
    return solution.state.q.copy('F'), solution.state.aux.copy('F'), auxbc


def psystem_oracle(coracle, claw):
    """the same steps on the oracle, the strain copy and its ghost cells refreshed by hand before every step:
    (q, ghosted aux as the last step saw it, ghosted aux as set-up filled it)"""
    solver, state = claw.solver, claw.solution.state
    kinds = {0: D.CUSTOM, 1: D.OUTFLOW, 2: D.PERIODIC, 3: D.REFLECTING}
    lo, hi = [kinds[b] for b in solver.bc_lower], [kinds[b] for b in solver.bc_upper]
    p = D.Problem(q=state.q.copy('F'), aux=state.aux.copy('F'), rp=O.RP_PSYSTEM_FWAVE_2D, rp_params=[0.0], mwaves=2,
                  limiters=solver.limiters, bc_lower=lo, bc_upper=hi, aux_bc_lower=lo, aux_bc_upper=hi,
                  d=tuple(state.grid.d), dim_split=False, order_trans=2, fwave=True, dt_initial=solver.dt_initial)
    D.setup(p)
    first = p.auxbc.copy('F')
    inner = (slice(None), slice(p.mbc, -p.mbc), slice(p.mbc, -p.mbc))
    for n in range(NSTEPS):
        p.aux[3] = p.q[0]
        p.auxbc[inner] = p.aux
        D.fill_ghosts(p.auxbc, p.mbc, p.aux_bc_lower, p.aux_bc_upper, is_aux=True)
        D.step_hyperbolic(p, coracle)
        assert p.cfl <= 1.0
        p.t += p.dt
    return np.array(p.q, order='F'), p.auxbc.copy('F'), first


def ghost_mask(auxbc, mbc=2):
    ghosts = np.ones(auxbc.shape, dtype=bool)
    ghosts[:, mbc:-mbc, mbc:-mbc] = False
    return ghosts


@pytest.mark.parametrize("bc", ["periodic", "reference"])
def test_psystem_unsplit_with_strain_hook(coracle, bc):
    """Linear stress law: bit for bit against the oracle loop -- q, the strain copy read back, and the resident aux
    with its ghost cells (pcl_get_aux) against the oracle's auxbc, which is what shows the ghost refresh behind the hook:
    periodic copies, and wall / extrapolation fills of pcl_bc_aux.

    Under the linear law sigma' = K does not depend on the strain, so rpt2_psystem never uses the value of aux(4) and q
    cannot tell a run with the hook from one without (measured: the two are equal bit for bit).  What the hook changes
    there is aux itself: the run without it ends with the INITIAL strain in aux(4), which is not the oracle loop's.
    test_psystem_exponential_law_needs_the_hook shows the hook, and the ghost cells, in q."""
    import pyclaw_amd as pyclaw
    claw = psystem_claw(pyclaw, bc)
    want, want_auxbc, first_auxbc = psystem_oracle(coracle, claw)
    q, aux, auxbc = psystem_run(claw)
    ghosts = ghost_mask(auxbc)
    print("p-system %s: max |q - oracle| = %g, max |aux - oracle| = %g, over the ghost cells %g"
          % (bc, np.abs(q - want).max(), np.abs(aux - want_auxbc[:, 2:-2, 2:-2]).max(),
             np.abs(auxbc[ghosts] - want_auxbc[ghosts]).max()))
    assert np.array_equal(q, want)
    assert np.array_equal(aux, want_auxbc[:, 2:-2, 2:-2])                  # state.aux follows the device
    assert np.array_equal(auxbc.view(np.uint64), want_auxbc.view(np.uint64))
    # the ghost cells are not the ones set-up uploaded, and the interior strain is not the initial one
    assert not np.array_equal(want_auxbc[ghosts], first_auxbc[ghosts])
    assert not np.array_equal(want_auxbc[3, 2:-2, 2:-2], first_auxbc[3, 2:-2, 2:-2])
    plain_q, plain_aux, plain_auxbc = psystem_run(psystem_claw(pyclaw, bc, hook=False))
    assert np.array_equal(plain_auxbc, first_auxbc)
    assert not np.array_equal(plain_auxbc, want_auxbc)                     # the hook is what the comparison sees


@pytest.mark.parametrize("bc", ["periodic", "reference"])
def test_psystem_exponential_law_needs_the_hook(coracle, bc):
    """sigma = exp(K eps) - 1: rpt2_psystem evaluates sigma'(aux(4)) of the neighbouring rows, ghost rows included, so a
    stale strain copy -- or stale ghost cells of it -- changes q.  The device's exp() and the oracle's differ by an ulp
    (tests/test_fwave.py), so this comparison takes the project's gate for arithmetic that is not bit-identical, 1e-12 of
    the largest |q|: an ulp (1.1e-16) per exp(), a few of them per cell and step, 8 steps of a scheme run at CFL 0.4
    stay two orders below it.  The run without the hook must miss that gate by orders of magnitude for the gate to tell
    the two apart: 1e-9 is asked."""
    import pyclaw_amd as pyclaw
    claw = psystem_claw(pyclaw, bc, linearity=2)
    want, want_auxbc, first_auxbc = psystem_oracle(coracle, claw)
    q, aux, auxbc = psystem_run(claw)
    plain_q = psystem_run(psystem_claw(pyclaw, bc, hook=False, linearity=2))[0]
    scale = np.abs(want).max()
    err, err_plain = np.abs(q - want).max() / scale, np.abs(plain_q - want).max() / scale
    err_aux = np.abs(auxbc[3] - want_auxbc[3]).max() / np.abs(want_auxbc[3]).max()
    print("p-system %s, exponential law: |q - oracle| / max|q| = %g with the hook, %g without; strain copy with ghosts %g"
          % (bc, err, err_plain, err_aux))
    assert err < RTOL
    assert err_aux < RTOL
    assert err_plain > 1e-9


def test_writes_aux_refuses_python_aux_bc():
    import pyclaw_amd as pyclaw
    claw = psystem_claw(pyclaw, "reference")
    claw.solver.aux_bc_lower[0] = pyclaw.BC.custom
    claw.solver.user_aux_bc_lower = lambda state, dim, t, auxbc, mbc: None
    with pytest.raises(NotImplementedError, match="user_aux_bc"):
        claw.solver.setup(claw.solution)
    claw.solver.teardown()


# ---- 12: two ranks on one GPU ---------------------------------------------------------------------------------------------
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
                    "PCL_PROC_GRID": "%dx1" % nranks, "TORCHELASTIC_RUN_ID": "cf%d" % port})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "cellfn_mp_worker.py"), case, ref_file],
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


@pytest.mark.parametrize("linearity", [1, 2])
def test_two_ranks_psystem_strain_hook(tmp_path, linearity):
    """Two blocks against one, device against device, so bit for bit under either law.  Global c.i / c.x do not enter
    here; the aux halo exchange behind the hook does: under the exponential law (2) q depends on the strain copy in the
    ghost columns next to the neighbour block, under the linear law (1) only aux shows it."""
    import pyclaw_amd as pyclaw
    claw = psystem_claw(pyclaw, "periodic", linearity=linearity)
    q, aux, auxbc = psystem_run(claw)
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, q=q, aux=aux, auxbc=auxbc, dt=claw.solver.dt_initial, linearity=linearity)
    launch("psystem", ref)


def test_two_ranks_index_stamp(tmp_path):
    import pyclaw_amd as pyclaw
    up, back = stamp_run(pyclaw, problems.acoustics2D(pyclaw, mx=65, my=3, run=False))
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, q=back[:, 2:-2, 2:-2])
    launch("stamp", ref)
