"""
GPU: functionals (pyclaw.CellFunctional, pcl_cellfn_reduce) -- per-cell integrands reduced over the
interior cells of the resident state.

Exact cases use integer-valued doubles: every partial sum is an integer below 2^53, so any order of summation gives the
same bits, and the device must equal numpy bitwise.  Cases on other data use the forward error bound of recursive
summation in any order, |s - fsum| <= N * 2^-53 * sum|f_i| with N the number of interior cells: no measured tolerance.

The wrapper's workgroup is 256 lanes (four wavefronts of 64) along x, one row per workgroup row; the second pass is ONE
workgroup of SECOND_PASS_THREADS = 256 threads per output, thread t folding partials t, t + 256, ... (in eight chains,
so a second round of a chain begins at 2048 partials: the 4096^2 benchmark has 65536).  The shapes are
the smallest that reach every path: a single lane, a partial wavefront, a partial workgroup, two workgroups in a row
(300 = 256 + 44), and 300 x 260 -> 2 * 260 = 520 partials per output, more than the second pass has threads.
"""
import ctypes
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECOND_PASS_THREADS = 256
U = 2.0 ** -53

# (% MEQN: the same text serves the one-component advection state and the systems)
FOUR = "f[0] = q[0]; f[1] = q[1 % MEQN] * q[2 % MEQN]; f[2] = q[0]; f[3] = q[1 % MEQN];"
FOUR_OPS = ('sum', 'abs_sum', 'max', 'min')
TV_2D = "f[0] = fabs(qn(0, 1, 0) - qn(0, 0, 0)) + fabs(qn(0, 0, 1) - qn(0, 0, 0));"


def four_terms(q):
    """the integrands of FOUR on the interior array q[m, ...]"""
    n = q.shape[0]
    return [q[0], np.abs(q[1 % n] * q[2 % n]), q[0], q[1 % n]]


def four_numpy(q):
    t = four_terms(q)
    return np.array([np.sum(t[0]), np.sum(t[1]), np.max(t[2]), np.min(t[3])])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def within_bound(got, terms):
    """the order-free bound of the sums; prints each figure before it asserts"""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    want, scale = math.fsum(terms), math.fsum(np.abs(terms))
    bound = terms.size * U * scale
    print("sum: device %r fsum %r |diff| %.3g bound %.3g (N = %d)" % (float(got), want, abs(got - want), bound, terms.size))
    assert abs(got - want) <= bound, (float(got), want, bound)


def check_four(got, q):
    """sums within the bound, extremes bitwise"""
    t = four_terms(q)
    within_bound(got[0], t[0])
    within_bound(got[1], t[1])
    assert bits(got[2:]).tolist() == bits([np.max(t[2]), np.min(t[3])]).tolist(), (got, np.max(t[2]), np.min(t[3]))


def make(shape, periodic=False):
    """a classic solver and solution of that interior shape, not set up: acoustics in 1-D (meqn 2), 2-D (3), 3-D (4)"""
    if len(shape) == 1:
        claw = problems.acoustics1D(pyclaw, mx=shape[0], run=False)[1]
        claw.solver.bc_lower[0] = claw.solver.bc_upper[0] = pyclaw.BC.outflow      # (a ghost fill that one cell can serve)
    elif len(shape) == 2:
        claw = problems.acoustics2D(pyclaw, mx=shape[0], my=shape[1], run=False)
    else:
        claw = problems.acoustics3D(pyclaw, test='hom', mx=shape[0], my=shape[1], mz=shape[2], run=False)
    if periodic:
        for k in range(len(shape)):
            claw.solver.bc_lower[k] = claw.solver.bc_upper[k] = pyclaw.BC.periodic
    assert tuple(claw.solution.state.q.shape[1:]) == tuple(shape)
    return claw.solver, claw.solution


def resident(solver, solution, q):
    """set up, put q on the device, fill its ghost cells (non-zero: a reduction that took them in would show)"""
    solution.state.q[...] = q
    solver.setup(solution)
    solver.begin_resident(solution)
    solver.apply_q_bcs(solution.state)


def integers(shape, meqn, seed=11):
    return np.random.default_rng(seed).integers(-1000, 1000, size=(meqn,) + tuple(shape)).astype(np.float64)


@pytest.fixture(scope="module")
def random_300x260():
    """the random state of tests 2 and 5, made once and left unchanged"""
    q = np.random.default_rng(5).standard_normal((3, 300, 260)) * np.array([1.0, 1e3, 1e-3])[:, None, None]
    q.setflags(write=False)
    return q


# ---- 1: exact values ---------------------------------------------------------------------------------------------------
# (5 x 2100: 2100 partials, so that every chain of the second pass goes round twice)
SHAPES = [(1,), (5,), (300,), (37, 21), (300, 260), (5, 2100), (9, 7, 6), (70, 5, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_exact_values_on_integer_data(shape):
    solver, solution = make(shape)
    if shape == (300, 260):
        partials = ((shape[0] + 255) // 256) * shape[1]
        assert partials == 520 > SECOND_PASS_THREADS
    q = integers(shape, solution.state.meqn)
    resident(solver, solution, q)
    ghosted = np.empty(solver.qbc.shape, order='F')
    _lib.check(_lib.lib().pcl_get_q(solver._h, _lib.d(ghosted), 1))
    got = pyclaw.CellFunctional(FOUR, 4, reduce=FOUR_OPS).evaluate(solver, solution.state)
    solver.end_resident(solution)
    solver.teardown()
    want = four_numpy(q)
    print(shape, got, want)
    assert got.dtype == np.float64 and got.shape == (4,)
    assert bits(got).tolist() == bits(want).tolist()
    # the ghost cells held something: the same reduction over the ghosted array gives other numbers
    assert np.abs(ghosted).sum() > np.abs(q).sum()
    assert four_numpy(ghosted)[0] != want[0] or four_numpy(ghosted)[1] != want[1]


# ---- 2, 5: random doubles, repeatability ---------------------------------------------------------------------------------
def test_random_doubles_and_repeatability(random_300x260):
    q = random_300x260
    solver, solution = make((300, 260))
    resident(solver, solution, q)
    F = pyclaw.CellFunctional(FOUR, 4, reduce=FOUR_OPS)
    first = F.evaluate(solver, solution.state)
    second = F.evaluate(solver, solution.state)
    # the same through the non-resident path: the host copy is uploaded first
    solver.end_resident(solution)
    third = F.evaluate(solver, solution.state)
    solver.teardown()
    check_four(first, q)
    assert bits(first).tolist() == bits(second).tolist() == bits(third).tolist()
    assert np.array_equal(solution.state.q, q)


def test_nan_is_passed_over_by_max_and_min_and_kept_by_the_sums():
    solver, solution = make((37, 21))
    q = integers((37, 21), 3)
    q[0, 5, 7] = np.nan
    q[1, 30, 2] = np.nan
    resident(solver, solution, q)
    got = pyclaw.CellFunctional(FOUR, 4, reduce=FOUR_OPS).evaluate(solver, solution.state)
    solver.end_resident(solution)
    solver.teardown()
    assert np.isnan(got[0]) and np.isnan(got[1])
    assert got[2] == np.nanmax(q[0]) and got[3] == np.nanmin(q[1])


# ---- 3: what the body sees -------------------------------------------------------------------------------------------------
def test_what_the_body_sees():
    claw = problems.vc_acoustics2D(pyclaw, mx=37, my=21, run=False)
    solver, solution = claw.solver, claw.solution
    st = solution.state
    rng = np.random.default_rng(3)
    st.aux[...] = rng.integers(1, 50, size=st.aux.shape).astype(np.float64)
    aux = st.aux.copy()
    q = integers((37, 21), st.meqn, seed=4)
    st.t = 0.375
    resident(solver, solution, q)
    body = ("f[0] = c.i[1]; f[1] = c.i[0]; f[2] = c.x[0] * c.d[0] * c.d[1]; f[3] = aux[1] * q[0]; f[4] = p[0] * q[2];\n"
            "f[5] = c.t; f[6] = c.dt; f[7] = c.x[1];")
    F = pyclaw.CellFunctional(body, 8, reduce=('sum', 'sum', 'sum', 'sum', 'sum', 'max', 'max', 'min'), params=[3.0])
    n0 = stats()
    a = F.evaluate(solver, st)
    n1 = stats()
    F.params = [-2.0]
    b = F.evaluate(solver, st)
    assert stats() == n1 and n1[0] == n0[0] + 1          # one compile, none for the new parameter
    solver.end_resident(solution)
    solver.teardown()
    I, J = np.meshgrid(np.arange(37), np.arange(21), indexing='ij')
    X, Y = st.grid.c_center
    dx, dy = st.grid.d
    assert a[0] == float(J.sum()) and a[1] == float(I.sum())
    within_bound(a[2], X * dx * dy)
    assert a[3] == float((aux[1] * q[0]).sum())
    assert a[4] == float((3.0 * q[2]).sum()) and b[4] == float((-2.0 * q[2]).sum()) and a[4] != b[4]
    assert a[5] == 0.375 and a[6] == 0.0
    assert abs(a[7] - Y.min()) <= 2 * U * abs(Y.min())
    assert bits(a[:4]).tolist() == bits(b[:4]).tolist()


def stats():
    n, h = ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(ctypes.byref(n), ctypes.byref(h)))
    return n.value, h.value


# ---- 4: neighbour reads ----------------------------------------------------------------------------------------------------
def tv_numpy(q0):
    return float(np.sum(np.abs(np.roll(q0, -1, 0) - q0) + np.abs(np.roll(q0, -1, 1) - q0)))


def test_neighbour_reads_classic():
    """periodic in both directions: the differences at the upper edges read ghost cells, which evaluate() fills first --
    the state is uploaded without them here"""
    solver, solution = make((37, 21), periodic=True)
    q = integers((37, 21), 3, seed=8)
    solution.state.q[...] = q
    solver.setup(solution)
    got = pyclaw.CellFunctional(TV_2D, 1, reach=1).evaluate(solver, solution.state)
    with pytest.raises(ValueError, match=r"reach=3, but the solver has mbc=2"):
        pyclaw.CellFunctional("f[0] = qn(0, 3, 0);", 1, reach=3).evaluate(solver, solution.state)
    # a handle compiled for another meqn is refused by the library's own check, in front of the launch
    other = pyclaw.CellFunctional("f[0] = q[0];", 1).compile(2, 0, 2)
    out = np.zeros(1)
    assert _lib.lib().pcl_cellfn_reduce(solver._h, other._fn, 0.0, None, 0, _lib.d(out)) == _lib.EINVAL
    assert b"compiled for meqn=2" in _lib.lib().pcl_last_error()
    solver.teardown()
    assert got[0] == tv_numpy(q[0]) and got[0] > 0


def sharp_run(with_calls, qint):
    claw = problems.acoustics2D(pyclaw, mx=37, my=21, solver_type='sharpclaw', time_integrator='SSP33', run=False)
    solver, solution = claw.solver, claw.solution
    for k in range(2):
        solver.bc_lower[k] = solver.bc_upper[k] = pyclaw.BC.periodic
    solver.setup(solution)
    assert solver.mbc == 3
    solver.dt = solver.dt_initial
    solver.evolve_to_time(solution)
    solution.state.q[...] = qint            # (the host copy is the state between two evolve_to_time calls)
    got = None
    if with_calls:
        got = pyclaw.CellFunctional(TV_2D, 1, reach=1).evaluate(solver, solution.state)
    solver.evolve_to_time(solution)
    solver.teardown()
    return got, solution.state.q.copy()


def test_neighbour_reads_sharpclaw_between_two_steps():
    q = integers((37, 21), 3, seed=9)
    got, with_calls = sharp_run(True, q)
    _, without = sharp_run(False, q)
    assert got[0] == tv_numpy(q[0]) and got[0] > 0
    assert np.isfinite(with_calls).all() and np.array_equal(bits(with_calls), bits(without))


# ---- 6: no side effects, classic run ---------------------------------------------------------------------------------------
def classic_run(dim_split, with_calls):
    claw = problems.acoustics2D(pyclaw, mx=37, my=21, dim_split=dim_split, run=False)
    solver, solution = claw.solver, claw.solution
    solver.setup(solution)
    solver.dt = solver.dt_initial
    F = pyclaw.CellFunctional(FOUR, 4, reduce=FOUR_OPS)
    seen = []
    for _ in range(10):
        solver.evolve_to_time(solution)
        if with_calls:
            seen.append((F.evaluate(solver, solution.state), solution.state.q.copy()))
    solver.teardown()
    return solution.state.q.copy(), seen


@pytest.mark.parametrize("dim_split", [1, 0], ids=["split", "unsplit"])
def test_no_side_effects_classic(dim_split):
    q_calls, seen = classic_run(dim_split, True)
    q_plain, _ = classic_run(dim_split, False)
    assert np.isfinite(q_plain).all() and np.array_equal(bits(q_calls), bits(q_plain))
    assert len(seen) == 10
    for got, q in seen:
        check_four(got, q)


# ---- 7: no side effects, resident run with step ahead ----------------------------------------------------------------------
MASS_ENERGY = "f[0] = q[0] * c.d[0] * c.d[1]; f[1] = q[3] * c.d[0] * c.d[1]; f[2] = q[0];"


def resident_run(with_calls, nsteps=40):
    claw = problems.shockbubble(pyclaw, mx=160, my=40, tfinal=1.0, device_callbacks=True, run=False)
    solver, solution = claw.solver, claw.solution
    assert solver.dt_variable
    solver.setup(solution)
    solver.dt = solver.dt_initial
    solver.begin_resident(solution)
    F = pyclaw.CellFunctional(MASS_ENERGY, 3, reduce=('sum', 'sum', 'max'))
    seen = []
    for _ in range(nsteps):
        solver.evolve_to_time(solution)
        if with_calls:
            got = F.evaluate(solver, solution.state)
            solver._pull(solution.state)            # pcl_get_q: the accepted state, and a read-only call as well
            seen.append((got, solution.state.q.copy()))
    a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.lib().pcl_step_ahead_stats(solver._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    armed = solver._step_ahead_sent
    solver.end_resident(solution)
    solver.teardown()
    return solution.state.q.copy(), float(solution.t), seen, (a.value, b.value, c.value), armed


def test_no_side_effects_resident_with_step_ahead():
    q_calls, t_calls, seen, ahead, armed = resident_run(True)
    q_plain, t_plain, _, ahead_plain, _ = resident_run(False)
    print("step ahead (enqueued, adopted, dropped): with calls %s, without %s" % (ahead, ahead_plain))
    assert armed and armed[0] == 2
    # the test means something: steps were enqueued ahead and adopted with an evaluate() behind every step, and not
    # one more was dropped than in the run without the calls
    assert ahead[1] > 0 and ahead == ahead_plain, (ahead, ahead_plain)
    assert t_calls == t_plain and np.isfinite(q_plain).all() and np.array_equal(bits(q_calls), bits(q_plain))
    dx, dy = 2.0 / 160, 0.5 / 40
    assert len(seen) == 40
    for got, q in seen:
        within_bound(got[0], q[0] * dx * dy)
        within_bound(got[1], q[3] * dx * dy)
        assert got[2] == q[0].max()
    assert np.array_equal(bits(seen[-1][1]), bits(q_plain))
    assert not np.array_equal(seen[0][1], seen[1][1])


# ---- 8: Controller ---------------------------------------------------------------------------------------------------------
def controller_run(tmp_path, name, compute_F, mF=0):
    claw = problems.acoustics2D(pyclaw, mx=37, my=21, tfinal=0.06, nout=3, run=False)
    claw.output_format = None
    claw.keep_copy = False
    claw.outdir = str(tmp_path / name)
    claw.compute_F = compute_F
    if mF:
        claw.solution.state.mF = mF
    claw.run()
    assert claw.solution.state.mF == mF
    with open(os.path.join(claw.outdir, "F.txt")) as f:
        return [line.split() for line in f.read().splitlines()], claw


def test_controller_writes_the_functional(tmp_path):
    def compute_F(state):
        dx, dy = state.grid.d
        state.F[0] = state.q[0] * dx * dy
        state.F[1] = state.q[1] * state.q[2]

    dev, claw = controller_run(tmp_path, "device",
                               pyclaw.CellFunctional("f[0] = q[0] * c.d[0] * c.d[1]; f[1] = q[1] * q[2];", 2, reduce='abs_sum'))
    host, _ = controller_run(tmp_path, "host", compute_F, mF=2)
    assert len(dev) == len(host) == 3 + 1 and all(len(r) == 2 + 1 for r in dev + host)
    assert [r[0] for r in dev] == [r[0] for r in host]
    n = 37 * 21
    for d, h in zip(dev, host):
        for a, b in zip(d[1:], h[1:]):
            a, b = float(a), float(b)
            # both are sums of the same N non-negative terms in some order: each is within N u S of the exact sum S
            print("F: device %r host %r" % (a, b))
            assert abs(a - b) <= 2 * n * U * max(a, b) * (1 + 2 * n * U)
    assert float(dev[1][1]) > 0 and float(dev[-1][2]) > 0


# ---- 9: two ranks on one GPU -----------------------------------------------------------------------------------------------
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
                    "PCL_PROC_GRID": "%dx1" % nranks, "TORCHELASTIC_RUN_ID": "cfn%d" % port})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "cellfunctional_mp_worker.py"), case,
                                       ref_file], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
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
    for out in outs:
        assert "bit-identical: True" in out, out[-1500:]


def test_two_ranks_return_the_single_block_values(tmp_path):
    solver, solution = problems.advection2D(pyclaw, 40, 24)
    q = integers((40, 24), 1, seed=21)
    solution.state.q[...] = q
    solver.setup(solution)
    four = pyclaw.CellFunctional(FOUR, 4, reduce=FOUR_OPS).evaluate(solver, solution.state)
    tv = pyclaw.CellFunctional(TV_2D, 1, reach=1).evaluate(solver, solution.state)
    solver.teardown()
    assert bits(four).tolist() == bits(four_numpy(q)).tolist() and tv[0] == tv_numpy(q[0])
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, q=q, four=four, tv=tv)
    launch("integers", ref)
