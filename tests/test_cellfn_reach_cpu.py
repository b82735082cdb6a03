"""
CPU: neighbour reads of cell functions (``reach``: qn / auxn in the bodies of pyclaw.CellSource / CellDqSource /
CellStartStep, pcl_cellfn_compile_reach in include/pyclaw_amd.h) as far as they go without a device -- the run-time
compile of every kind, dimension and reach, its diagnostics, the cache key, and every refusal of the new argument, each
raised before any device call.
"""
import ctypes as C

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

STENCIL = {1: "qn(0, -1) + qn(0, 1)", 2: "qn(0, -1, 0) + qn(0, 0, 1)", 3: "qn(0, -1, 0, 0) + qn(0, 0, 1, 0) + qn(0, 0, 0, -1)"}


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


@pytest.mark.parametrize("reach", [1, 2])
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_the_three_kinds_compile_without_a_device(ndim, reach):
    s = STENCIL[ndim]
    assert pyclaw.CellSource("q[0] = 0.5 * (%s) + auxn(1, %d);" % (s, reach), reach=reach).compile(2, 2, ndim).code_size > 0
    assert pyclaw.CellDqSource("dq[1] = c.dt * (%s);" % s, reach=reach).compile(2, 0, ndim).code_size > 0
    assert pyclaw.CellStartStep("q[1] = %s;" % s, reach=reach).compile(2, 0, ndim).code_size > 0


def test_the_bodies_of_the_problems_module_compile():
    assert pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC, params=[0.01, 0], reach=1).compile(3, 0, 2).code_size > 0
    assert pyclaw.CellSource(problems.DIFFUSION_3D_CELL_SRC, params=[0.01, 0], reach=1).compile(4, 2, 3).code_size > 0
    assert pyclaw.CellSource(problems.AUX_GRADIENT_CELL_SRC, params=[1.0], reach=1).compile(3, 2, 2).code_size > 0
    for ndim in (1, 2):
        assert pyclaw.CellDqSource(problems.LAPLACIAN4_DQ_CELL_SRC, params=[0.01], reach=2).compile(2, 0, ndim).code_size > 0


def test_auxn_is_absent_without_aux():
    with pytest.raises(_lib.PclError, match="auxn"):
        pyclaw.CellSource("q[0] = auxn(0, 1);", reach=1).compile(1, 0, 1)


def test_compile_error_keeps_the_body_line():
    bad = "const double a = qn(0, 1);\nq[0] = a + no_such_name;\n"
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellSource(bad, reach=1).compile(1, 0, 1)
    assert "no_such_name" in str(e.value) and "step_src:2" in str(e.value)


def test_reach_is_part_of_the_cache_key_and_zero_is_the_plain_entry():
    body = "q[0] = q[0] * p[0];   // reach cache test\n"
    n0, h0 = stats()
    plain = pyclaw.CellSource(body).compile(2, 0, 2)
    zero = pyclaw.CellSource(body, reach=0).compile(2, 0, 2)
    assert stats() == (n0 + 1, h0 + 1)
    assert zero._fn.value == plain._fn.value and zero.code_size == plain.code_size
    one = pyclaw.CellSource(body, reach=1).compile(2, 0, 2)
    assert stats() == (n0 + 2, h0 + 1)
    assert one._fn.value != plain._fn.value
    two = pyclaw.CellSource(body, reach=2).compile(2, 0, 2)
    assert stats() == (n0 + 3, h0 + 1) and two._fn.value != one._fn.value
    # the C entries: pcl_cellfn_compile is the reach = 0 case of pcl_cellfn_compile_reach
    L = _lib.lib()
    a, b = C.c_void_p(), C.c_void_p()
    _lib.check(L.pcl_cellfn_compile(1, body.encode(), b"", 2, 0, 2, 0, 0, C.byref(a), None))
    _lib.check(L.pcl_cellfn_compile_reach(1, body.encode(), b"", 2, 0, 2, 0, 0, 0, C.byref(b), None))
    assert a.value == b.value == plain._fn.value and stats() == (n0 + 3, h0 + 3)
    L.pcl_cellfn_release(a)
    L.pcl_cellfn_release(b)


def test_qn_in_a_body_without_reach_says_so():
    for make in (lambda: pyclaw.CellSource("q[0] = qn(0, 1);"), lambda: pyclaw.CellStartStep("q[0] = qn(0, 0, 1);", reach=0),
                 lambda: pyclaw.CellDqSource("dq[0] = auxn(0, 1);")):
        with pytest.raises(_lib.PclError, match="reach"):
            make().compile(1, 1, 2)


def test_reach_outside_0_to_8_is_refused_at_construction():
    for cls in (pyclaw.CellSource, pyclaw.CellDqSource, pyclaw.CellStartStep):
        with pytest.raises(ValueError, match=r"reach must be >= 0.*got -1"):
            cls("q[0] = 0.0;", reach=-1)
        with pytest.raises(ValueError, match=r"reach must be <= 8, the largest mbc.*got 9"):
            cls("q[0] = 0.0;", reach=9)
        assert cls("(void)c;", reach=8).reach == 8
    with pytest.raises(ValueError, match="integer"):
        pyclaw.CellSource("q[0] = 0.0;", reach=1.5)


def test_writes_aux_with_reach_is_refused():
    with pytest.raises(ValueError, match="writes_aux=True together with reach=1.*second snapshot"):
        pyclaw.CellStartStep("aux[0] = qn(0, 1);", writes_aux=True, reach=1)
    fn = C.c_void_p()
    rc = _lib.lib().pcl_cellfn_compile_reach(3, b"aux[0] = q[0];", b"", 1, 1, 1, 0, 1, 1, C.byref(fn), None)
    assert rc == _lib.EINVAL and b"writes_aux with reach > 0" in _lib.lib().pcl_last_error()


def test_cell_bc_takes_no_reach():
    with pytest.raises(TypeError, match="reach"):
        pyclaw.CellBC("q[0] = qin(0, 0);", reach=1)
    fn = C.c_void_p()
    L = _lib.lib()
    rc = L.pcl_cellfn_compile_reach(4, b"q[0] = qin(0, 0);", b"", 1, 0, 1, 0, 0, 1, C.byref(fn), None)
    assert rc == _lib.EINVAL and b"takes no reach" in L.pcl_last_error() and not fn.value
    _lib.check(L.pcl_cellfn_compile_reach(4, b"q[0] = qin(0, 0);", b"", 1, 0, 1, 0, 0, 0, C.byref(fn), None))
    L.pcl_cellfn_release(fn)


def test_the_c_entry_refuses_a_reach_outside_0_to_8():
    fn = C.c_void_p()
    L = _lib.lib()
    for reach in (-1, 9, 1 << 20):
        rc = L.pcl_cellfn_compile_reach(1, b"q[0] = 0.0;", b"", 1, 0, 1, 0, 0, reach, C.byref(fn), None)
        assert rc == _lib.EINVAL and b"reach must be 0..8" in L.pcl_last_error() and not fn.value


def classic_1d(mx=20):
    solver = pyclaw.ClawSolver1D()
    solver.rp = pyclaw.riemann.rp_advection_1d
    solver.mwaves = 1
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx)), 1)
    state.aux_global['u'] = 1.
    state.q[0, :] = np.linspace(0.0, 1.0, mx)
    return solver, pyclaw.Solution(state)


def test_reach_beyond_mbc_is_refused_at_setup_classic():
    """mbc = 2 for the classic solvers (3-D included): reach = 3 is refused by setup() before the handle is created,
    so this machine, without a device, reaches the message"""
    for name, make in (("step_src", lambda: pyclaw.CellSource("q[0] = qn(0, 3);", reach=3)),
                       ("start_step", lambda: pyclaw.CellStartStep("q[0] = qn(0, 3);", reach=3))):
        solver, solution = classic_1d()
        setattr(solver, name, make())
        with pytest.raises(ValueError, match=r"reach=3, but the solver has mbc=2"):
            solver.setup(solution)
        assert solver._h is None
    claw = problems.acoustics3D(pyclaw, test='hom', mx=9, my=7, mz=5, run=False)
    claw.solver.step_src = pyclaw.CellSource(problems.DIFFUSION_3D_CELL_SRC, params=[0.01, 0], reach=3)
    with pytest.raises(ValueError, match=r"reach=3, but the solver has mbc=2"):
        claw.solver.setup(claw.solution)


def test_reach_beyond_mbc_is_refused_at_setup_sharpclaw():
    """SharpClaw's mbc is (weno_order + 1) // 2 = 3 by default"""
    for name, make in (("dq_src", lambda: pyclaw.CellDqSource("dq[0] = qn(0, 4, 0);", reach=4)),
                       ("start_step", lambda: pyclaw.CellStartStep("q[0] = qn(0, 4, 0);", reach=4))):
        claw = problems.acoustics2D(pyclaw, mx=12, my=10, solver_type='sharpclaw', run=False)
        setattr(claw.solver, name, make())
        with pytest.raises(ValueError, match=r"reach=4, but the solver has mbc=3"):
            claw.solver.setup(claw.solution)
        assert claw.solver._h is None


def test_reach_beyond_mbc_is_refused_where_the_function_was_assigned_after_setup():
    """the check of the first step(): apply() runs it in front of the ghost fill and the launch"""
    solver, solution = classic_1d()
    src = pyclaw.CellSource("q[0] = qn(0, 3);", reach=3)
    with pytest.raises(ValueError, match=r"reach=3, but the solver has mbc=2"):
        src.apply(solver, solution.state, 0.1)
    hook = pyclaw.CellStartStep("q[0] = qn(0, 3);", reach=3)
    with pytest.raises(ValueError, match=r"reach=3, but the solver has mbc=2"):
        hook.apply(solver, solution.state)
