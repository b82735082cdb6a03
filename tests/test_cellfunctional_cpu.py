"""
CPU: functionals (pyclaw.CellFunctional; pcl_cellfn_compile_reduce and pcl_cellfn_reduce in include/pyclaw_amd.h) as far
as they go without a device -- the run-time compile for every dimension, reach and operation, the constructor's
refusals, the compiler's diagnostics, the cache key, and the refusals of the launch that come before any device call.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib, parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ('sum', 'abs_sum', 'max', 'min')
NEIGHBOUR = {1: "qn(0, 1)", 2: "qn(0, 1, 0) + qn(1, 0, -1)", 3: "qn(0, 1, 0, 0) + qn(1, 0, 0, -1) + auxn(0, 0, 1, 0)"}


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("reach", [0, 1])
@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_compiles_without_a_device(ndim, reach, op):
    body = "f[0] = q[0] * c.d[0] + aux[0] + p[1] + c.t + c.x[NDIM - 1] + c.i[0];"
    if reach:
        body += " f[0] += %s;" % NEIGHBOUR[ndim]
    assert pyclaw.CellFunctional(body, 1, reduce=op, reach=reach).compile(2, 1, ndim).code_size > 0


def test_eight_outputs_with_mixed_operations_compile():
    body = "for (int m = 0; m < NOUT; m++) f[m] = q[m % MEQN] + m;"
    F = pyclaw.CellFunctional(body, 8, reduce=OPS + OPS)
    assert F.compile(3, 0, 2, math='fast').code_size > 0 and F.reduce == OPS + OPS


def test_constructor_refusals_name_the_value():
    with pytest.raises(ValueError, match=r"nout must be an integer 1\.\.8, got 0"):
        pyclaw.CellFunctional("f[0] = 1.0;", 0)
    with pytest.raises(ValueError, match=r"nout must be an integer 1\.\.8, got 9"):
        pyclaw.CellFunctional("f[0] = 1.0;", 9)
    with pytest.raises(ValueError, match=r"reduce must be 'sum', 'abs_sum', 'max' or 'min', got 'mean'"):
        pyclaw.CellFunctional("f[0] = 1.0;", 1, reduce='mean')
    with pytest.raises(ValueError, match=r"got 'prod'"):
        pyclaw.CellFunctional("f[0] = 1.0;", 2, reduce=('sum', 'prod'))
    with pytest.raises(ValueError, match=r"reduce names 2 operations, but nout=3"):
        pyclaw.CellFunctional("f[0] = 1.0;", 3, reduce=('sum', 'max'))
    with pytest.raises(ValueError, match=r"at most 16 parameters, got 17"):
        pyclaw.CellFunctional("f[0] = 1.0;", 1, params=[0.0] * 17)
    with pytest.raises(ValueError, match=r"reach must be <= 8.*got 9"):
        pyclaw.CellFunctional("f[0] = 1.0;", 1, reach=9)
    F = pyclaw.CellFunctional("f[0] = 1.0;", 2, params=range(16), reach=8)
    assert F.reduce == ('sum', 'sum') and len(F.params) == 16
    with pytest.raises(ValueError, match="at most 16 parameters"):
        F.params = [0.0] * 17


def test_the_c_entry_refuses_what_the_constructor_refuses():
    L = _lib.lib()
    fn = C.c_void_p()
    ops = np.array([0, 7], dtype=np.int32)
    for nout in (0, 9):
        rc = L.pcl_cellfn_compile_reduce(b"f[0] = 1.0;", b"", 1, 0, 1, 0, 0, nout, _lib.i(ops), C.byref(fn), None)
        assert rc == _lib.EINVAL and b"nout must be 1..8, got %d" % nout in L.pcl_last_error() and not fn.value
    rc = L.pcl_cellfn_compile_reduce(b"f[0] = 1.0;", b"", 1, 0, 1, 0, 0, 2, _lib.i(ops), C.byref(fn), None)
    assert rc == _lib.EINVAL and b"ops[1] = 7" in L.pcl_last_error() and not fn.value
    rc = L.pcl_cellfn_compile_reduce(b"f[0] = 1.0;", b"", 1, 0, 1, 0, 9, 1, _lib.i(ops), C.byref(fn), None)
    assert rc == _lib.EINVAL and b"reach must be 0..8" in L.pcl_last_error() and not fn.value


def test_the_kind_is_not_one_of_the_public_compile():
    """functionals are reachable through pcl_cellfn_compile_reduce alone"""
    L = _lib.lib()
    fn = C.c_void_p()
    for kind in (0, pyclaw.CellFunctional.kind, 6):
        assert L.pcl_cellfn_compile(kind, b"f[0] = 1.0;", b"", 1, 0, 1, 0, 0, C.byref(fn), None) == _lib.EINVAL
        assert L.pcl_cellfn_compile_reach(kind, b"f[0] = 1.0;", b"", 1, 0, 1, 0, 0, 0, C.byref(fn), None) == _lib.EINVAL
        assert not fn.value


def test_a_body_that_assigns_q_or_aux_fails_with_the_compilers_log():
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellFunctional("f[0] = q[0];\nq[0] = 1.0;\n", 1).compile(2, 0, 2)
    assert "functional:2" in str(e.value) and "const" in str(e.value)
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellFunctional("aux[0] = 1.0;", 1).compile(2, 1, 2)
    assert "functional:1" in str(e.value) and "const" in str(e.value)
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellFunctional("f[0] = q[0];\nf[1] = no_such_name;\n", 2).compile(2, 0, 1)
    assert "no_such_name" in str(e.value) and "functional:2" in str(e.value)


def test_qn_in_a_body_without_reach_says_so():
    with pytest.raises(_lib.PclError, match="reach"):
        pyclaw.CellFunctional("f[0] = qn(0, 1);", 1).compile(1, 0, 1)
    with pytest.raises(_lib.PclError, match="reach"):
        pyclaw.CellFunctional("f[0] = auxn(0, 0, 1);", 1, reach=0).compile(1, 1, 2)


def test_operations_and_nout_are_part_of_the_cache_key():
    body = "f[0] = q[0];     // functional cache test\n"
    n0, h0 = stats()
    a = pyclaw.CellFunctional(body, 1, reduce='sum').compile(2, 0, 2)
    assert stats() == (n0 + 1, h0)
    b = pyclaw.CellFunctional(body, 1, reduce='max').compile(2, 0, 2)
    assert stats() == (n0 + 2, h0) and b._fn.value != a._fn.value
    c = pyclaw.CellFunctional(body, 2, reduce='sum').compile(2, 0, 2)
    assert stats() == (n0 + 3, h0) and c._fn.value not in (a._fn.value, b._fn.value)
    d = pyclaw.CellFunctional(body, 2, reduce=('sum', 'min')).compile(2, 0, 2)
    assert stats() == (n0 + 4, h0)
    e = pyclaw.CellFunctional(body, 1, reduce='sum', reach=1).compile(2, 0, 2)
    assert stats() == (n0 + 5, h0) and e._fn.value != a._fn.value
    again = pyclaw.CellFunctional(body, 1, reduce=['sum']).compile(2, 0, 2)
    assert stats() == (n0 + 5, h0 + 1) and again._fn.value == a._fn.value
    # the same object compiled again for the same constants asks nobody
    assert a.compile(2, 0, 2) is a and stats() == (n0 + 5, h0 + 1)
    # the text of a source term with the same body is another kind, another entry
    pyclaw.CellFunctional(body, 1, params=[1.0, 2.0]).compile(2, 0, 2)
    assert stats() == (n0 + 5, h0 + 2)          # params are no part of the compile
    assert d.code_size > 0


def test_refusals_before_any_device_call():
    """No solver handle exists here: each of these returns from the host-only checks in front of the launch."""
    L = _lib.lib()
    out = np.zeros(8)
    red = pyclaw.CellFunctional("f[0] = q[0];", 1).compile(3, 0, 2)
    src = pyclaw.CellSource("q[0] = 0.0;").compile(3, 0, 2)
    bc = pyclaw.CellBC("q[0] = qin(0, 0);").compile(3, 0, 2)
    # the other launches refuse a functional
    assert L.pcl_cellfn_apply(None, red._fn, 0.0, 0.0, None, 0) == _lib.EINVAL
    assert b"a functional runs through pcl_cellfn_reduce" in L.pcl_last_error()
    assert L.pcl_cellbc_apply(None, red._fn, 0, 0, 0.0, None, 0) == _lib.EINVAL
    assert b"the handle is a functional cell function, not a boundary condition" in L.pcl_last_error()
    # the functional's launch refuses the other kinds
    for other, name in ((src, b"step_src"), (bc, b"bc")):
        assert L.pcl_cellfn_reduce(None, other._fn, 0.0, None, 0, _lib.d(out)) == _lib.EINVAL
        assert b"the handle is a " + name + b" cell function, not a functional" in L.pcl_last_error()
    assert L.pcl_cellfn_reduce(None, None, 0.0, None, 0, _lib.d(out)) == _lib.EINVAL
    assert L.pcl_cellfn_reduce(None, red._fn, 0.0, None, 17, _lib.d(out)) == _lib.EINVAL
    assert b"at most 16 parameters" in L.pcl_last_error()
    # a good handle, but no solver
    assert L.pcl_cellfn_reduce(None, red._fn, 0.0, None, 0, _lib.d(out)) == _lib.EINVAL
    assert b"null argument" in L.pcl_last_error()
    # a handle compiled for another meqn: the check pcl_cellfn_reduce makes against the solver's constants
    assert L.pcl_cellfn_check(red._fn, 3, 0, 2) == 0
    assert L.pcl_cellfn_check(red._fn, 4, 0, 2) == _lib.EINVAL
    msg = L.pcl_last_error().decode()
    assert "compiled for meqn=3" in msg and "solver has meqn=4" in msg
    assert not out.any()


def test_reach_beyond_mbc_is_refused_on_the_host():
    """mbc = 2 for the classic solvers: evaluate() refuses reach = 3 before it looks for a device handle"""
    solver = pyclaw.ClawSolver1D()
    solver.rp = pyclaw.riemann.rp_advection_1d
    solver.mwaves = 1
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, 20)), 1)
    F = pyclaw.CellFunctional("f[0] = qn(0, 3);", 1, reach=3)
    with pytest.raises(ValueError, match=r"CellFunctional: reach=3, but the solver has mbc=2"):
        F.evaluate(solver, state)
    assert solver._h is None
    # within mbc the next thing asked for is the handle
    with pytest.raises(Exception, match="setup"):
        pyclaw.CellFunctional("f[0] = qn(0, 2);", 1, reach=2).evaluate(solver, state)


def test_a_functional_cannot_be_launched_as_a_cell_function():
    with pytest.raises(NotImplementedError, match="evaluate"):
        pyclaw.CellFunctional("f[0] = 1.0;", 1).launch(None, 0.0, 0.0)


def test_host_combination_of_the_ranks_without_a_group():
    assert parallel.allreduce_minmax_host([1.0, -2.0], [True, False]) == [1.0, -2.0]


def body_of(src, head):
    b = src[src.index(head):]
    return re.sub(r"//[^\n]*", "", b[:b.index("\n}\n")])


def test_the_reduce_entry_point_is_a_read_only_call():
    """pcl_cellfn_reduce stands with the read-only calls of the quiet tiles and of pcl_step_ahead (a step enqueued ahead
    is still adopted behind it): its body names none of the host state those rules guard, reads the selected register,
    and the header lists it."""
    src = open(os.path.join(ROOT, "pyclaw_amd", "csrc", "pclaw.hip")).read()
    b = body_of(src, "int pcl_cellfn_reduce(pcl_solver *")
    assert not re.search(r"\b(qt|plan|ahead|form|glog|halo)\s*\.", b), "host state of the step rules"
    assert not re.search(r"undo_slot|cf_snap|hipMemcpyDeviceToDevice|upload\(", b)
    assert b.count("cur(s)") == 2 and "a.dq = s->cf_part;" in b
    # host-only refusals come in front of the first HIP call
    first_hip = re.search(r"\bhip[A-Z]\w*\(", b).start()
    for msg in ("not a functional", "cellfn_check_locked", "cells away (reach)"):
        assert b.index(msg) < first_hip, msg
    hdr = open(os.path.join(ROOT, "include", "pyclaw_amd.h")).read()
    contract = hdr[hdr.index("step ahead: the next step is enqueued"):]
    assert "pcl_cellfn_reduce" in contract[:contract.index("int pcl_step_ahead(")]
    # the wrapper's text: q and aux are const, and the partial buffer is the only array a lane stores into
    text = open(os.path.join(ROOT, "pyclaw_amd", "csrc", "cellfn.hpp")).read()
    tail = text[text.index("kCellfnReduceTail"):]
    tail = tail[:tail.index(')PCLSRC"')]
    stores = re.findall(r"\ba\.(\w+)\[[^\]]*\]\s*=[^=]", tail)
    assert stores == ["dq"], stores
    assert "atomic" not in tail.lower()
