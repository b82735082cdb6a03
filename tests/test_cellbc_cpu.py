"""
CPU: custom boundary conditions as cell functions (pyclaw.CellBC, PCL_CELLFN_BC and pcl_cellbc_apply in
include/pyclaw_amd.h) as far as they go without a device -- the run-time compile of the boundary-condition wrapper for
the library's architecture, what its body sees, its diagnostics, the per-process cache, and the argument checks that
refuse a launch before anything is launched.
"""
import ctypes as C

import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib

# every name of the body's surface: the inward reads, the layer, the side, indices, coordinates, time and parameters
BODY = ("for (int m = 0; m < MEQN; m++) q[m] = (1.0 + c.g) * (2.0 * qin(m, 0) - qin(m, 1));\n"
        "q[0] = q[0] + auxin(0, c.g) * aux[0] + c.side + c.idim + c.i[0] + c.x[NDIM - 1] * c.d[0] + c.t * p[0];\n")


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


@pytest.mark.parametrize("ndim", [1, 2, 3])
def test_bc_body_compiles_without_a_device(ndim):
    bc = pyclaw.CellBC(BODY, params=[0.5]).compile(ndim + 1, 1, ndim)
    assert bc.code_size > 0
    assert isinstance(bc, pyclaw.DeviceBC) and isinstance(bc, pyclaw.CellFunction)


def test_bc_body_without_aux_and_with_a_preamble():
    pre = "__device__ inline double twice(double v) { return 2.0 * v; }\n"
    assert pyclaw.CellBC("q[0] = twice(qin(0, 0)) - qin(0, 1) + auxin(0, 0);", preamble=pre).compile(1, 0, 1).code_size > 0


def test_compile_error_names_identifier_and_body_line():
    bad = "q[0] = qin(0, 0);\nq[1] = q[1] + no_such_name;\n"
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellBC(bad).compile(3, 0, 2)
    assert "no_such_name" in str(e.value) and "bc:2" in str(e.value)
    # aux is const, and the interior-only names of the other kinds are not part of this surface
    with pytest.raises(_lib.PclError, match="bc:1"):
        pyclaw.CellBC("aux[0] = 1.0;").compile(3, 1, 2)
    with pytest.raises(_lib.PclError, match="bc:1"):
        pyclaw.CellBC("q[0] = c.dt;").compile(3, 1, 2)


def test_same_text_is_compiled_once_and_math_mode_is_part_of_the_key():
    """idim and side are run-time fields of the launch: the key is the text, the shape constants and the math mode, and
    one code object serves every side."""
    body = BODY + "// cache test\n"
    n0, h0 = stats()
    a = pyclaw.CellBC(body).compile(5, 1, 2)
    b = pyclaw.CellBC(body, dims=[0]).compile(5, 1, 2)
    assert stats() == (n0 + 1, h0 + 1)
    assert a._fn.value == b._fn.value
    c = pyclaw.CellBC(body).compile(5, 1, 2, math='fast')
    assert stats() == (n0 + 2, h0 + 1)
    assert c._fn.value != a._fn.value
    d = pyclaw.CellBC(body).compile(5, 1, 3)
    assert stats() == (n0 + 3, h0 + 1) and d._fn.value != a._fn.value
    # the kind is part of the key too: the same text as a start_step is another function (and does not compile: no qin)
    with pytest.raises(_lib.PclError, match="start_step:1"):
        pyclaw.CellStartStep(body).compile(5, 1, 2)


def test_more_than_16_params_are_refused():
    with pytest.raises(ValueError, match="at most 16 parameters"):
        pyclaw.CellBC(BODY, params=range(17))
    bc = pyclaw.CellBC(BODY, params=range(16))
    with pytest.raises(ValueError, match="at most 16 parameters"):
        bc.params = [0.0] * 17
    # and by the library itself, in front of every other check of the launch
    rc = _lib.lib().pcl_cellbc_apply(None, None, 0, 0, 0.0, None, 17)
    assert rc == _lib.EINVAL and b"at most 16 parameters" in _lib.lib().pcl_last_error()


def test_handle_for_another_meqn_is_refused():
    bc = pyclaw.CellBC(BODY).compile(5, 1, 2)
    L = _lib.lib()
    assert L.pcl_cellfn_check(bc._fn, 5, 1, 2) == 0
    assert L.pcl_cellfn_check(bc._fn, 4, 1, 2) == _lib.EINVAL
    msg = L.pcl_last_error().decode()
    assert "compiled for meqn=5" in msg and "solver has meqn=4" in msg
    assert L.pcl_cellfn_check(bc._fn, 5, 1, 3) == _lib.EINVAL


def test_apply_refuses_bad_side_and_other_kinds_before_any_device_call():
    """No solver handle exists here: every one of these returns from the host-only checks in front of the launch."""
    L = _lib.lib()
    bc = pyclaw.CellBC(BODY).compile(5, 1, 2)
    for idim, side in ((-1, 0), (3, 0), (0, -1), (0, 2)):
        assert L.pcl_cellbc_apply(None, bc._fn, idim, side, 0.0, None, 0) == _lib.EINVAL
        assert b"bad idim/side" in L.pcl_last_error()
    src = pyclaw.CellSource("q[0] = 0.0;").compile(5, 1, 2)
    assert L.pcl_cellbc_apply(None, src._fn, 0, 0, 0.0, None, 0) == _lib.EINVAL
    assert b"step_src cell function, not a boundary condition" in L.pcl_last_error()
    assert L.pcl_cellbc_apply(None, None, 0, 0, 0.0, None, 0) == _lib.EINVAL
    # a good handle and a good side, but no solver
    assert L.pcl_cellbc_apply(None, bc._fn, 1, 1, 0.0, None, 0) == _lib.EINVAL
    assert b"null argument" in L.pcl_last_error()
    # the compile refuses what the kind cannot have
    fn = C.c_void_p()
    assert L.pcl_cellfn_compile(4, b"q[0] = 1.0;", b"", 3, 1, 2, 0, 1, C.byref(fn), None) == _lib.EINVAL      # writes_aux
    assert L.pcl_cellfn_compile(5, b"q[0] = 1.0;", b"", 3, 1, 2, 0, 0, C.byref(fn), None) == _lib.EINVAL      # no such kind
