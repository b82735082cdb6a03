"""
CPU: cell functions (pyclaw.CellSource / CellDqSource / CellStartStep, pcl_cellfn_* in include/pyclaw_amd.h) as far as
they go without a device -- the run-time compile for the library's architecture, its diagnostics with the body's own
line numbers, the per-process cache, and the argument checks that refuse a launch before anything is launched.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BODY = "q[0] = q[0] - c.dt * p[0] * aux[0] * q[4];\nq[3] = q[3] + c.x[1] * c.d[0] + c.t + c.i[0];\n"


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def test_step_src_compiles_without_a_device():
    src = pyclaw.CellSource(BODY, params=[0.5]).compile(5, 1, 2)
    assert src.code_size > 0


def test_compile_error_names_identifier_and_body_line():
    bad = "q[0] = q[0] - c.dt * p[0] * aux[0] * q[4];\nq[3] = q[3] + no_such_name;\n"
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellSource(bad).compile(5, 1, 2)
    assert "no_such_name" in str(e.value) and "step_src:2" in str(e.value)


def test_same_text_is_compiled_once_and_math_mode_is_part_of_the_key():
    body = BODY + "// cache test\n"
    n0, h0 = stats()
    a = pyclaw.CellSource(body).compile(5, 1, 2)
    b = pyclaw.CellSource(body).compile(5, 1, 2)
    assert stats() == (n0 + 1, h0 + 1)
    assert a._fn.value == b._fn.value
    c = pyclaw.CellSource(body).compile(5, 1, 2, math='fast')
    assert stats() == (n0 + 2, h0 + 1)
    assert c._fn.value != a._fn.value


def test_cache_outlives_the_objects_and_a_changed_text_recompiles():
    body = BODY + "// lifetime test\n"
    n0, h0 = stats()
    src = pyclaw.CellSource(body).compile(5, 1, 2)
    first = src._fn.value
    src.release()
    again = pyclaw.CellSource(body).compile(5, 1, 2)         # the text was released, not forgotten
    assert stats() == (n0 + 1, h0 + 1) and again._fn.value == first
    again.body = body + "q[1] = 0.0;\n"                      # reassigned after a compile: not the old kernel
    again.compile(5, 1, 2)
    assert stats() == (n0 + 2, h0 + 1) and again._fn.value != first
    # both references to the first text are gone (release(), and compile() of the changed text): one more is refused
    assert _lib.lib().pcl_cellfn_release(C.c_void_p(first)) == _lib.EINVAL


def test_more_than_16_params_are_refused():
    with pytest.raises(ValueError, match="at most 16 parameters"):
        pyclaw.CellSource(BODY, params=range(17))
    src = pyclaw.CellSource(BODY, params=range(16))
    with pytest.raises(ValueError, match="at most 16 parameters"):
        src.params = [0.0] * 17
    # and by the library itself, in front of every other check of the launch
    rc = _lib.lib().pcl_cellfn_apply(None, None, 0.0, 0.0, None, 17)
    assert rc == _lib.EINVAL and b"at most 16 parameters" in _lib.lib().pcl_last_error()


def test_writes_aux_without_aux_is_refused():
    hook = pyclaw.CellStartStep("q[0] = 1.0;", writes_aux=True)
    with pytest.raises(ValueError, match="maux == 0"):
        hook.compile(3, 0, 2)
    fn = C.c_void_p()
    rc = _lib.lib().pcl_cellfn_compile(3, b"q[0] = 1.0;", b"", 3, 0, 2, 0, 1, C.byref(fn), None)
    assert rc == _lib.EINVAL and b"maux == 0" in _lib.lib().pcl_last_error()
    # only a start_step may write aux
    rc = _lib.lib().pcl_cellfn_compile(1, b"q[0] = 1.0;", b"", 3, 1, 2, 0, 1, C.byref(fn), None)
    assert rc == _lib.EINVAL


def test_handle_for_another_meqn_is_refused():
    src = pyclaw.CellSource(BODY).compile(5, 1, 2)
    L = _lib.lib()
    assert L.pcl_cellfn_check(src._fn, 5, 1, 2) == 0
    assert L.pcl_cellfn_check(src._fn, 4, 1, 2) == _lib.EINVAL
    msg = L.pcl_last_error().decode()
    assert "compiled for meqn=5" in msg and "solver has meqn=4" in msg
    assert L.pcl_cellfn_check(None, 5, 1, 2) == _lib.EINVAL


def test_preamble_and_the_three_kinds_compile():
    pre = "__device__ inline double twice(double v) { return 2.0 * v; }\n"
    assert pyclaw.CellSource("q[0] = twice(q[0]);", preamble=pre).compile(1, 0, 1).code_size > 0
    assert pyclaw.CellDqSource("dq[0] = -c.dt * q[1];").compile(2, 0, 1).code_size > 0
    assert pyclaw.CellStartStep("aux[3] = q[0];", writes_aux=True).compile(3, 4, 2).code_size > 0
    with pytest.raises(_lib.PclError, match="dq_src:1"):          # q is const for a dq_src
        pyclaw.CellDqSource("q[0] = 0.0;").compile(2, 0, 1)
    with pytest.raises(_lib.PclError, match="start_step:1"):      # aux is const unless writes_aux
        pyclaw.CellStartStep("aux[3] = q[0];").compile(3, 4, 2)


def test_library_works_where_hiprtc_cannot_be_opened(tmp_path):
    """The loader's override pointed at a file that does not exist: the library loads, every host-only call works, and
    only the compile fails, with a message that says why."""
    code = ("import ctypes as C\n"
            "import numpy as np\n"
            "import pyclaw_amd as pyclaw\n"
            "from pyclaw_amd import _lib\n"
            "L = _lib.lib()\n"
            "assert L.pcl_version() >= 101\n"
            "o = np.zeros(4, dtype=np.int32)\n"
            "_lib.check(L.pcl_halo_region(0, 1, 15, 11, 2, _lib.i(o)))\n"
            "try:\n"
            "    pyclaw.CellSource('q[0] = 0.0;').compile(1, 0, 1)\n"
            "except _lib.PclError as e:\n"
            "    assert 'libhiprtc' in str(e), str(e)\n"
            "    print('refused')\n")
    env = dict(os.environ, PCL_HIPRTC_LIB=str(tmp_path / "no_such_libhiprtc.so"), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=120)
    assert out.returncode == 0 and "refused" in out.stdout, out.stdout
