"""
CPU: user-written Riemann solvers (pyclaw.CellRiemann, pcl_cellrp_* and PCL_RP_CELL in include/pyclaw_amd.h) as far as
they go without a device -- the run-time compile of the library's own sweep kernel around the body for every arithmetic
mode, its diagnostics with the body's line numbers, the shared per-process cache, and every refusal, each of which
comes before any device call.  Also what the feature must not have moved: the table of built-in solvers, pcl_rp_info
and the kinds of pcl_cellfn_compile.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from apps import problems
from pyclaw_amd import _lib, riemann

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (meqn, mwaves, ndim)
BODIES = {"ACOUSTICS_1D_RP": (2, 2, 1), "BURGERS_1D_RP": (1, 1, 1), "ADVECTION_2D_RP": (1, 1, 2),
          "ACOUSTICS_2D_RP": (3, 2, 2), "BURGERS_2D_RP": (1, 1, 2)}
PCL_RP_CELL = 100


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


@pytest.mark.parametrize("math", ["exact", "fast", "strict"])
@pytest.mark.parametrize("name", sorted(BODIES))
def test_every_body_compiles_in_every_mode(name, math):
    meqn, mwaves, ndim = BODIES[name]
    rp = pyclaw.CellRiemann(getattr(problems, name), meqn, mwaves, ndim).compile(math)
    assert rp.code_size > 0


def test_same_text_is_a_cache_hit_and_mwaves_and_math_are_part_of_the_key():
    body = problems.BURGERS_1D_RP + "// cache test\n"
    n0, h0 = stats()
    a = pyclaw.CellRiemann(body, 1, 1, 1).compile()
    b = pyclaw.CellRiemann(body, 1, 1, 1).compile()
    assert stats() == (n0 + 1, h0 + 1)
    assert a._rp.value == b._rp.value
    c = pyclaw.CellRiemann(body, 1, 2, 1).compile()             # another mwaves: another function
    assert stats() == (n0 + 2, h0 + 1) and c._rp.value != a._rp.value
    d = pyclaw.CellRiemann(body, 1, 1, 1).compile('fast')
    assert stats() == (n0 + 3, h0 + 1) and d._rp.value != a._rp.value
    first = a._rp.value
    a.release()
    b.release()
    assert _lib.lib().pcl_cellrp_release(C.c_void_p(first)) == _lib.EINVAL     # both references are gone
    assert pyclaw.CellRiemann(body, 1, 1, 1).compile()._rp.value == first       # released, not forgotten
    assert stats() == (n0 + 3, h0 + 2)


def test_diagnostics_carry_the_users_line_numbers():
    bad = "wave[0][0] = qr[0] - ql[0];\ns[0] = 1.0;\namdq[0] = no_such_name;\n"
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann(bad, 1, 1, 1).compile()
    assert "no_such_name" in str(e.value) and "riemann:3" in str(e.value)
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann("s[0] = half(1.0);", 1, 1, 1,
                           preamble="__device__ inline double half(double v) {\n  return 0.5 * v + other_name;\n}\n").compile()
    assert "other_name" in str(e.value) and "preamble:2" in str(e.value)


def test_preamble_helpers_and_rp_helpers_are_in_scope():
    pre = "__device__ inline double mean(double a, double b) { return 0.5 * (a + b); }\n"
    body = "wave[0][0] = qr[0] - ql[0];\ns[0] = fdiv(dsqrt(mean(ql[0], qr[0])), Recip(p[0]).div(1.0));\n" \
           "amdq[0] = dmin(s[0], 0.0) * wave[0][0];\napdq[0] = dmax(s[0], 0.0) * wave[0][0];\n"
    assert pyclaw.CellRiemann(body, 1, 1, 2, params=[2.0], preamble=pre).compile().code_size > 0


@pytest.mark.parametrize("meqn,mwaves", [(0, 1), (9, 1), (1, 0), (1, 9)])
def test_sizes_outside_1_to_8_are_refused(meqn, mwaves):
    with pytest.raises(ValueError, match="1 <= meqn <= 8 and 1 <= mwaves <= 8"):
        pyclaw.CellRiemann("s[0] = 1.0;", meqn, mwaves, 1)
    rp = C.c_void_p()
    rc = _lib.lib().pcl_cellrp_compile(b"s[0] = 1.0;", b"", meqn, mwaves, 1, 0, C.byref(rp), None)
    assert rc == _lib.EINVAL and "1 <= meqn <= 8 and 1 <= mwaves <= 8" in last_error()


def test_nine_parameters_ndim_3_and_bad_arguments_are_refused():
    with pytest.raises(ValueError, match="at most 8 parameters"):
        pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 1, params=range(9))
    rp = pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 1, params=range(8))
    with pytest.raises(ValueError, match="at most 8 parameters"):
        rp.params = [0.0] * 9
    L = _lib.lib()
    assert L.pcl_cellrp_params(None, None, 9) == _lib.EINVAL and "at most 8 parameters" in last_error()
    with pytest.raises(ValueError, match="ndim must be 1 or 2"):
        pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 3)
    h = C.c_void_p()
    assert L.pcl_cellrp_compile(b"s[0] = 1.0;", b"", 1, 1, 3, 0, C.byref(h), None) == _lib.EINVAL
    assert "ndim must be 1 or 2" in last_error()
    assert L.pcl_cellrp_compile(b"s[0] = 1.0;", b"", 1, 1, 1, 7, C.byref(h), None) == _lib.EINVAL      # no such math mode
    assert L.pcl_cellrp_compile(None, b"", 1, 1, 1, 0, C.byref(h), None) == _lib.EINVAL
    assert L.pcl_cellrp_attach(None, None) == _lib.EINVAL


def test_a_handle_compiled_for_other_constants_is_refused():
    rp = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2).compile()
    L = _lib.lib()
    assert L.pcl_cellrp_check(rp._rp, 3, 2, 2, 0) == 0
    for other in [(4, 2, 2, 0), (3, 3, 2, 0), (3, 2, 1, 0), (3, 2, 2, 1)]:
        assert L.pcl_cellrp_check(rp._rp, *other) == _lib.EINVAL
        assert "compiled for meqn=3 mwaves=2 ndim=2 math=0" in last_error()
    assert L.pcl_cellrp_check(None, 3, 2, 2, 0) == _lib.EINVAL
    # a cell function handle is not a Riemann solver handle, and the other way round
    src = pyclaw.CellSource("q[0] = 0.0;").compile(3, 0, 2)
    assert L.pcl_cellrp_check(src._fn, 3, 2, 2, 0) == _lib.EINVAL
    assert L.pcl_cellfn_check(rp._rp, 3, 0, 2) == _lib.EINVAL


def cell_config(ndim=2, **over):
    cfg = _lib.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, 3, 2, 0
    for k, v in enumerate([1, 2, -1 if ndim > 1 else 0, 0, 0, 0, 0]):
        cfg.method[k] = v
    cfg.rp = PCL_RP_CELL
    for k, v in over.items():
        if k == "mcapa":
            cfg.method[5] = v
        elif k == "order_trans":
            cfg.method[2] = v
        else:
            setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("over,word", [(dict(fwave=1), "f-waves"), (dict(mcapa=1, maux=1), "capacity function"),
                                       (dict(kind=1, mbc=3, lim_type=2), "SharpClaw"), (dict(order_trans=1), "transverse"),
                                       (dict(meqn=9), "meqn")])
def test_pcl_create_refuses_what_a_user_solver_does_not_serve(over, word):
    """EINVAL with the reason, from the host-only checks: not ENODEVICE, which is what a machine without a GPU answers
    once the argument checks are through."""
    h = C.c_void_p()
    rc = _lib.lib().pcl_create(C.byref(cell_config(**over)), C.byref(h))
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and word in last_error()


def test_pcl_create_refuses_a_user_solver_in_3d():
    h = C.c_void_p()
    cfg = cell_config(ndim=3, maux=2)
    cfg.method[2] = -1
    assert _lib.lib().pcl_create(C.byref(cfg), C.byref(h)) == _lib.EINVAL
    assert "PCL_RP_CELL" in last_error() and "ndim == 3" in last_error()


def test_stateless_calls_take_no_user_solver():
    q = np.zeros((1, 12), order='F')
    cfl = C.c_double()
    method = np.array([1, 2, 0, 0, 0, 0, 0], dtype=np.int32)
    mthlim = np.array([4], dtype=np.int32)
    rc = _lib.lib().pcl_step1(PCL_RP_CELL, None, 1, 1, 0, 2, 8, _lib.d(q), None, 0.1, 0.01, _lib.i(method), _lib.i(mthlim),
                              C.byref(cfl))
    assert rc == _lib.EINVAL and "user-written" in last_error()


def make_solution(ndim, meqn=1, mcapa=None):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xyz"[:ndim]]
    state = pyclaw.State(pyclaw.Grid(dims), meqn, 1 if mcapa is not None else 0)
    state.q[...] = 1.0
    if mcapa is not None:
        state.aux[...] = 1.0
        state.mcapa = mcapa
    return pyclaw.Solution(state)


def test_setup_says_why_it_refuses():
    body = problems.BURGERS_2D_RP
    s = pyclaw.ClawSolver2D()
    s.rp = pyclaw.CellRiemann(body, 1, 1, 2)
    s.mwaves = 1
    s.dim_split = False
    with pytest.raises(NotImplementedError, match="transverse Riemann solver"):
        s.setup(make_solution(2))
    s = pyclaw.ClawSolver2D()
    s.rp = pyclaw.CellRiemann(body, 1, 1, 2)
    s.mwaves = 1
    s.fwave = True
    with pytest.raises(NotImplementedError, match="fwave = True"):
        s.setup(make_solution(2))
    s = pyclaw.ClawSolver2D()
    s.rp = pyclaw.CellRiemann(body, 1, 1, 2)
    s.mwaves = 1
    with pytest.raises(NotImplementedError, match="capacity function"):
        s.setup(make_solution(2, mcapa=0))
    s = pyclaw.ClawSolver3D()
    s.rp = pyclaw.CellRiemann(body, 1, 1, 2)
    s.mwaves = 1
    with pytest.raises(NotImplementedError, match="ClawSolver3D"):
        s.setup(make_solution(3))
    for cls, nd in [(pyclaw.SharpClawSolver1D, 1), (pyclaw.SharpClawSolver2D, 2)]:
        s = cls()
        s.rp = pyclaw.CellRiemann(body, 1, 1, nd)
        s.mwaves = 1
        with pytest.raises(NotImplementedError, match="SharpClaw"):
            s.setup(make_solution(nd))


def test_more_than_one_rank_is_refused(monkeypatch):
    from pyclaw_amd import parallel
    sol = make_solution(2)
    sol.states[0].decomp = object()         # only looked at as "decomposed"; the refusal comes before it is used
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    s = pyclaw.ClawSolver2D()
    s.rp = pyclaw.CellRiemann(problems.BURGERS_2D_RP, 1, 1, 2)
    s.mwaves = 1
    with pytest.raises(NotImplementedError, match="more than one rank"):
        s.setup(sol)


def test_the_user_solver_is_no_table_entry():
    rp = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2, params=[1.0, 4.0, 2.0, 2.0], name="mine")
    assert isinstance(rp, riemann.RiemannSolver) and rp.id == PCL_RP_CELL and rp.cparam == () and not rp.has_transverse
    assert riemann.get(rp) is rp
    assert rp.all_params(None) == [1.0, 4.0, 2.0, 2.0]
    assert len(riemann._ALL) == 16 and rp not in riemann._ALL and "mine" not in riemann.BY_NAME
    assert all(r.id != PCL_RP_CELL for r in riemann._ALL)
    info = np.zeros(10, dtype=np.int32)
    assert _lib.lib().pcl_rp_info(PCL_RP_CELL, _lib.i(info)) == _lib.EINVAL
    fn = C.c_void_p()
    assert _lib.lib().pcl_cellfn_compile(5, b"q[0] = 1.0;", b"", 1, 0, 1, 0, 0, C.byref(fn), None) == _lib.EINVAL
    assert _lib.lib().pcl_version() >= 106


def test_library_works_where_hiprtc_cannot_be_opened(tmp_path):
    code = ("import numpy as np\n"
            "import pyclaw_amd as pyclaw\n"
            "from pyclaw_amd import _lib\n"
            "L = _lib.lib()\n"
            "o = np.zeros(4, dtype=np.int32)\n"
            "_lib.check(L.pcl_halo_region(0, 1, 15, 11, 2, _lib.i(o)))\n"
            "try:\n"
            "    pyclaw.CellRiemann('s[0] = 1.0;', 1, 1, 1).compile()\n"
            "except _lib.PclError as e:\n"
            "    assert 'libhiprtc' in str(e), str(e)\n"
            "    print('refused')\n"
            "_lib.check(L.pcl_halo_region(0, 1, 15, 11, 2, _lib.i(o)))\n")
    env = dict(os.environ, PCL_HIPRTC_LIB=str(tmp_path / "no_such_libhiprtc.so"), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=120)
    assert out.returncode == 0 and "refused" in out.stdout, out.stdout
