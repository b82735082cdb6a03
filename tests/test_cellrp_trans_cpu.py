"""
CPU: the transverse body of a user-written Riemann solver (pyclaw.CellRiemann(..., transverse=...), pcl_cellrp_compile_t,
pcl_cellrp_transverse, pcl_create_cellrp) as far as it goes without a device: the run-time compile of the
two unsplit kernels next to the sweeps, the slices per workgroup the handle records, the diagnostics with the transverse
body's own line numbers, the cache, and every refusal -- each of which comes before any device call.
"""
import ctypes as C

import pytest

import pyclaw_amd as pyclaw
from apps import problems
from pyclaw_amd import _lib

PCL_RP_CELL = 100


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def transverse_of(rp):
    has, slices = C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.lib().pcl_cellrp_transverse(rp._rp, C.byref(has), C.byref(slices)))
    return has.value, slices.value


def test_the_transverse_text_makes_another_larger_program_and_is_cached():
    tag = "// trans cpu test\n"
    plain = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP + tag, 3, 2, 2).compile()
    n0, h0 = stats()
    full = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP + tag, 3, 2, 2, transverse=problems.ACOUSTICS_2D_RPT).compile()
    assert stats() == (n0 + 1, h0)
    assert full._rp.value != plain._rp.value and full.code_size > plain.code_size
    assert full.has_transverse and not plain.has_transverse
    assert transverse_of(full) == (1, 16)
    assert transverse_of(plain)[0] == 0
    again = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP + tag, 3, 2, 2, transverse=problems.ACOUSTICS_2D_RPT).compile()
    assert stats() == (n0 + 1, h0 + 1) and again._rp.value == full._rp.value
    # the transverse text is part of the key
    other = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP + tag, 3, 2, 2, transverse=problems.ACOUSTICS_2D_RPT + tag).compile()
    assert stats() == (n0 + 2, h0 + 1) and other._rp.value != full._rp.value
    # a null transverse text through the new entry point is pcl_cellrp_compile itself: the same handle
    h = C.c_void_p()
    rc = _lib.lib().pcl_cellrp_compile_t((problems.ACOUSTICS_2D_RP + tag).encode(), None, b"", 3, 2, 2, 0, None, 0, C.byref(h), None)
    assert rc == 0 and h.value == plain._rp.value and stats() == (n0 + 2, h0 + 2)
    _lib.lib().pcl_cellrp_release(h)
    assert _lib.lib().pcl_cellrp_transverse(None, C.byref(C.c_int()), None) == _lib.EINVAL


def test_eight_equations_take_twelve_slices():
    rp = pyclaw.CellRiemann(problems.SCALARS_2D_RP, 8, 8, 2, transverse=problems.SCALARS_2D_RPT).compile()
    assert transverse_of(rp) == (1, 12)


def test_diagnostics_carry_the_transverse_bodys_line_numbers():
    bad = "const double stran = p[2 - ixy];\nbmasdq[0] = no_such_name * asdq[0];\n"
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann(problems.ADVECTION_2D_RP, 1, 1, 2, transverse=bad).compile()
    assert "no_such_name" in str(e.value) and "transverse:2:" in str(e.value)
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann("s[0] = 1.0;\namdq[0] = other_name;\n", 1, 1, 2, transverse=problems.ADVECTION_2D_RPT).compile()
    assert "other_name" in str(e.value) and "riemann:2:" in str(e.value) and "transverse:" not in str(e.value)


def test_a_transverse_body_in_1d_is_refused():
    with pytest.raises(ValueError, match="transverse"):
        pyclaw.CellRiemann(problems.BURGERS_1D_RP, 1, 1, 1, transverse=problems.BURGERS_2D_RPT)
    h = C.c_void_p()
    rc = _lib.lib().pcl_cellrp_compile_t(problems.BURGERS_1D_RP.encode(), problems.BURGERS_2D_RPT.encode(), b"", 1, 1, 1, 0,
                                         None, 0, C.byref(h), None)
    assert rc == _lib.EINVAL and "ndim must be 2" in last_error()


def cell_config(**over):
    cfg = _lib.Config()
    cfg.ndim = over.pop("ndim", 2)
    for k in range(cfg.ndim):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, 3, 2, 0
    for k, v in enumerate([1, 2, 2, 0, 0, 0, 0]):           # unsplit, order_trans = 2
        cfg.method[k] = v
    cfg.mthlim[0] = cfg.mthlim[1] = 4
    cfg.rp = PCL_RP_CELL
    for k, v in enumerate([1.0, 4.0, 2.0, 2.0]):
        cfg.rp_params[k] = v
    for k, v in over.items():
        if k == "mcapa":
            cfg.method[5] = v
        else:
            setattr(cfg, k, v)
    return cfg


@pytest.fixture(scope="module")
def handles():
    plain = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2).compile()
    full = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2, transverse=problems.ACOUSTICS_2D_RPT).compile()
    return plain, full


def test_pcl_create_cellrp_takes_an_unsplit_config_only_with_a_transverse_body(handles):
    plain, full = handles
    L = _lib.lib()
    s = C.c_void_p()
    rc = L.pcl_create_cellrp(C.byref(cell_config()), plain._rp, C.byref(s))
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and "transverse" in last_error()
    rc = L.pcl_create_cellrp(C.byref(cell_config()), full._rp, C.byref(s))
    assert rc in (_lib.OK, _lib.ENODEVICE), last_error()     # the argument checks are through: no device, or a solver
    if rc == _lib.OK:
        L.pcl_destroy(s)
    # pcl_create cannot know the handle and goes on refusing
    assert L.pcl_create(C.byref(cell_config()), C.byref(s)) == _lib.EINVAL and "transverse" in last_error()
    assert L.pcl_create_cellrp(C.byref(cell_config()), None, C.byref(s)) == _lib.EINVAL
    assert L.pcl_create_cellrp(C.byref(cell_config(rp=10)), full._rp, C.byref(s)) == _lib.EINVAL


@pytest.mark.parametrize("over,word", [(dict(fwave=1), "f-waves"), (dict(mcapa=1, maux=1), "capacity function"),
                                       (dict(kind=1, mbc=3, lim_type=2), "SharpClaw"), (dict(ndim=3, maux=2), "ndim == 3")])
def test_pcl_create_cellrp_keeps_the_other_refusals(handles, over, word):
    s = C.c_void_p()
    rc = _lib.lib().pcl_create_cellrp(C.byref(cell_config(**over)), handles[1]._rp, C.byref(s))
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and word in last_error()


def make_solution(mcapa=None):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xy"]
    state = pyclaw.State(pyclaw.Grid(dims), 1, 1 if mcapa is not None else 0)
    state.q[...] = 1.0
    if mcapa is not None:
        state.aux[...] = 1.0
        state.mcapa = mcapa
    return pyclaw.Solution(state)


def unsplit_solver(transverse):
    s = pyclaw.ClawSolver2D()
    s.rp = pyclaw.CellRiemann(problems.BURGERS_2D_RP, 1, 1, 2, transverse=transverse)
    s.mwaves = 1
    s.dim_split = False
    return s


def test_setup_unsplit_says_why_it_refuses(monkeypatch):
    with pytest.raises(NotImplementedError, match="transverse Riemann solver"):
        unsplit_solver(None).setup(make_solution())
    s = unsplit_solver(problems.BURGERS_2D_RPT)
    s.fwave = True
    with pytest.raises(NotImplementedError, match="fwave = True"):
        s.setup(make_solution())
    with pytest.raises(NotImplementedError, match="capacity function"):
        unsplit_solver(problems.BURGERS_2D_RPT).setup(make_solution(mcapa=0))
    from pyclaw_amd import parallel
    sol = make_solution()
    sol.states[0].decomp = object()         # only looked at as "decomposed"; the refusal comes before it is used
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        unsplit_solver(problems.BURGERS_2D_RPT).setup(sol)
