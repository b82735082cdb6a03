"""
CPU: user-written Riemann solvers that read aux arrays (pyclaw.CellRiemann(..., aux=...), pcl_cellrp_compile_aux and
pcl_cellrp_aux in include/pyclaw_amd.h) as far as they go without a device -- the run-time compile of the sweep kernel
with NAUX > 0 around the body for every arithmetic mode, the list as part of the cache key, and every new refusal, each
of which comes before any device call (an index past maux would be a read outside the aux allocation).  Also that what a
CellRiemann was refused before it is still refused, in the same words, when it lists aux.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from apps import problems
from pyclaw_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (meqn, mwaves, ndim, aux)
BODIES = {"ADVECTION_COLOR_1D_RP": (1, 1, 1, (0,)), "VC_ADVECTION_2D_RP": (1, 1, 2, (0, 1)),
          "VC_ACOUSTICS_2D_RP": (3, 2, 2, (0, 1)), "VC_ACOUSTICS_1D_RP": (2, 2, 1, (0, 1))}
PCL_RP_CELL = 100


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def compile_aux(body, meqn, mwaves, ndim, aux, math=0):
    """pcl_cellrp_compile_aux -> (return code, handle value)"""
    h = C.c_void_p()
    rc = _lib.lib().pcl_cellrp_compile_aux(body.encode(), b"", meqn, mwaves, ndim, math, ints(*aux), len(aux), C.byref(h), None)
    return rc, h.value


@pytest.mark.parametrize("math", ["exact", "fast", "strict"])
@pytest.mark.parametrize("name", sorted(BODIES))
def test_every_aux_body_compiles_in_every_mode(name, math):
    meqn, mwaves, ndim, aux = BODIES[name]
    rp = pyclaw.CellRiemann(getattr(problems, name), meqn, mwaves, ndim, aux=aux).compile(math)
    assert rp.code_size > 0 and rp.aux == aux and not rp.has_transverse


def test_the_list_and_its_order_are_part_of_the_cache_key():
    body = problems.VC_ACOUSTICS_2D_RP + "// aux cache test\n"
    n0, h0 = stats()
    a = pyclaw.CellRiemann(body, 3, 2, 2, aux=(0, 1)).compile()
    b = pyclaw.CellRiemann(body, 3, 2, 2, aux=(0, 1)).compile()
    assert stats() == (n0 + 1, h0 + 1) and a._rp.value == b._rp.value
    c = pyclaw.CellRiemann(body, 3, 2, 2, aux=(0, 2)).compile()             # another list: another program
    assert stats() == (n0 + 2, h0 + 1) and c._rp.value != a._rp.value
    d = pyclaw.CellRiemann(body, 3, 2, 2, aux=(1, 0)).compile()             # another order: another program
    assert stats() == (n0 + 3, h0 + 1) and d._rp.value not in (a._rp.value, c._rp.value)
    rc, raw = compile_aux(body, 3, 2, 2, (1, 0))                           # the C entry point meets the Python object's entry
    assert rc == 0 and raw == d._rp.value and stats() == (n0 + 3, h0 + 2)
    assert _lib.lib().pcl_cellrp_release(C.c_void_p(raw)) == 0
    # the same CellRiemann object compiles again when its list changed and not when it did not
    assert a.compile() is a and stats() == (n0 + 3, h0 + 2)


def test_an_empty_list_is_pcl_cellrp_compile_itself():
    body = problems.BURGERS_1D_RP + "// empty aux list\n"
    n0, h0 = stats()
    plain = pyclaw.CellRiemann(body, 1, 1, 1).compile()
    rc, raw = compile_aux(body, 1, 1, 1, ())
    assert rc == 0 and raw == plain._rp.value and stats() == (n0 + 1, h0 + 1)
    assert _lib.lib().pcl_cellrp_release(C.c_void_p(raw)) == 0
    assert pyclaw.CellRiemann(body, 1, 1, 1, aux=()).compile()._rp.value == raw
    h = C.c_void_p()
    assert _lib.lib().pcl_cellrp_compile_aux(body.encode(), b"", 1, 1, 1, 0, None, 0, C.byref(h), None) == 0 and h.value == raw
    assert _lib.lib().pcl_cellrp_release(h) == 0
    n, idx = C.c_int(-1), ints(*[-1] * 8)
    assert _lib.lib().pcl_cellrp_aux(plain._rp, C.byref(n), idx) == 0 and n.value == 0 and list(idx) == [-1] * 8


def test_pcl_cellrp_aux_returns_the_list_and_check_answers_as_before():
    L = _lib.lib()
    rp = pyclaw.CellRiemann(problems.VC_ACOUSTICS_2D_RP, 3, 2, 2, aux=(3, 1)).compile()
    n, idx = C.c_int(), ints(*[-1] * 8)
    assert L.pcl_cellrp_aux(rp._rp, C.byref(n), idx) == 0
    assert n.value == 2 and list(idx) == [3, 1] + [-1] * 6
    assert L.pcl_cellrp_aux(rp._rp, C.byref(n), None) == 0 and n.value == 2
    assert L.pcl_cellrp_aux(None, C.byref(n), idx) == _lib.EINVAL
    assert L.pcl_cellrp_aux(rp._rp, None, idx) == _lib.EINVAL
    assert L.pcl_cellrp_check(rp._rp, 3, 2, 2, 0) == 0
    for other in [(4, 2, 2, 0), (3, 3, 2, 0), (3, 2, 1, 0), (3, 2, 2, 1)]:
        assert L.pcl_cellrp_check(rp._rp, *other) == _lib.EINVAL
        assert "compiled for meqn=3 mwaves=2 ndim=2 math=0" in last_error()


def test_bad_lists_are_refused_with_the_reason():
    body = "s[0] = auxr[0];"
    rc, _ = compile_aux(body, 1, 1, 1, (0, -1))
    assert rc == _lib.EINVAL and "-1" in last_error() and "negative" in last_error()
    rc, _ = compile_aux(body, 1, 1, 1, (2, 0, 2))
    assert rc == _lib.EINVAL and "aux index 2" in last_error() and "twice" in last_error()
    h = C.c_void_p()
    rc = _lib.lib().pcl_cellrp_compile_aux(body.encode(), b"", 1, 1, 1, 0, ints(0), -1, C.byref(h), None)
    assert rc == _lib.EINVAL and "naux" in last_error()
    rc = _lib.lib().pcl_cellrp_compile_aux(body.encode(), b"", 1, 1, 1, 0, None, 1, C.byref(h), None)
    assert rc == _lib.EINVAL
    with pytest.raises(ValueError, match="negative"):
        pyclaw.CellRiemann(body, 1, 1, 1, aux=(0, -1))
    with pytest.raises(ValueError, match="twice"):
        pyclaw.CellRiemann(body, 1, 1, 1, aux=(2, 0, 2))


@pytest.mark.parametrize("meqn,naux", [(3, 6), (8, 1), (1, 8)])
def test_more_planes_than_the_tile_holds_are_refused_with_the_limit(meqn, naux):
    """the tile of the y pass is 64 x 16 cells: 65536 / (8 * 1024) = 8 planes of q and aux together"""
    n0 = stats()
    rc, _ = compile_aux("s[0] = auxr[0];", meqn, 1, 2, tuple(range(naux)))
    assert rc == _lib.EINVAL and "meqn + naux = %d" % (meqn + naux) in last_error() and "at most 8 planes" in last_error()
    assert stats() == n0                        # refused before the compiler ran
    with pytest.raises(ValueError, match=r"meqn \+ len\(aux\) = %d.*at most 8 planes" % (meqn + naux)):
        pyclaw.CellRiemann("s[0] = auxr[0];", meqn, 1, 2, aux=range(naux))
    # what fits compiles: the static_assert of the program text counts the same sum
    if meqn == 3:
        assert pyclaw.CellRiemann("s[0] = auxr[4];", 3, 1, 2, aux=range(5)).compile().code_size > 0


def test_a_body_that_reads_aux_without_a_list_does_not_compile():
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann("wave[0][0] = qr[0] - ql[0];\ns[0] = auxl[0];\n", 1, 1, 1).compile()
    assert "auxl" in str(e.value) and "riemann:2" in str(e.value)
    with pytest.raises(_lib.PclError) as e:           # and with a list the diagnostics keep the body's line numbers
        pyclaw.CellRiemann("wave[0][0] = qr[0] - ql[0];\ns[0] = auxr[0];\namdq[0] = no_such_name;\n", 1, 1, 1, aux=(0,)).compile()
    assert "no_such_name" in str(e.value) and "riemann:3" in str(e.value)


def make_solution(ndim, meqn=1, maux=0, mcapa=None):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xyz"[:ndim]]
    state = pyclaw.State(pyclaw.Grid(dims), meqn, maux)
    state.q[...] = 1.0
    if maux:
        state.aux[...] = 1.0
    if mcapa is not None:
        state.mcapa = mcapa
    return pyclaw.Solution(state)


def user_solver(cls, ndim, aux=(0, 1)):
    s = cls()
    s.rp = pyclaw.CellRiemann(problems.VC_ADVECTION_2D_RP if ndim == 2 else problems.ADVECTION_COLOR_1D_RP, 1, 1, ndim,
                              aux=aux if ndim == 2 else aux[:1])
    s.mwaves = 1
    return s


def test_setup_refuses_a_state_whose_aux_does_not_reach_the_list():
    """ValueError before pcl_create: a machine without a GPU would answer ENODEVICE there (a PclError), and one with a GPU
    would go on to pcl_cellrp_attach and its refusal (a PclError as well)"""
    s = user_solver(pyclaw.ClawSolver2D, 2, aux=(0, 2))
    with pytest.raises(ValueError, match=r"aux component 2 \(0-based\) and state.maux = 2"):
        s.setup(make_solution(2, maux=2))
    s = user_solver(pyclaw.ClawSolver2D, 2)
    sol = make_solution(2)
    assert sol.states[0].aux is None
    with pytest.raises(ValueError, match="state.aux is None"):
        s.setup(sol)


def test_what_a_user_solver_does_not_serve_is_still_refused_with_aux():
    s = user_solver(pyclaw.ClawSolver2D, 2)
    s.dim_split = False
    with pytest.raises(NotImplementedError, match="transverse Riemann solver"):
        s.setup(make_solution(2, maux=2))
    s = user_solver(pyclaw.ClawSolver2D, 2)
    s.fwave = True
    with pytest.raises(NotImplementedError, match="fwave = True"):
        s.setup(make_solution(2, maux=2))
    s = user_solver(pyclaw.ClawSolver2D, 2)
    with pytest.raises(NotImplementedError, match="capacity function"):
        s.setup(make_solution(2, maux=3, mcapa=2))
    s = user_solver(pyclaw.ClawSolver3D, 2)
    with pytest.raises(NotImplementedError, match="ClawSolver3D"):
        s.setup(make_solution(3, maux=2))
    for cls, nd in [(pyclaw.SharpClawSolver1D, 1), (pyclaw.SharpClawSolver2D, 2)]:
        s = user_solver(cls, nd)
        with pytest.raises(NotImplementedError, match="SharpClaw"):
            s.setup(make_solution(nd, maux=2))
    capacity_function_beside_aux_is_refused_by_pcl_create()


def test_more_than_one_rank_is_still_refused_with_aux(monkeypatch):
    from pyclaw_amd import parallel
    sol = make_solution(2, maux=2)
    sol.states[0].decomp = object()         # only looked at as "decomposed"; the refusal comes before it is used
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    s = user_solver(pyclaw.ClawSolver2D, 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        s.setup(sol)


def capacity_function_beside_aux_is_refused_by_pcl_create():
    cfg = _lib.Config()
    cfg.ndim = 2
    for k in range(2):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, 3, 2, 3
    for k, v in enumerate([1, 2, -1, 0, 0, 3, 3]):
        cfg.method[k] = v
    cfg.rp = PCL_RP_CELL
    h = C.c_void_p()
    rc = _lib.lib().pcl_create(C.byref(cfg), C.byref(h))
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and "capacity function" in last_error()


def test_version_and_the_binding_table():
    assert _lib.lib().pcl_version() >= 107
    text = open(os.path.join(ROOT, "include", "pyclaw_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(pcl_[a-z0-9_]+)\s*\(", text)))
    assert "pcl_cellrp_compile_aux" in syms and "pcl_cellrp_aux" in syms
    assert sorted(_lib.PROTOTYPES) == syms
    # pcl_cellrp_compile and pcl_cellrp_check keep their signatures
    assert len(_lib.PROTOTYPES["pcl_cellrp_compile"][1]) == 8 and len(_lib.PROTOTYPES["pcl_cellrp_check"][1]) == 5
    assert np.dtype(np.int32).itemsize == C.sizeof(C.c_int)      # the list travels as C ints
