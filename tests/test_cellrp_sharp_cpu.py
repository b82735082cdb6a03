"""
CPU: user-written Riemann solvers in the SharpClaw stages (pyclaw.CellRiemann(..., sharpclaw=True),
pcl_cellrp_compile_sharp, pcl_cellrp_sharp, pcl_create_cellrp with cfg.kind = 1) as far as it goes without
a device: the run-time compile of the SharpClaw kernels around a body, the cache and its key, the diagnostics, and every
refusal, each of which comes before the compiler or before any device call.
"""
import ctypes as C

import pytest

import pyclaw_amd as pyclaw
from apps import problems
from pyclaw_amd import _lib

PCL_RP_CELL = 100
FWAVE, CAPA = 1, 2
# assigns neither wave nor fwave, reads no aux: compiles in every form, with any list
TINY = "s[0] = p[0];\namdq[0] = dmin(p[0], 0.0) * (qr[0] - ql[0]);\napdq[0] = dmax(p[0], 0.0) * (qr[0] - ql[0]);\n"


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def sharp_of(handle):
    v = [C.c_int(-1) for _ in range(3)]
    _lib.check(_lib.lib().pcl_cellrp_sharp(handle, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def compile_sharp(body, meqn, mwaves, ndim, lim_type, weno_order, char_decomp, aux=(), form=0, math=0):
    h, size = C.c_void_p(), C.c_long()
    rc = _lib.lib().pcl_cellrp_compile_sharp(body.encode(), b"", meqn, mwaves, ndim, math,
                                             (C.c_int * len(aux))(*aux) if aux else None, len(aux), form, lim_type, weno_order,
                                             char_decomp, C.byref(h), C.byref(size))
    return rc, h, size.value


def test_version():
    assert _lib.lib().pcl_version() >= 110


def test_a_sharpclaw_compile_and_its_cache_key():
    body = "// sharp cpu test 0\n" + TINY
    n0, h0 = stats()
    rc, base, size = compile_sharp(body, 1, 1, 1, 2, 5, 0)
    assert rc == 0 and base.value and size > 0, last_error()
    assert sharp_of(base) == (2, 5, 0)
    assert stats() == (n0 + 1, h0)
    rc, again, size2 = compile_sharp(body, 1, 1, 1, 2, 5, 0)
    assert rc == 0 and again.value == base.value and size2 == size and stats() == (n0 + 1, h0 + 1)
    seen = {base.value}
    # each of lim_type, weno_order, char_decomp, the capa bit and the aux list is part of the key
    others = [dict(lim_type=1), dict(weno_order=7), dict(char_decomp=1), dict(form=CAPA), dict(aux=(0,))]
    for k, over in enumerate(others):
        kw = dict(lim_type=2, weno_order=5, char_decomp=0, aux=(), form=0)
        kw.update(over)
        rc, h, size = compile_sharp(body, 1, 1, 1, **kw)
        assert rc == 0 and size > 0, (over, last_error())
        assert h.value not in seen, over
        seen.add(h.value)
        assert stats() == (n0 + 2 + k, h0 + 1), over
        assert sharp_of(h) == (kw["lim_type"], kw["weno_order"], kw["char_decomp"])
        f = C.c_int(-1)
        _lib.check(_lib.lib().pcl_cellrp_form(h, C.byref(f)))
        assert f.value == kw["form"]
    # a classic handle of the same text: an entry of its own, the one pcl_cellrp_compile has always made, and three zeros
    n1, h1 = stats()
    rp = pyclaw.CellRiemann(body, 1, 1, 1).compile()
    assert rp._rp.value not in seen and stats() == (n1 + 1, h1)
    assert sharp_of(rp._rp) == (0, 0, 0)
    g, gsize = C.c_void_p(), C.c_long()
    assert _lib.lib().pcl_cellrp_compile(body.encode(), b"", 1, 1, 1, 0, C.byref(g), C.byref(gsize)) == 0
    assert g.value == rp._rp.value and stats() == (n1 + 1, h1 + 1)
    # the Python object: the three are part of its key too
    user = pyclaw.CellRiemann(body, 1, 1, 1, sharpclaw=True)
    user.compile(sharp=(2, 5, 0))
    assert user._rp.value == base.value and user.code_size > 0
    user.compile(sharp=(1, 5, 0))
    assert user._rp.value != base.value and sharp_of(user._rp) == (1, 5, 0)
    with pytest.raises(ValueError, match="sharpclaw=True"):
        user.compile()
    with pytest.raises(ValueError, match="sharpclaw=True"):
        rp.compile(sharp=(2, 5, 0))
    v = C.c_int()
    assert _lib.lib().pcl_cellrp_sharp(None, C.byref(v), C.byref(v), C.byref(v)) == _lib.EINVAL
    assert _lib.lib().pcl_cellrp_sharp(base, None, C.byref(v), C.byref(v)) == _lib.EINVAL


def test_two_dimensions_and_the_other_modes_compile():
    """Both passes of a 2-D system with aux and a capacity function, and the fast and strict texts."""
    rp = pyclaw.CellRiemann(problems.VC_ACOUSTICS_2D_RP, 3, 2, 2, aux=(0, 1), capa=True, sharpclaw=True)
    assert rp.compile(sharp=(2, 5, 0)).code_size > 0
    for math in ("fast", "strict"):
        rp = pyclaw.CellRiemann(problems.ACOUSTICS_1D_RP, 2, 2, 1, sharpclaw=True)
        assert rp.compile(math, sharp=(2, 5, 0)).code_size > 0


def test_a_syntax_error_keeps_the_users_line():
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann("s[0] = 1.0;\namdq[0] = = 2.0;\n", 1, 1, 1, sharpclaw=True).compile(sharp=(2, 5, 0))
    assert "riemann:2:" in str(e.value)
    rc, h, _ = compile_sharp("s[0] = 1.0;\nnot_declared = 2.0;\n", 1, 1, 2, 3, 5, 0)
    assert rc == _lib.EINVAL and h.value is None and "riemann:2:" in last_error()


# ---- the compile entry point's refusals: before the compiler -----------------------------------------------------------

@pytest.mark.parametrize("kw,word", [
    (dict(lim_type=1, weno_order=7), "lim_type 2"), (dict(lim_type=3, weno_order=17), "lim_type 2"),      # weno_order > 5
    (dict(lim_type=0), "lim_type"), (dict(lim_type=4), "lim_type"),
    (dict(weno_order=6), "weno_order"), (dict(weno_order=3), "weno_order"), (dict(weno_order=19), "weno_order"),
    (dict(char_decomp=2), "char_decomp"),
    (dict(char_decomp=1, ndim=2), "char_decomp = 1"), (dict(char_decomp=1, form=FWAVE), "char_decomp = 1"),
    (dict(char_decomp=1, weno_order=7), "char_decomp = 1"), (dict(char_decomp=1, lim_type=3), "char_decomp = 1"),
])
def test_compile_refuses_what_no_sharpclaw_kernel_exists_for(kw, word):
    n0, h0 = stats()
    a = dict(ndim=1, lim_type=2, weno_order=5, char_decomp=0, form=0)
    a.update(kw)
    ndim = a.pop("ndim")
    rc, h, _ = compile_sharp("s[0] = 1.0; // never compiled", 1, 1, ndim, **a)
    assert rc == _lib.EINVAL and h.value is None and word in last_error(), last_error()
    assert stats() == (n0, h0)


def test_the_plane_limit():
    """meqn + capa + naux = 9 planes of the 2-D y tile (16 strips x 64 cells x 8 bytes each) are 72 KB."""
    n0, h0 = stats()
    rc, h, _ = compile_sharp("s[0] = 1.0; // never compiled", 3, 1, 2, 2, 5, 0, aux=(0, 1, 2, 3, 4), form=CAPA)
    assert rc == _lib.EINVAL and "meqn + capa + naux = 9" in last_error() and "at most 8" in last_error()
    rc, h, _ = compile_sharp("s[0] = 1.0; // never compiled", 4, 1, 2, 2, 5, 0, aux=(0, 1, 2, 3, 4))
    assert rc == _lib.EINVAL and "meqn + capa + naux = 9" in last_error()
    # the x tile holds q and the capacity function
    rc, h, _ = compile_sharp("s[0] = 1.0; // never compiled", 8, 1, 1, 2, 5, 0, form=CAPA)
    assert rc == _lib.EINVAL and "meqn + capa = 9" in last_error() and "at most 8" in last_error()
    assert stats() == (n0, h0)
    with pytest.raises(ValueError, match=r"meqn \+ capa \+ len\(aux\) = 9"):
        pyclaw.CellRiemann("s[0] = 1.0;", 3, 1, 2, aux=(0, 1, 2, 3, 4), capa=True, sharpclaw=True)
    with pytest.raises(ValueError, match=r"= 9 with sharpclaw=True"):
        pyclaw.CellRiemann("s[0] = 1.0;", 8, 1, 1, capa=True, sharpclaw=True)
    # MAX_PLANES promises no more than the library accepts: 8 planes compile, and so do 10 with six aux components (the
    # y tile then has 8 strips)
    rp = pyclaw.CellRiemann("s[0] = 1.0; // sharp cpu test planes", 3, 1, 2, aux=(0, 1, 2, 3), capa=True, sharpclaw=True)
    assert rp.meqn + 1 + len(rp.aux) == pyclaw.CellRiemann.MAX_PLANES and rp.compile(sharp=(2, 5, 0)).code_size > 0
    rp = pyclaw.CellRiemann("s[0] = 1.0; // sharp cpu test planes", 3, 1, 2, aux=(0, 1, 2, 3, 4, 5), capa=True, sharpclaw=True)
    assert rp.compile(sharp=(2, 5, 0)).code_size > 0
    # 1-D has no y tile: the aux list does not count
    pyclaw.CellRiemann("s[0] = 1.0;", 4, 1, 1, aux=(0, 1, 2, 3, 4), sharpclaw=True)


# ---- pcl_create_cellrp: the configuration against what the handle was compiled for --------------------------------------

def sharp_config(ndim=1, lim_type=2, mbc=3, char_decomp=0, fwave=0, mcapa=0, maux=0, kind=1):
    cfg = _lib.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = mbc, 1, 1, maux
    for k, v in enumerate([1, 2, 0 if kind == 1 or ndim == 1 else -1, 0, char_decomp, mcapa, maux]):
        cfg.method[k] = v
    cfg.mthlim[0] = 4
    cfg.fwave = fwave
    cfg.rp = PCL_RP_CELL
    cfg.rp_params[0] = 1.0
    cfg.kind = kind
    cfg.lim_type = lim_type
    return cfg


@pytest.fixture(scope="module")
def handles():
    """1-D handles of one text: (lim_type, weno_order, char_decomp, form) -> handle; 'classic': the classic sweeps."""
    body = "// sharp cpu test 1\n" + TINY
    out = {}
    for key in [(2, 5, 0, 0), (1, 5, 0, 0), (2, 7, 0, 0), (2, 5, 1, 0), (2, 5, 0, FWAVE), (2, 5, 0, CAPA)]:
        rc, h, _ = compile_sharp(body, 1, 1, 1, key[0], key[1], key[2], form=key[3])
        assert rc == 0, last_error()
        out[key] = h
    out["classic"] = pyclaw.CellRiemann(body, 1, 1, 1).compile()
    rc, h, _ = compile_sharp(body, 1, 1, 2, 2, 5, 0)
    assert rc == 0, last_error()
    out["2d"] = h
    return out


def through(rc, s):
    """the argument checks are through: no device, or a solver"""
    L = _lib.lib()
    assert rc == (_lib.ENODEVICE if L.pcl_device_count() < 1 else _lib.OK), last_error()
    if rc == _lib.OK:
        L.pcl_destroy(s)


CFG_OF = {(2, 5, 0, 0): dict(), (1, 5, 0, 0): dict(lim_type=1), (2, 7, 0, 0): dict(mbc=4), (2, 5, 1, 0): dict(char_decomp=1),
          (2, 5, 0, FWAVE): dict(fwave=1), (2, 5, 0, CAPA): dict(mcapa=1, maux=1)}


@pytest.mark.parametrize("key", sorted(CFG_OF))
def test_pcl_create_cellrp_accepts_the_configuration_the_handle_was_compiled_for(handles, key):
    s = C.c_void_p()
    through(_lib.lib().pcl_create_cellrp(C.byref(sharp_config(**CFG_OF[key])), handles[key], C.byref(s)), s)


@pytest.mark.parametrize("other,word", [((1, 5, 0, 0), "lim_type"), ((2, 7, 0, 0), "weno_order"), ((2, 5, 1, 0), "char_decomp"),
                                        ((2, 5, 0, FWAVE), "f-waves"), ((2, 5, 0, CAPA), "capacity function")])
def test_every_mismatch_is_refused_in_both_directions(handles, other, word):
    """EINVAL from the host-only checks (not ENODEVICE) with a sentence that names both sides."""
    L = _lib.lib()
    base = (2, 5, 0, 0)
    s = C.c_void_p()
    for have, want in ((base, other), (other, base)):
        rc = L.pcl_create_cellrp(C.byref(sharp_config(**CFG_OF[want])), handles[have], C.byref(s))
        assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and word in last_error(), (have, want, last_error())
        assert "handle" in last_error() and s.value is None
    if word == "weno_order":
        assert "mbc" in last_error()


def test_a_sharpclaw_handle_serves_sharpclaw_and_a_classic_handle_the_classic_step(handles):
    L = _lib.lib()
    s = C.c_void_p()
    rc = L.pcl_create_cellrp(C.byref(sharp_config(kind=0, mbc=2)), handles[(2, 5, 0, 0)], C.byref(s))
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and "SharpClaw" in last_error() and "classic" in last_error()
    rc = L.pcl_create_cellrp(C.byref(sharp_config()), handles["classic"]._rp, C.byref(s))
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and "SharpClaw" in last_error()
    # the classic handle still serves the classic step, and pcl_create still knows no handle
    through(L.pcl_create_cellrp(C.byref(sharp_config(kind=0, mbc=2)), handles["classic"]._rp, C.byref(s)), s)
    rc = L.pcl_create(C.byref(sharp_config()), C.byref(s))
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error() and "SharpClaw" in last_error()
    # two dimensions: the configuration's method[2] is not a transverse order under SharpClaw
    through(L.pcl_create_cellrp(C.byref(sharp_config(ndim=2)), handles["2d"], C.byref(s)), s)


def test_the_configurations_own_conditions_hold_for_a_user_solver(handles):
    """What pcl_create refuses of any SharpClaw configuration, with a handle too: EINVAL, not ENODEVICE."""
    L = _lib.lib()
    s = C.c_void_p()
    for cfg, h, word in [(sharp_config(lim_type=1, mbc=4), handles[(2, 7, 0, 0)], "lim_type 2"),
                         (sharp_config(ndim=2, char_decomp=1), handles["2d"], "char_decomp = 1"),
                         (sharp_config(char_decomp=1, fwave=1), handles[(2, 5, 1, 0)], "char_decomp = 1"),
                         (sharp_config(char_decomp=1, mbc=4), handles[(2, 5, 1, 0)], "char_decomp = 1"),
                         (sharp_config(char_decomp=2), handles[(2, 5, 0, 0)], "char_decomp")]:
        assert L.pcl_create_cellrp(C.byref(cfg), h, C.byref(s)) == _lib.EINVAL and word in last_error(), last_error()


def test_aux_listed_beyond_maux(handles):
    rc, h, _ = compile_sharp("// sharp cpu test 2\n" + TINY, 1, 1, 1, 2, 5, 0, aux=(1,))
    assert rc == 0
    s = C.c_void_p()
    assert _lib.lib().pcl_create_cellrp(C.byref(sharp_config(maux=1)), h, C.byref(s)) == _lib.EINVAL
    assert "aux component 1" in last_error() and "maux = 1" in last_error()
    through(_lib.lib().pcl_create_cellrp(C.byref(sharp_config(maux=2)), h, C.byref(s)), s)


def test_no_fused_dq_source(handles):
    """pcl_sharp_fuse_dq_src takes a solver handle, so it runs where there is a device (tests/test_gpu_cellrp_sharp.py has
    the same check under the gpu mark); without one the create stops at the device and there is nothing to ask."""
    L = _lib.lib()
    s = C.c_void_p()
    rc = L.pcl_create_cellrp(C.byref(sharp_config()), handles[(2, 5, 0, 0)], C.byref(s))
    if L.pcl_device_count() < 1:
        assert rc == _lib.ENODEVICE
        assert L.pcl_sharp_fuse_dq_src(None, 1, None, 0) == _lib.EINVAL
        return
    assert rc == _lib.OK, last_error()
    p = (C.c_double * 2)(0.4, 2.0)
    assert L.pcl_sharp_fuse_dq_src(s, 1, p, 2) == _lib.EINVAL and "PCL_RP_CELL" in last_error()
    L.pcl_destroy(s)


# ---- setup() -----------------------------------------------------------------------------------------------------------

def make_solution(ndim, maux=0, mcapa=None):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xy"[:ndim]]
    state = pyclaw.State(pyclaw.Grid(dims), 1, maux)
    state.q[...] = 1.0
    if maux:
        state.aux[...] = 1.0
    if mcapa is not None:
        state.mcapa = mcapa
    return pyclaw.Solution(state)


SETUP_BODY = "// sharp cpu test 3\n" + TINY


def sharp_solver(ndim, **kw):
    attrs = dict((k, kw.pop(k)) for k in list(kw) if k in ("lim_type", "weno_order", "char_decomp", "fwave", "tfluct_solver"))
    s = (pyclaw.SharpClawSolver1D if ndim == 1 else pyclaw.SharpClawSolver2D)()
    s.rp = pyclaw.CellRiemann(SETUP_BODY, 1, 1, ndim, params=[1.0], sharpclaw=True, **kw)
    s.mwaves = 1
    for k in range(ndim):       # (where there is a device setup() goes on to the ghost cells)
        s.bc_lower[k] = s.bc_upper[k] = s.aux_bc_lower[k] = s.aux_bc_upper[k] = pyclaw.BC.outflow
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def accepted(solver, solution):
    """setup() gets as far as the device: a solver, or the library's PCL_ENODEVICE from pcl_create_cellrp"""
    if _lib.lib().pcl_device_count() < 1:
        with pytest.raises(_lib.PclError) as e:
            solver.setup(solution)
        assert e.value.code == _lib.ENODEVICE, str(e.value)
    else:
        solver.setup(solution)
        solver._release()


@pytest.mark.parametrize("ndim", [1, 2])
def test_setup_compiles_for_the_solvers_own_reconstruction(ndim):
    for lim_type, weno_order in [(2, 5), (1, 5), (3, 5)]:
        s = sharp_solver(ndim, lim_type=lim_type, weno_order=weno_order)
        accepted(s, make_solution(ndim))
        assert sharp_of(s.rp._rp) == (lim_type, weno_order, 0)
    if ndim == 1:
        s = sharp_solver(1, char_decomp=1)
        accepted(s, make_solution(1))
        assert sharp_of(s.rp._rp) == (2, 5, 1)


def test_setup_says_why_it_refuses():
    # a classic solver with a solver object compiled for SharpClaw
    for cls, nd in [(pyclaw.ClawSolver1D, 1), (pyclaw.ClawSolver2D, 2)]:
        s = cls()
        s.rp = pyclaw.CellRiemann(SETUP_BODY, 1, 1, nd, sharpclaw=True)
        s.mwaves = 1
        with pytest.raises(NotImplementedError, match="sharpclaw=True"):
            s.setup(make_solution(nd))
    with pytest.raises(ValueError, match="transverse"):
        pyclaw.CellRiemann(SETUP_BODY, 1, 1, 2, transverse="", sharpclaw=True)
    # the form: solver.fwave and state.mcapa against the solver object, each way
    with pytest.raises(NotImplementedError, match="fwave = True"):
        sharp_solver(1, fwave=True).setup(make_solution(1))
    s = sharp_solver(1)
    s.rp.fwave = True
    with pytest.raises(ValueError, match="solver.fwave"):
        s.setup(make_solution(1))
    with pytest.raises(NotImplementedError, match="capacity function"):
        sharp_solver(2).setup(make_solution(2, maux=1, mcapa=0))
    with pytest.raises(ValueError, match="state.mcapa"):
        sharp_solver(2, capa=True).setup(make_solution(2, maux=1))
    # weno_order > 5 is a lim_type 2 reconstruction
    with pytest.raises(NotImplementedError, match="weno_order > 5"):
        sharp_solver(1, lim_type=1, weno_order=7).setup(make_solution(1))
    # char_decomp = 1: 1-D, wave form, order 5
    with pytest.raises(NotImplementedError, match="char_decomp=1"):
        sharp_solver(2, char_decomp=1).setup(make_solution(2))
    with pytest.raises(NotImplementedError, match="char_decomp=1"):
        sharp_solver(1, char_decomp=1, fwave=True).setup(make_solution(1))
    with pytest.raises(NotImplementedError, match="char_decomp=1"):
        sharp_solver(1, char_decomp=1, weno_order=7).setup(make_solution(1))
    with pytest.raises(NotImplementedError, match="char_decomp 2 / 3"):
        sharp_solver(1, char_decomp=2).setup(make_solution(1))
    with pytest.raises(NotImplementedError, match="tfluct_solver"):
        sharp_solver(1, tfluct_solver=True).setup(make_solution(1))
    # aux listed beyond state.maux, and without aux at all
    with pytest.raises(ValueError, match="state.maux = 1"):
        sharp_solver(1, aux=(1,)).setup(make_solution(1, maux=1))
    with pytest.raises(ValueError, match="state.aux is None"):
        sharp_solver(1, aux=(0,)).setup(make_solution(1))
    # sizes against the problem
    s = sharp_solver(1)
    s.mwaves = 2
    with pytest.raises(Exception, match="ndim/mwaves/meqn"):
        s.setup(make_solution(1))
    # the accepted forms get as far as the device
    s = sharp_solver(2, capa=True, aux=(1,))
    accepted(s, make_solution(2, maux=2, mcapa=0))
    s = sharp_solver(1)
    s.rp.fwave = True
    s.fwave = True
    accepted(s, make_solution(1))


def test_more_than_one_rank_is_refused(monkeypatch):
    from pyclaw_amd import parallel
    sol = make_solution(2)
    sol.states[0].decomp = object()         # only looked at as "decomposed"; the refusal comes before it is used
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        sharp_solver(2).setup(sol)


def test_the_keyword_trails_and_is_an_attribute():
    rp = pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 1, (), "", "user", (), None, False, False, True)
    assert rp.sharpclaw is True
    assert pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 1).sharpclaw is False
