"""
CPU: the FORM of a user-written Riemann solver -- f-waves and a capacity function (pyclaw.CellRiemann(..., fwave=...,
capa=...), pcl_cellrp_compile_form, pcl_cellrp_form, pcl_create_cellrp) -- as far as it goes without a
device: the run-time compile of every new body in the three arithmetic modes, form 0 as the entry it extends, the cache,
the diagnostics, and every refusal, each of which comes before the compiler or before any device call.
"""
import ctypes as C

import pytest

import pyclaw_amd as pyclaw
from apps import problems, psystem
from pyclaw_amd import _lib

PCL_RP_CELL = 100
FWAVE, CAPA = 1, 2


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def form_of(rp):
    f = C.c_int(-1)
    _lib.check(_lib.lib().pcl_cellrp_form(rp._rp, C.byref(f)))
    return f.value


# (body, transverse, meqn, mwaves, ndim, aux, keywords)
NEW_BODIES = {
    "elasticity": (problems.ELASTICITY_FWAVE_1D_RP, None, 2, 2, 1, (0, 1, 2), dict(fwave=True)),
    "vc_advection": (problems.VC_ADVECTION_FWAVE_1D_RP, None, 1, 1, 1, (0,), dict(fwave=True)),
    "vc_advection_capa": (problems.VC_ADVECTION_FWAVE_1D_RP, None, 1, 1, 1, (0,), dict(fwave=True, capa=True)),
    "shallow_bathy": (problems.SHALLOW_BATHY_FWAVE_1D_RP, None, 2, 2, 1, (0,), dict(fwave=True)),
    "psystem": (psystem.PSYSTEM_FWAVE_2D_RP, None, 3, 2, 2, (0, 1, 2, 3), dict(fwave=True)),
    "psystem_unsplit_capa": (psystem.PSYSTEM_FWAVE_2D_RP, psystem.PSYSTEM_FWAVE_2D_RPT, 3, 2, 2, (0, 1, 2, 3),
                             dict(fwave=True, capa=True)),
}


@pytest.mark.parametrize("math", ["exact", "fast", "strict"])
@pytest.mark.parametrize("name", sorted(NEW_BODIES))
def test_every_new_body_compiles_in_the_three_modes(name, math):
    body, trans, meqn, mwaves, ndim, aux, kw = NEW_BODIES[name]
    rp = pyclaw.CellRiemann(body, meqn, mwaves, ndim, aux=aux, transverse=trans, **kw).compile(math)
    assert rp.code_size > 0
    assert form_of(rp) == (FWAVE if kw.get("fwave") else 0) | (CAPA if kw.get("capa") else 0)
    assert rp.fwave == bool(kw.get("fwave")) and rp.capa == bool(kw.get("capa"))


def test_form_zero_is_the_entry_it_extends():
    L = _lib.lib()
    tag = "// form cpu test 0\n"
    body, trans = (problems.ACOUSTICS_2D_RP + tag).encode(), problems.ACOUSTICS_2D_RPT.encode()
    h, size = C.c_void_p(), C.c_long()
    assert L.pcl_cellrp_compile_t(body, trans, b"", 3, 2, 2, 0, None, 0, C.byref(h), C.byref(size)) == 0
    n0, h0 = stats()
    g, gsize = C.c_void_p(), C.c_long()
    assert L.pcl_cellrp_compile_form(body, trans, b"", 3, 2, 2, 0, None, 0, 0, C.byref(g), C.byref(gsize)) == 0
    assert g.value == h.value and gsize.value == size.value
    assert stats() == (n0, h0 + 1)           # the same object: the compile counter has not moved
    f = C.c_int(-1)
    assert L.pcl_cellrp_form(g, C.byref(f)) == 0 and f.value == 0
    # without a transverse text either
    assert L.pcl_cellrp_compile(body, b"", 3, 2, 2, 0, C.byref(h), C.byref(size)) == 0
    n1, h1 = stats()
    assert L.pcl_cellrp_compile_form(body, None, b"", 3, 2, 2, 0, None, 0, 0, C.byref(g), C.byref(gsize)) == 0
    assert g.value == h.value and gsize.value == size.value and stats() == (n1, h1 + 1)
    assert L.pcl_cellrp_form(None, C.byref(f)) == _lib.EINVAL
    assert L.pcl_cellrp_form(g, None) == _lib.EINVAL


def test_each_form_is_its_own_cache_entry():
    """One text, four forms: four programs.  (The body assigns neither wave nor fwave, so it compiles in every form.)"""
    tag = "// form cpu test 1\n"
    body = tag + "s[0] = p[0];\namdq[0] = dmin(p[0], 0.0) * (qr[0] - ql[0]);\napdq[0] = dmax(p[0], 0.0) * (qr[0] - ql[0]);\n"
    seen = {}
    for form in (0, FWAVE, CAPA, FWAVE | CAPA):
        n0, h0 = stats()
        rp = pyclaw.CellRiemann(body, 1, 1, 2, fwave=bool(form & FWAVE), capa=bool(form & CAPA)).compile()
        assert stats() == (n0 + 1, h0), form
        assert form_of(rp) == form
        again = pyclaw.CellRiemann(body, 1, 1, 2, fwave=bool(form & FWAVE), capa=bool(form & CAPA)).compile()
        assert stats() == (n0 + 1, h0 + 1) and again._rp.value == rp._rp.value
        seen[form] = rp
    assert len(set(rp._rp.value for rp in seen.values())) == 4
    # the same CellRiemann object recompiles when its form changes: the form is part of its key
    rp = seen[0]
    first = rp._rp.value
    rp.fwave = True
    rp.compile()
    assert rp._rp.value == seen[FWAVE]._rp.value != first


def test_an_fwave_body_that_assigns_wave_gets_its_line():
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann("s[0] = 1.0;\n\nwave[0][0] = qr[0] - ql[0];\n", 1, 1, 1, fwave=True).compile()
    assert "riemann:3:" in str(e.value) and "wave" in str(e.value)
    # and the other way round
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann("s[0] = 1.0;\nfwave[0][0] = qr[0] - ql[0];\n", 1, 1, 1).compile()
    assert "riemann:2:" in str(e.value) and "fwave" in str(e.value)


def test_refusals_come_before_the_compiler():
    L = _lib.lib()
    h = C.c_void_p()
    n0, h0 = stats()
    for bad in (4, 8, 7, -1):
        rc = L.pcl_cellrp_compile_form(b"s[0] = 1.0; // never compiled", None, b"", 1, 1, 1, 0, None, 0, bad, C.byref(h), None)
        assert rc == _lib.EINVAL and "form" in last_error() and h.value is None, bad
    # meqn + 1 + naux = 9 with a capacity function; the same list without one is 8 and compiles
    aux = (C.c_int * 5)(0, 1, 2, 3, 4)
    rc = L.pcl_cellrp_compile_form(b"s[0] = 1.0; // never compiled", None, b"", 3, 1, 2, 0, aux, 5, CAPA, C.byref(h), None)
    assert rc == _lib.EINVAL and "meqn + 1 + naux = 9" in last_error() and "at most 8" in last_error()
    assert stats() == (n0, h0)
    with pytest.raises(ValueError, match=r"meqn \+ 1 \+ len\(aux\) = 9"):
        pyclaw.CellRiemann("s[0] = 1.0;", 3, 1, 2, aux=(0, 1, 2, 3, 4), capa=True)
    assert stats() == (n0, h0)
    rp = pyclaw.CellRiemann("s[0] = 1.0; // form cpu test planes", 3, 1, 2, aux=(0, 1, 2, 3), capa=True).compile()   # 8
    assert form_of(rp) == CAPA


def cell_config(ndim, meqn, mwaves, maux, fwave=0, mcapa=0, unsplit=False):
    cfg = _lib.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, meqn, mwaves, maux
    for k, v in enumerate([1, 2, 2 if unsplit else -1, 0, 0, mcapa, maux]):
        cfg.method[k] = v
    for k in range(mwaves):
        cfg.mthlim[k] = 4
    cfg.fwave = fwave
    cfg.rp = PCL_RP_CELL
    for k, v in enumerate([1.0, 4.0, 2.0, 2.0]):
        cfg.rp_params[k] = v
    return cfg


@pytest.fixture(scope="module")
def four_forms():
    """ACOUSTICS_2D-sized handles (3 equations, 2 waves, 2-D, with a transverse body) of the four forms; the body assigns
    neither array."""
    body = "// form cpu test 2\ns[0] = -p[2]; s[1] = p[2];\n"
    return dict((form, pyclaw.CellRiemann(body, 3, 2, 2, transverse="", fwave=bool(form & FWAVE),
                                          capa=bool(form & CAPA)).compile())
                for form in (0, FWAVE, CAPA, FWAVE | CAPA))


@pytest.mark.parametrize("unsplit", [False, True])
@pytest.mark.parametrize("want", [0, FWAVE, CAPA, FWAVE | CAPA])
@pytest.mark.parametrize("have", [0, FWAVE, CAPA, FWAVE | CAPA])
def test_pcl_create_cellrp_takes_the_form_of_the_handle_and_no_other(four_forms, have, want, unsplit):
    L = _lib.lib()
    cfg = cell_config(2, 3, 2, 2, fwave=1 if want & FWAVE else 0, mcapa=2 if want & CAPA else 0, unsplit=unsplit)
    s = C.c_void_p()
    rc = L.pcl_create_cellrp(C.byref(cfg), four_forms[have]._rp, C.byref(s))
    if have == want:
        # the argument checks are through: no device, or a solver
        assert rc == (_lib.ENODEVICE if L.pcl_device_count() < 1 else _lib.OK), last_error()
        if rc == _lib.OK:
            L.pcl_destroy(s)
        return
    assert rc == _lib.EINVAL and "PCL_RP_CELL" in last_error()
    if (have ^ want) & FWAVE:           # the f-wave bit is looked at first
        assert "f-waves" in last_error()
    else:
        assert "capacity function" in last_error()
    # pcl_create cannot know a handle: its refusals, in its words
    if want:
        assert L.pcl_create(C.byref(cfg), C.byref(s)) == _lib.EINVAL and "PCL_RP_CELL" in last_error()
        assert ("f-waves" if want & FWAVE else "capacity function") in last_error()


def test_mcapa_stays_within_maux(four_forms):
    s = C.c_void_p()
    cfg = cell_config(2, 3, 2, 2, mcapa=3)
    assert _lib.lib().pcl_create_cellrp(C.byref(cfg), four_forms[CAPA]._rp, C.byref(s)) == _lib.EINVAL
    assert "mcapa out of range" in last_error()


# ---- setup(): every row of the table -------------------------------------------------------------------------------

def make_solution(ndim, mcapa=None, maux=1):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xyz"[:ndim]]
    state = pyclaw.State(pyclaw.Grid(dims), 1, maux)
    state.q[...] = 1.0
    state.aux[...] = 1.0
    if mcapa is not None:
        state.mcapa = mcapa
    return pyclaw.Solution(state)


SETUP_BODY = "// form cpu test 3\ns[0] = auxr[0];\n"


def user_solver(ndim, solver_fwave, **kw):
    s = (pyclaw.ClawSolver1D if ndim == 1 else pyclaw.ClawSolver2D)()
    s.rp = pyclaw.CellRiemann(SETUP_BODY, 1, 1, ndim, aux=(0,), **kw)
    s.mwaves = 1
    s.fwave = solver_fwave
    if ndim == 2:
        s.dim_split = True
    return s


def accepted(solver, solution):
    """setup() gets as far as the device: a solver, or on a machine without one the library's PCL_ENODEVICE from
    pcl_create_cellrp -- every check of the table is through either way."""
    if _lib.lib().pcl_device_count() < 1:
        with pytest.raises(_lib.PclError) as e:
            solver.setup(solution)
        assert e.value.code == _lib.ENODEVICE, str(e.value)
    else:
        solver.setup(solution)
        solver._release()


@pytest.mark.parametrize("ndim", [1, 2])
def test_setup_table(ndim):
    # solver.fwave = True
    accepted(user_solver(ndim, True, fwave=True), make_solution(ndim))
    with pytest.raises(NotImplementedError, match="fwave = True"):
        user_solver(ndim, True).setup(make_solution(ndim))
    with pytest.raises(ValueError, match="fwave") as e:
        user_solver(ndim, False, fwave=True).setup(make_solution(ndim))
    assert "fwave=True" in str(e.value) and "solver.fwave" in str(e.value)      # names both
    # state.mcapa
    accepted(user_solver(ndim, False, capa=True), make_solution(ndim, mcapa=1, maux=2))
    with pytest.raises(NotImplementedError, match="capacity function"):
        user_solver(ndim, False).setup(make_solution(ndim, mcapa=1, maux=2))
    with pytest.raises(ValueError, match="capa") as e:
        user_solver(ndim, False, capa=True).setup(make_solution(ndim, maux=2))
    assert "capa=True" in str(e.value) and "state.mcapa" in str(e.value)
    # both at once
    accepted(user_solver(ndim, True, fwave=True, capa=True), make_solution(ndim, mcapa=1, maux=2))


def test_the_keywords_trail_and_are_attributes():
    rp = pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 1, (), "", "user", (), None, True, True)
    assert rp.fwave is True and rp.capa is True
    rp = pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 1)
    assert rp.fwave is False and rp.capa is False


def test_version():
    assert _lib.lib().pcl_version() >= 109
