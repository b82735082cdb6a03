"""
CPU: a user-written Riemann solver compiled WITH the one-kernel form of the dimension-split 2-D step
(pyclaw.CellRiemann(..., one_kernel=True), pcl_cellrp_compile_onek, pcl_cellrp_onek) as far as it goes
without a device: the run-time compile of step2ds_kernel around the restated solvers in every form and arithmetic mode, the
cache (a handle with the kernel is another entry than the same text without it, and every older call gives the handle
it always gave), and every refusal, each of which comes before the compiler.
"""
import ctypes as C

import pytest

import pyclaw_amd as pyclaw
from apps import problems, psystem
from pyclaw_amd import _lib

FWAVE, CAPA = 1, 2
NEVER = b"s[0] = 1.0; // never compiled (onek cpu test)"


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def onek_of(handle):
    has = C.c_int(-1)
    _lib.check(_lib.lib().pcl_cellrp_onek(handle, C.byref(has)))
    return has.value


def test_version():
    assert _lib.lib().pcl_version() >= 112


def test_compile_onek_is_its_own_cache_entry_and_a_larger_program():
    L = _lib.lib()
    body = (problems.ACOUSTICS_2D_RP + "// onek cpu test 0\n").encode()
    plain, psize = C.c_void_p(), C.c_long()
    assert L.pcl_cellrp_compile(body, b"", 3, 2, 2, 0, C.byref(plain), C.byref(psize)) == 0
    n0, h0 = stats()
    h, size = C.c_void_p(), C.c_long()
    assert L.pcl_cellrp_compile_onek(body, None, b"", 3, 2, 0, None, 0, 0, C.byref(h), C.byref(size)) == 0, last_error()
    assert stats() == (n0 + 1, h0)                  # compiled: another entry than the plain handle of the same text
    assert h.value is not None and h.value != plain.value
    assert onek_of(h) == 1 and onek_of(plain) == 0
    assert size.value > psize.value > 0
    # again: a cache hit, the same handle
    g, gsize = C.c_void_p(), C.c_long()
    assert L.pcl_cellrp_compile_onek(body, None, b"", 3, 2, 0, None, 0, 0, C.byref(g), C.byref(gsize)) == 0
    assert stats() == (n0 + 1, h0 + 1) and g.value == h.value and gsize.value == size.value
    # and the plain call still finds the plain handle
    assert L.pcl_cellrp_compile_form(body, None, b"", 3, 2, 2, 0, None, 0, 0, C.byref(g), C.byref(gsize)) == 0
    assert stats() == (n0 + 1, h0 + 2) and g.value == plain.value and gsize.value == psize.value
    # the query's own refusals
    has = C.c_int()
    assert L.pcl_cellrp_onek(None, C.byref(has)) == _lib.EINVAL
    assert L.pcl_cellrp_onek(h, None) == _lib.EINVAL


def test_handles_of_every_older_call_report_zero():
    L = _lib.lib()
    tag = "// onek cpu test 1\n"
    aux = (C.c_int * 2)(0, 1)
    h = C.c_void_p()
    calls = [
        lambda: L.pcl_cellrp_compile((problems.BURGERS_1D_RP + tag).encode(), b"", 1, 1, 1, 0, C.byref(h), None),
        lambda: L.pcl_cellrp_compile_aux((problems.VC_ACOUSTICS_2D_RP + tag).encode(), b"", 3, 2, 2, 0, aux, 2, C.byref(h), None),
        lambda: L.pcl_cellrp_compile_t((problems.ACOUSTICS_2D_RP + tag).encode(), problems.ACOUSTICS_2D_RPT.encode(), b"", 3, 2, 2,
                                       0, None, 0, C.byref(h), None),
        lambda: L.pcl_cellrp_compile_form((problems.ACOUSTICS_2D_RP + tag).encode(), None, b"", 3, 2, 2, 0, None, 0, CAPA,
                                          C.byref(h), None),
        lambda: L.pcl_cellrp_compile_sharp((problems.ACOUSTICS_2D_RP + tag).encode(), b"", 3, 2, 2, 0, None, 0, 0, 2, 5, 0,
                                           C.byref(h), None),
        lambda: L.pcl_cellrp_compile3((problems.ACOUSTICS_3D_RP + tag).encode(), b"", 4, 2, 0, None, 0, 0, C.byref(h), None),
    ]
    for k, call in enumerate(calls):
        assert call() == 0, (k, last_error())
        assert onek_of(h) == 0, k


# (body, transverse, meqn, mwaves, aux, keywords)
BODIES = {
    "acoustics": (problems.ACOUSTICS_2D_RP, None, 3, 2, (), {}),
    "acoustics_trans": (problems.ACOUSTICS_2D_RP, problems.ACOUSTICS_2D_RPT, 3, 2, (), {}),
    "acoustics_capa": (problems.ACOUSTICS_2D_RP, None, 3, 2, (), dict(capa=True)),
    "shallow": (problems.SHALLOW_2D_RP, None, 3, 3, (), {}),
    "burgers": (problems.BURGERS_2D_RP, None, 1, 1, (), {}),
    "scalars5": (problems.SCALARS_2D_RP, None, 5, 5, (), {}),
    "euler5": (problems.EULER_3D_RP, None, 5, 3, (), {}),
    "vc_acoustics": (problems.VC_ACOUSTICS_2D_RP, None, 3, 2, (0, 1), {}),
    "vc_acoustics_capa": (problems.VC_ACOUSTICS_2D_RP, None, 3, 2, (0, 1), dict(capa=True)),
    "psystem_fwave": (psystem.PSYSTEM_FWAVE_2D_RP, None, 3, 2, (0, 1, 2, 3), dict(fwave=True)),
    "psystem_fwave_capa": (psystem.PSYSTEM_FWAVE_2D_RP, None, 3, 2, (0, 1, 2, 3), dict(fwave=True, capa=True)),
}


# every body in 'exact'; the other two modes (other flags and another namespace around the same text) for one body of each
# kind: plain, aux with a capacity function, f-waves
CASES = [(name, "exact") for name in sorted(BODIES)] + [(name, math) for math in ("fast", "strict")
                                                         for name in ("acoustics", "vc_acoustics_capa", "psystem_fwave")]


@pytest.mark.parametrize("name,math", CASES)
def test_the_forms_an_aux_list_a_transverse_body_and_the_three_modes_compile(name, math):
    body, trans, meqn, mwaves, aux, kw = BODIES[name]
    rp = pyclaw.CellRiemann(body, meqn, mwaves, 2, aux=aux, transverse=trans, one_kernel=True, **kw).compile(math)
    assert rp.code_size > 0 and onek_of(rp._rp) == 1 and rp.one_kernel is True
    form = C.c_int(-1)
    _lib.check(_lib.lib().pcl_cellrp_form(rp._rp, C.byref(form)))
    assert form.value == (FWAVE if kw.get("fwave") else 0) | (CAPA if kw.get("capa") else 0)
    has, slices = C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.lib().pcl_cellrp_transverse(rp._rp, C.byref(has), C.byref(slices)))
    assert has.value == (1 if trans is not None else 0)


def test_each_form_with_the_kernel_is_its_own_entry():
    """(the body assigns neither wave nor fwave, so it compiles in every form)"""
    body = "// onek cpu test 2\ns[0] = p[0];\namdq[0] = dmin(p[0], 0.0) * (qr[0] - ql[0]);\napdq[0] = dmax(p[0], 0.0) * (qr[0] - ql[0]);\n"
    seen = set()
    for form in (0, FWAVE, CAPA, FWAVE | CAPA):
        for onek in (False, True):
            n0, h0 = stats()
            rp = pyclaw.CellRiemann(body, 1, 1, 2, fwave=bool(form & FWAVE), capa=bool(form & CAPA), one_kernel=onek).compile()
            assert stats() == (n0 + 1, h0), (form, onek)
            assert onek_of(rp._rp) == int(onek)
            seen.add(rp._rp.value)
    assert len(seen) == 8


def test_refusals_come_before_the_compiler():
    L = _lib.lib()
    h = C.c_void_p()
    n0, h0 = stats()
    # more than five equations: the rule of the one-kernel step for every solver
    for meqn in (6, 8):
        rc = L.pcl_cellrp_compile_onek(NEVER, None, b"", meqn, 1, 0, None, 0, 0, C.byref(h), None)
        assert rc == _lib.EINVAL and "pcl_cellrp_compile_onek" in last_error() and "meqn > 5" in last_error(), meqn
        assert h.value is None
    # what pcl_cellrp_compile_form refuses, in its words: a form bit outside the two, the two-pass tile's plane limit (it
    # lies inside the one-kernel tile's), the aux list, the sizes, the mode
    for bad in (4, 8, -1):
        rc = L.pcl_cellrp_compile_onek(NEVER, None, b"", 1, 1, 0, None, 0, bad, C.byref(h), None)
        assert rc == _lib.EINVAL and "form" in last_error(), bad
    aux = (C.c_int * 5)(0, 1, 2, 3, 4)
    rc = L.pcl_cellrp_compile_onek(NEVER, None, b"", 3, 1, 0, aux, 5, CAPA, C.byref(h), None)
    assert rc == _lib.EINVAL and "meqn + 1 + naux = 9" in last_error() and "at most 8" in last_error()
    rc = L.pcl_cellrp_compile_onek(NEVER, None, b"", 4, 1, 0, aux, 5, 0, C.byref(h), None)
    assert rc == _lib.EINVAL and "meqn + naux = 9" in last_error()
    twice = (C.c_int * 2)(1, 1)
    assert L.pcl_cellrp_compile_onek(NEVER, None, b"", 3, 1, 0, twice, 2, 0, C.byref(h), None) == _lib.EINVAL
    assert "listed twice" in last_error()
    assert L.pcl_cellrp_compile_onek(NEVER, None, b"", 3, 1, 0, None, 2, 0, C.byref(h), None) == _lib.EINVAL
    assert L.pcl_cellrp_compile_onek(NEVER, None, b"", 0, 1, 0, None, 0, 0, C.byref(h), None) == _lib.EINVAL
    assert L.pcl_cellrp_compile_onek(NEVER, None, b"", 3, 9, 0, None, 0, 0, C.byref(h), None) == _lib.EINVAL
    assert L.pcl_cellrp_compile_onek(NEVER, None, b"", 3, 2, 7, None, 0, 0, C.byref(h), None) == _lib.EINVAL
    assert "math" in last_error()
    assert L.pcl_cellrp_compile_onek(None, None, b"", 3, 2, 0, None, 0, 0, C.byref(h), None) == _lib.EINVAL
    assert L.pcl_cellrp_compile_onek(NEVER, None, b"", 3, 2, 0, None, 0, 0, None, None) == _lib.EINVAL
    assert stats() == (n0, h0)
    # the keyword's refusals, each with its reason, before anything is compiled
    with pytest.raises(ValueError, match="ndim must be 2"):
        pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 1, one_kernel=True)
    with pytest.raises(ValueError, match="sharpclaw=True"):
        pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 2, sharpclaw=True, one_kernel=True)
    with pytest.raises(ValueError, match=r"meqn > 5"):
        pyclaw.CellRiemann("s[0] = 1.0;", 6, 1, 2, one_kernel=True)
    with pytest.raises(ValueError):            # ndim = 3 is a CellRiemann3D, which has no such keyword
        pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 3, one_kernel=True)
    with pytest.raises(TypeError):
        pyclaw.CellRiemann3D("s[0] = 1.0;", 1, 1, one_kernel=True)
    assert stats() == (n0, h0)


def test_the_keyword_assigned_after_construction_is_checked_at_compile():
    n0, h0 = stats()
    rp = pyclaw.CellRiemann("s[0] = 1.0; // onek cpu test late", 1, 1, 1)
    rp.one_kernel = True
    with pytest.raises(ValueError, match="ndim must be 2"):
        rp.compile()
    rp = pyclaw.CellRiemann("s[0] = 1.0; // onek cpu test late", 1, 1, 2, sharpclaw=True)
    rp.one_kernel = True
    with pytest.raises(ValueError, match="sharpclaw=True"):
        rp.compile(sharp=(2, 5, 0))
    rp = pyclaw.CellRiemann("s[0] = 1.0; // onek cpu test late", 6, 1, 2)
    rp.one_kernel = True
    with pytest.raises(ValueError, match="meqn > 5"):
        rp.compile()
    rp = pyclaw.CellRiemann3D("s[0] = 1.0; // onek cpu test late", 1, 1)
    rp.one_kernel = True
    with pytest.raises(ValueError, match="ndim must be 2"):
        rp.compile()
    assert stats() == (n0, h0)


def test_a_diagnostic_of_the_body_keeps_its_line():
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann("s[0] = 1.0;\n\nnot_declared = 2.0;\n", 1, 1, 2, one_kernel=True).compile()
    assert "riemann:3:" in str(e.value) and "not_declared" in str(e.value)


def test_the_keyword_is_part_of_the_key_an_attribute_and_off_by_default():
    body = problems.ACOUSTICS_2D_RP + "// onek cpu test 3\n"
    rp = pyclaw.CellRiemann(body, 3, 2, 2)
    assert rp.one_kernel is False
    # the default compiles today's handle: the one pcl_cellrp_compile gives for the text
    h = C.c_void_p()
    assert _lib.lib().pcl_cellrp_compile(body.encode(), b"", 3, 2, 2, 0, C.byref(h), None) == 0
    rp.compile()
    assert rp._rp.value == h.value and onek_of(rp._rp) == 0
    first, key0 = rp._rp.value, rp._key
    # the same object recompiles when the keyword changes
    rp.one_kernel = True
    rp.compile()
    assert rp._key != key0 and rp._rp.value != first and onek_of(rp._rp) == 1
    assert pyclaw.CellRiemann(body, 3, 2, 2, one_kernel=True).one_kernel is True
    # trailing keyword: the positional order of the older ones is untouched
    rp = pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 2, (), "", "user", (), None, False, False, False, True)
    assert rp.one_kernel is True and rp.sharpclaw is False


def test_an_unsplit_solver_keeps_its_kernels_next_to_the_extra_one():
    """a transverse body and one_kernel=True: five kernels in one module; the unsplit configuration takes the handle"""
    L = _lib.lib()
    rp = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP + "// onek cpu test 4\n", 3, 2, 2, transverse=problems.ACOUSTICS_2D_RPT,
                            one_kernel=True).compile()
    plain = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP + "// onek cpu test 4\n", 3, 2, 2,
                               transverse=problems.ACOUSTICS_2D_RPT).compile()
    assert rp.code_size > plain.code_size
    for unsplit in (False, True):
        cfg = _lib.Config()
        cfg.ndim = 2
        for k in range(2):
            cfg.n[k], cfg.d[k] = 8, 0.1
        cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, 3, 2, 0
        for k, v in enumerate([1, 2, 2 if unsplit else -1, 0, 0, 0, 0]):
            cfg.method[k] = v
        cfg.mthlim[0] = cfg.mthlim[1] = 4
        cfg.rp = 100
        s = C.c_void_p()
        rc = L.pcl_create_cellrp(C.byref(cfg), rp._rp, C.byref(s))
        assert rc == (_lib.ENODEVICE if L.pcl_device_count() < 1 else _lib.OK), last_error()
        if rc == _lib.OK:
            L.pcl_destroy(s)
