"""
CPU: user-written Riemann solvers in the UNSPLIT 3-D step (pyclaw.CellRiemann3D(..., rpt3=..., rptt3=...),
pcl_cellrp_compile3t) as far as they go without a device -- the run-time compile of the pieces kernels of
the general unsplit step (csrc/classic3.hpp) around the three texts, the cache, the diagnostics, every refusal of the
compile call, of pcl_create_cellrp and of the Python surface (each comes before any device call: a machine without a GPU
answers ENODEVICE once the argument checks are through), and the scratch-size rule.
"""
import ctypes as C

import pytest

import pyclaw_amd as pyclaw
from apps import problems
from pyclaw_amd import _lib

PCL_RP_CELL = 100
FWAVE, CAPA = 1, 2
MODES = ["exact", "fast", "strict"]
BODIES = {"vc_acoustics": ("VC_ACOUSTICS_3D", 4, 2, (0, 1)), "acoustics": ("ACOUSTICS_3D", 4, 2, ()),
          "advection": ("ADVECTION_3D", 1, 1, ()), "euler": ("EULER_3D", 5, 3, ())}
TINY = "wave[0][0] = qr[0] - ql[0];\ns[0] = p[ixy - 1];\namdq[0] = dmin(s[0], 0.0) * wave[0][0];\n" \
       "apdq[0] = dmax(s[0], 0.0) * wave[0][0];\n// unsplit 3-D cpu test\n"
TINY_T = "bmasdq[0] = dmin(p[(ixyz + icoor - 2) % 3], 0.0) * asdq[0];\nbpasdq[0] = dmax(p[(ixyz + icoor - 2) % 3], 0.0) * asdq[0];\n"
TINY_TT = "cmbsasdq[0] = dmin(p[(ixyz + icoor - 2) % 3], 0.0) * bsasdq[0];\ncpbsasdq[0] = dmax(p[(ixyz + icoor - 2) % 3], 0.0) * bsasdq[0];\n"


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def enc(text):
    return None if text is None else text.encode()


def compile3t(body, rpt3, rptt3, meqn, mwaves, aux=(), form=0, math=0):
    h, size = C.c_void_p(), C.c_long()
    rc = _lib.lib().pcl_cellrp_compile3t(enc(body), enc(rpt3), enc(rptt3), b"", meqn, mwaves, math,
                                         (C.c_int * len(aux))(*aux) if aux else None, len(aux), form, C.byref(h), C.byref(size))
    return rc, h, size.value


def trans3_of(h):
    t = C.c_int(-1)
    _lib.check(_lib.lib().pcl_cellrp_transverse3(h, C.byref(t)))
    return t.value


def texts(name):
    stem, meqn, mwaves, aux = BODIES[name]
    return (getattr(problems, stem + "_RP"), getattr(problems, stem + "_RPT"), getattr(problems, stem + "_RPTT"), meqn, mwaves, aux)


# ---- the compile call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", MODES)
@pytest.mark.parametrize("name", sorted(BODIES))
def test_every_text_compiles_in_every_mode_and_the_handle_reports_trans3(name, math):
    body, rpt3, rptt3, meqn, mwaves, aux = texts(name)
    rp = pyclaw.CellRiemann3D(body, meqn, mwaves, aux=aux, rpt3=rpt3, rptt3=rptt3).compile(math)
    assert rp.code_size > 0 and rp.ndim == 3 and rp.has_transverse
    assert _lib.lib().pcl_cellrp_check(rp._rp, meqn, mwaves, 3, MODES.index(math)) == 0
    assert trans3_of(rp._rp) == 2
    rp1 = pyclaw.CellRiemann3D(body, meqn, mwaves, aux=aux, rpt3=rpt3).compile(math)
    assert trans3_of(rp1._rp) == 1 and rp1._rp.value != rp._rp.value
    rp0 = pyclaw.CellRiemann3D(body, meqn, mwaves, aux=aux).compile(math)
    assert trans3_of(rp0._rp) == 0 and rp0._rp.value not in (rp._rp.value, rp1._rp.value)


def test_the_same_texts_compile_once_and_each_text_is_part_of_the_key():
    assert _lib.lib().pcl_version() >= 113
    n0, h0 = stats()
    rc, h, size = compile3t(TINY, TINY_T + "// once\n", TINY_TT, 1, 1)
    assert rc == 0 and size > 0, last_error()
    assert stats() == (n0 + 1, h0)
    rc, h2, size2 = compile3t(TINY, TINY_T + "// once\n", TINY_TT, 1, 1)
    assert rc == 0 and h2.value == h.value and size2 == size and stats() == (n0 + 1, h0 + 1)
    rc, h3, _ = compile3t(TINY, TINY_T + "// once\n", TINY_TT + "// other\n", 1, 1)
    assert rc == 0 and h3.value != h.value and stats() == (n0 + 2, h0 + 1)
    rc, h4, _ = compile3t(TINY, TINY_T + "// other\n", TINY_TT, 1, 1)
    assert rc == 0 and h4.value not in (h.value, h3.value) and stats() == (n0 + 3, h0 + 1)
    # without the texts: pcl_cellrp_compile3 itself, the same handle
    rc, h5, _ = compile3t(TINY, None, None, 1, 1)
    h6, size6 = C.c_void_p(), C.c_long()
    assert rc == 0 and _lib.lib().pcl_cellrp_compile3(TINY.encode(), b"", 1, 1, 0, None, 0, 0, C.byref(h6), C.byref(size6)) == 0
    assert h6.value == h5.value and trans3_of(h5) == 0


def test_eight_equations_and_eight_waves_compile():
    """more planes than the tile of the dimension-split sweeps holds: such a handle serves the unsplit step alone"""
    body = "for (int m = 0; m < 8; m++) { wave[m][m] = qr[m] - ql[m]; s[m] = p[0]; apdq[m] = p[0] * wave[m][m]; }\n"
    rpt3 = "for (int m = 0; m < 8; m++) bpasdq[m] = p[1] * asdq[m];\n"
    rptt3 = "for (int m = 0; m < 8; m++) cpbsasdq[m] = p[1] * bsasdq[m];\n"
    rc, h, size = compile3t(body, rpt3, rptt3, 8, 8)
    assert rc == 0 and size > 0 and trans3_of(h) == 2, last_error()
    assert create(cell_config(meqn=8, mwaves=8, maux=0, order_trans=22), h) in (0, _lib.ENODEVICE), last_error()
    assert create(cell_config(meqn=8, mwaves=8, maux=0), h) == _lib.EINVAL
    assert "unsplit step alone" in last_error()
    with pytest.raises(ValueError, match="at most 7 planes"):
        pyclaw.CellRiemann3D(body, 8, 8)


def test_diagnostics_carry_the_texts_own_lines():
    rc, h, _ = compile3t(TINY, "bmasdq[0] = 0.0;\nbpasdq[0] = no_such_name;\n", TINY_TT, 1, 1)
    assert rc == _lib.EINVAL and "no_such_name" in last_error() and "rpt3:2" in last_error()
    rc, h, _ = compile3t(TINY, TINY_T, "\n\ncmbsasdq[0] = 0.0 +;\n", 1, 1)
    assert rc == _lib.EINVAL and "rptt3:3" in last_error()
    # no imp without an aux list: the pair of cells is the same for both sides
    rc, h, _ = compile3t(TINY, "bmasdq[0] = imp * asdq[0];\n", None, 1, 1)
    assert rc == _lib.EINVAL and "undeclared" in last_error() and "imp" in last_error() and "rpt3:1" in last_error()
    # with one: imp, q1 and auxb, and no cells
    rc, h, _ = compile3t(TINY, "bmasdq[0] = imp * q1[0] * auxb[0][2][0] * asdq[0];\n",
                         "cmbsasdq[0] = impt * imp * auxb[2][0][0] * bsasdq[0];\n", 1, 1, aux=(1,))
    assert rc == 0, last_error()
    rc, h, _ = compile3t(TINY, "bmasdq[0] = ql[0] * asdq[0];\n", None, 1, 1, aux=(1,))
    assert rc == _lib.EINVAL and "undeclared" in last_error() and "ql" in last_error()
    # every direction and both splits are instantiated
    rc, h, _ = compile3t(TINY, 'static_assert(!(ixyz == 3 && icoor == 3), "z sweep, z-like split");\n', None, 1, 1)
    assert rc == _lib.EINVAL and "z sweep, z-like split" in last_error()
    rc, h, _ = compile3t(TINY, 'static_assert(ixy == ixyz && ixyz >= 1 && ixyz <= 3 && (icoor == 2 || icoor == 3), "");\n',
                         'static_assert(ixy == ixyz && (icoor == 2 || icoor == 3), "");\n', 1, 1)
    assert rc == 0, last_error()


def test_the_compile_call_refuses_with_the_reason():
    n0, h0 = stats()
    rc, h, _ = compile3t(TINY, None, TINY_TT, 1, 1)
    assert rc == _lib.EINVAL and "rptt3 body without an rpt3" in last_error()
    for form in (FWAVE, FWAVE | CAPA):
        rc, h, _ = compile3t(TINY, TINY_T, TINY_TT, 1, 1, form=form)
        assert rc == _lib.EINVAL and "f-wave" in last_error()
    rc, h, _ = compile3t(TINY, TINY_T, TINY_TT, 1, 1, aux=(0,), form=CAPA)
    assert rc == _lib.EINVAL and "capacity function" in last_error() and "PCL_CELLRP_FORM_CAPA" in last_error()
    rc, h, _ = compile3t(None, TINY_T, TINY_TT, 1, 1)
    assert rc == _lib.EINVAL
    assert stats() == (n0, h0)
    # the 2-D call keeps refusing ndim == 3
    hh = C.c_void_p()
    assert _lib.lib().pcl_cellrp_compile_t(TINY.encode(), TINY_T.encode(), b"", 1, 1, 3, 0, None, 0, C.byref(hh), None) == _lib.EINVAL
    assert "ndim must be 2" in last_error()


# ---- pcl_create_cellrp ----------------------------------------------------------------------------------------------------
def cell_config(ndim=3, meqn=4, mwaves=2, maux=2, **over):
    cfg = _lib.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, meqn, mwaves, maux
    for k, v in enumerate([1, 2, -1, 0, 0, 0, maux]):
        cfg.method[k] = v
    cfg.mthlim[0] = cfg.mthlim[1] = 4
    cfg.rp = PCL_RP_CELL
    for k, v in over.items():
        if k == "mcapa":
            cfg.method[5] = v
        elif k == "order_trans":
            cfg.method[2] = v
        else:
            setattr(cfg, k, v)
    return cfg


def create(cfg, handle):
    s = C.c_void_p()
    rc = _lib.lib().pcl_create_cellrp(C.byref(cfg), handle, C.byref(s))
    if rc == 0:
        _lib.lib().pcl_destroy(s)
    return rc


@pytest.fixture(scope="module")
def handles():
    body, rpt3, rptt3, meqn, mwaves, aux = texts("vc_acoustics")
    out = {"both": pyclaw.CellRiemann3D(body, meqn, mwaves, aux=aux, rpt3=rpt3, rptt3=rptt3).compile(),
           "rpt3": pyclaw.CellRiemann3D(body, meqn, mwaves, aux=aux, rpt3=rpt3).compile(),
           "none": pyclaw.CellRiemann3D(body, meqn, mwaves, aux=aux).compile()}
    yield out
    for rp in out.values():
        rp.release()


@pytest.mark.parametrize("which,trans", [("both", t) for t in (0, 10, 11, 20, 21, 22, -1)] + [("rpt3", t) for t in (0, 10, 20, -1)])
def test_the_transverse_modes_a_handle_serves_pass_the_argument_checks(handles, which, trans):
    """OK on a machine with a device, ENODEVICE without one: not EINVAL"""
    assert create(cell_config(order_trans=trans), handles[which]._rp) in (0, _lib.ENODEVICE), last_error()


@pytest.mark.parametrize("which,over,words", [
    ("both", dict(order_trans=12), ["method[2] = 12", "0, 10, 11, 20, 21 or 22"]),
    ("both", dict(order_trans=30), ["method[2] = 30", "0, 10, 11, 20, 21 or 22"]),
    ("both", dict(order_trans=23), ["method[2] = 23", "0, 10, 11, 20, 21 or 22"]),
    ("both", dict(order_trans=1), ["method[2] = 1", "0, 10, 11, 20, 21 or 22"]),
    ("rpt3", dict(order_trans=11), ["method[2] = 11", "rptt3"]),
    ("rpt3", dict(order_trans=21), ["method[2] = 21", "rptt3"]),
    ("rpt3", dict(order_trans=22), ["method[2] = 22", "rptt3"]),
    ("both", dict(order_trans=22, mbc=3), ["mbc == 2"]),
    ("both", dict(order_trans=22, fwave=1), ["f-waves", "3-D"]),
    ("both", dict(order_trans=22, maux=3, mcapa=3), ["capacity function"]),
    ("none", dict(order_trans=0), ["rpt3", "rptt3", "method[2]"]),
    ("none", dict(order_trans=22), ["rpt3", "rptt3", "method[2]"]),
])
def test_pcl_create_cellrp_refuses_with_the_reason(handles, which, over, words):
    """EINVAL from the host-only checks, not ENODEVICE"""
    rc = create(cell_config(**over), handles[which]._rp)
    assert rc == _lib.EINVAL, (rc, last_error())
    for w in words:
        assert w in last_error(), (w, last_error())


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def make_solution(maux=0):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xyz"]
    state = pyclaw.State(pyclaw.Grid(dims), 1, maux)
    state.q[...] = 1.0
    if maux:
        state.aux[...] = 1.0
    return pyclaw.Solution(state)


def solver3(order_trans=22, dim_split=False, **kw):
    s = pyclaw.ClawSolver3D()
    s.rp = pyclaw.CellRiemann3D(TINY, 1, 1, params=[1.0, 0.5, 0.25], **kw)
    s.mwaves = 1
    s.limiters = 4
    s.dim_split = dim_split
    s.order_trans = order_trans
    return s


def accepted(solver, solution):
    """setup() up to the device: on a machine without one the library answers ENODEVICE behind every argument check"""
    try:
        solver.setup(solution)
    except _lib.PclError as e:
        assert e.code == _lib.ENODEVICE, e
    else:
        solver.teardown()


def test_the_python_surface():
    with pytest.raises(ValueError, match="rptt3 without rpt3"):
        pyclaw.CellRiemann3D(TINY, 1, 1, rptt3=TINY_TT)
    with pytest.raises(ValueError, match="capa=True with rpt3"):
        pyclaw.CellRiemann3D(TINY, 1, 1, aux=(0,), capa=True, rpt3=TINY_T)
    for trans in (0, 10, 11, 20, 21, 22):
        s = solver3(trans, rpt3=TINY_T, rptt3=TINY_TT)
        accepted(s, make_solution())
        assert s.method[2] == trans
    for trans in (0, 10, 20):
        accepted(solver3(trans, rpt3=TINY_T), make_solution())
    for trans in (11, 21, 22):
        with pytest.raises(NotImplementedError, match="rptt3"):
            solver3(trans, rpt3=TINY_T).setup(make_solution())
    with pytest.raises(ValueError, match="order_trans"):
        solver3(12, rpt3=TINY_T, rptt3=TINY_TT).setup(make_solution())
    # without the texts: the old refusal, which now names the keywords
    with pytest.raises(NotImplementedError, match="rpt3=") as e:
        solver3().setup(make_solution())
    assert "rptt3=" in str(e.value)
    # a handle with the texts still serves the dimension-split step
    s = solver3(dim_split=True, rpt3=TINY_T, rptt3=TINY_TT)
    accepted(s, make_solution())
    assert s.method[2] == -1
    # the aux form of the texts through the solver
    accepted(solver3(10, aux=(1,), rpt3="bmasdq[0] = imp * auxb[1][1][0] * asdq[0];\n"), make_solution(maux=2))
    with pytest.raises(ValueError, match="aux component 2"):
        solver3(10, aux=(2,), rpt3="bmasdq[0] = auxb[1][1][0] * asdq[0];\n").setup(make_solution(maux=2))


# ---- the scratch-size rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meqn,n", [(4, (30, 30, 30)), (5, (7, 6, 5)), (4, (256, 256, 256))])
def test_the_scratch_size_rule(meqn, n):
    want = 14 * meqn * (n[0] + 4) * (n[1] + 4) * (n[2] + 4) * 8
    assert _lib.lib().pcl_unsplit3_scratch_bytes(meqn, n[0], n[1], n[2], 2) == want
    assert _lib.lib().pcl_unsplit3_scratch_live() >= 0
