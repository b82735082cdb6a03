"""
CPU: SharpClaw in 3-D (pyclaw.SharpClawSolver3D over pyclaw.SharpCellRiemann3D, pcl_cellrp_compile3_sharp) as
far as it goes without a device -- the numpy reference the device is held to (tests/sharp3_reference.py) against the frozen
oracle in two dimensions, the run-time compile of the three passes of sharp3_kernel around a body, the cache, and every
refusal of the compile call, of pcl_create_cellrp and of the Python surface, each of which comes before any device call (a
machine without a GPU answers ENODEVICE once the argument checks are through).
"""
import ctypes as C

import numpy as np
import pytest

import pyclaw_amd as pyclaw
import sharp3_reference as R
from apps import problems
from oracle import oracle as O
from pyclaw_amd import _lib, parallel

PCL_RP_CELL = 100
FWAVE, CAPA = 1, 2


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def compile3s(body, meqn, mwaves, aux=(), form=0, lim_type=2, weno_order=5, math=0):
    h = C.c_void_p()
    rc = _lib.lib().pcl_cellrp_compile3_sharp(body.encode(), b"", meqn, mwaves, math, (C.c_int * len(aux))(*aux) if aux else None,
                                              len(aux), form, lim_type, weno_order, C.byref(h))
    return rc, h


# ---- the reference's glue against the oracle, in two dimensions ---------------------------------------------------------------
@pytest.mark.parametrize("mcapa", [0, 1], ids=["nocapa", "capa"])
@pytest.mark.parametrize("lim_type,weno_order", [(1, 5), (2, 5), (3, 5), (2, 7)])
def test_the_glue_in_two_dimensions_is_the_oracles_flux2(coracle, lim_type, weno_order, mcapa):
    """13 x 9 acoustics, random state: dq over the whole array (the ghost lines 0 and m+1 included) and cfl, bit for bit"""
    rng = np.random.default_rng(100 * lim_type + 10 * weno_order + mcapa)
    mx, my, mbc = 13, 9, (weno_order + 1) // 2
    q = np.asfortranarray(rng.uniform(-1.0, 1.0, (3, mx + 2 * mbc, my + 2 * mbc)))
    aux = np.asfortranarray(rng.uniform(0.5, 1.5, (1, mx + 2 * mbc, my + 2 * mbc))) if mcapa else None
    par = [1.0, 4.0, 2.0, 2.0]
    mthlim = [4, 2, 1]          # by component
    dx, dy, dt = 0.1, 0.07, 0.013
    coracle.set_weno_order(weno_order)
    coracle.set_sharp_mthlim(np.array(mthlim, dtype=np.int32))
    try:
        want, cfl_want = coracle.sharp_flux2(O.RP_ACOUSTICS_2D, par, lim_type, 2, mcapa, mbc, mx, my, q, aux, dx, dy, dt)
    finally:
        coracle.set_weno_order(5)
        coracle.set_sharp_mthlim(np.array([1], dtype=np.int32))
    rpn = R.oracle_rpn2(coracle, O.RP_ACOUSTICS_2D, par, 3, 2, mbc)
    got, cfl = R.dq_reference(rpn, R.reconstruction(coracle, lim_type, weno_order, mbc, mthlim), q, aux, mcapa, mbc, (dx, dy), dt)
    print("max |glue - oracle| = %g, cfl %r / %r" % (np.abs(got - want).max(), cfl, cfl_want))
    assert np.abs(want).max() > 1e-3 and cfl_want > 0.0
    assert cfl == cfl_want
    assert np.array_equal(got, want)


def test_the_ghost_fill_of_the_reference():
    q = np.arange(2 * 4 * 3 * 2, dtype=float).reshape((2, 4, 3, 2)) + 1.0
    qb = R.fill_ghosts(q, 3, [R.PERIODIC, R.EXTRAP, R.WALL], [R.PERIODIC, R.EXTRAP, R.WALL])
    assert qb.shape == (2, 10, 9, 8)
    inner = qb[:, 3:-3, 3:-3, 3:-3]
    assert np.array_equal(inner, q)
    assert np.array_equal(qb[:, 0:3, 3:-3, 3:-3], q[:, 1:4]) and np.array_equal(qb[:, 7:10, 3:-3, 3:-3], q[:, 0:3])
    assert np.array_equal(qb[:, 3:-3, 0, 3:-3], q[:, :, 0]) and np.array_equal(qb[:, 3:-3, 8, 3:-3], q[:, :, 2])
    # the wall in z: mirror images; component 3 does not exist here (two components), so nothing is negated
    assert np.array_equal(qb[:, 3:-3, 3:-3, 2], q[:, :, :, 0]) and np.array_equal(qb[:, 3:-3, 3:-3, 1], q[:, :, :, 1])
    q4 = np.ones((4, 3, 4, 5))
    qb = R.fill_ghosts(q4, 3, [R.WALL] * 3, [R.WALL] * 3)
    assert (qb[1, :3] == -1).all() and (qb[2, 3:-3, :3] == -1).all() and (qb[3, 3:-3, 3:-3, -3:] == -1).all() and (qb[0] == 1).all()


# ---- the compile call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,meqn,mwaves,aux", [("VC_ACOUSTICS_3D_RP", 4, 2, (0, 1)), ("EULER_3D_RP", 5, 3, ())])
def test_the_bodies_compile_and_the_handle_says_what_it_is(name, meqn, mwaves, aux):
    L = _lib.lib()
    assert L.pcl_version() >= 115
    rp = pyclaw.SharpCellRiemann3D(getattr(problems, name) + "// sharp3 cpu test\n", meqn, mwaves, aux=aux)
    n0, h0 = stats()
    rp.compile('exact', sharp=(2, 5))
    assert stats() == (n0 + 1, h0)
    assert L.pcl_cellrp_check(rp._rp, meqn, mwaves, 3, 0) == 0
    assert L.pcl_cellrp_check(rp._rp, meqn, mwaves, 2, 0) == _lib.EINVAL and "ndim=3" in last_error()
    lim, order, cd = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(L.pcl_cellrp_sharp(rp._rp, C.byref(lim), C.byref(order), C.byref(cd)))
    assert (lim.value, order.value, cd.value) == (2, 5, 0)
    t3 = C.c_int(-1)
    _lib.check(L.pcl_cellrp_transverse3(rp._rp, C.byref(t3)))
    assert t3.value == 0
    # the same again compiles nothing; another reconstruction is another program
    rp.compile('exact', sharp=(2, 5))
    assert stats() == (n0 + 1, h0)
    rp.compile('exact', sharp=(3, 5))
    assert stats() == (n0 + 2, h0)
    rp.release()


def test_ixy_is_1_2_or_3_and_every_order_compiles_for_lim_type_2():
    rc, h = compile3s('static_assert(ixy != 3, "no z pass");\ns[0] = 1.0;\n', 1, 1)
    assert rc == _lib.EINVAL and "no z pass" in last_error() and "riemann:1" in last_error()
    rc, h = compile3s('static_assert(ixy >= 1 && ixy <= 3, "");\ns[0] = p[ixy - 1]; // orders\n', 1, 1, weno_order=17)
    assert rc == 0, last_error()
    rc, h = compile3s("s[0] = 1.0; // at the plane limit\n", 4, 1, aux=(0, 1, 2), form=CAPA, lim_type=1)
    assert rc == 0, last_error()


@pytest.mark.parametrize("kw,words", [
    (dict(form=FWAVE), ["PCL_CELLRP_FORM_FWAVE", "f-wave"]),
    (dict(form=FWAVE | CAPA), ["PCL_CELLRP_FORM_FWAVE", "PCL_CELLRP_FORM_CAPA only"]),
    (dict(form=4), ["form = 4"]),
    (dict(lim_type=0), ["lim_type must be 1", "got 0"]),
    (dict(lim_type=4), ["lim_type must be 1", "got 4"]),
    (dict(weno_order=3), ["weno_order must be odd, 5..17", "got 3"]),
    (dict(weno_order=6), ["weno_order must be odd, 5..17", "got 6"]),
    (dict(weno_order=19), ["weno_order must be odd, 5..17", "got 19"]),
    (dict(weno_order=7, lim_type=3), ["weno_order 7", "lim_type 2 only"]),
    (dict(weno_order=7, lim_type=1), ["weno_order 7", "lim_type 2 only"]),
    (dict(meqn=4, aux=(0, 1, 2, 3, 4)), ["meqn + capa + naux = 9", "at most 8"]),
    (dict(meqn=4, aux=(0, 1, 2, 3), form=CAPA), ["meqn + capa + naux = 9", "at most 8"]),
    (dict(meqn=8, form=CAPA), ["meqn + capa + naux = 9", "at most 8"]),
    (dict(meqn=9), ["1 <= meqn <= 8"]),
    (dict(meqn=0), ["1 <= meqn <= 8"]),
    (dict(mwaves=9), ["1 <= mwaves <= 8"]),
    (dict(aux=(0, 0)), ["listed twice"]),
    (dict(aux=(-1,)), ["negative"]),
    (dict(math=3), ["math mode"]),
])
def test_the_compile_call_refuses_before_the_compiler_with_the_reason(kw, words):
    args = dict(meqn=2, mwaves=1)
    args.update(kw)
    n0, h0 = stats()
    rc, h = compile3s("s[0] = 1.0; // never compiled\n", **args)
    assert rc == _lib.EINVAL and not h.value, last_error()
    assert "pcl_cellrp_compile" in last_error() or "math" in last_error()
    for w in words:
        assert w in last_error(), (w, last_error())
    assert stats() == (n0, h0)


def test_the_other_compile_calls_keep_their_answers_for_three_dimensions():
    L = _lib.lib()
    h, size = C.c_void_p(), C.c_long()
    rc = L.pcl_cellrp_compile_sharp(b"s[0] = 1.0;", b"", 1, 1, 3, 0, None, 0, 0, 2, 5, 0, C.byref(h), C.byref(size))
    assert rc == _lib.EINVAL and "ndim must be 1 or 2" in last_error()
    assert L.pcl_cellrp_compile3_sharp(None, b"", 1, 1, 0, None, 0, 0, 2, 5, C.byref(h)) == _lib.EINVAL and "null" in last_error()
    assert L.pcl_cellrp_compile3_sharp(b"s[0] = 1.0;", b"", 1, 1, 0, None, 0, 0, 2, 5, None) == _lib.EINVAL and "null" in last_error()


# ---- pcl_create_cellrp --------------------------------------------------------------------------------------------------------
def sharp_config(ndim=3, meqn=4, mwaves=2, maux=2, **over):
    cfg = _lib.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 3, meqn, mwaves, maux
    for k, v in enumerate([0, 2, 0, 0, 0, 0, maux]):      # as SharpClawSolver.setup fills it: method[2] stays 0
        cfg.method[k] = v
    cfg.mthlim[0] = cfg.mthlim[1] = 1
    cfg.rp = PCL_RP_CELL
    cfg.kind, cfg.lim_type = 1, 2
    for k, v in over.items():
        if k == "mcapa":
            cfg.method[5] = v
        elif k == "char_decomp":
            cfg.method[4] = v
        else:
            setattr(cfg, k, v)
    return cfg


@pytest.fixture(scope="module")
def handles():
    vc = problems.VC_ACOUSTICS_3D_RP
    out = {"w5": pyclaw.SharpCellRiemann3D(vc, 4, 2, aux=(0, 1)).compile('exact', sharp=(2, 5)),
           "legacy": pyclaw.SharpCellRiemann3D(vc, 4, 2, aux=(0, 1)).compile('exact', sharp=(3, 5)),
           "w7": pyclaw.SharpCellRiemann3D(vc, 4, 2, aux=(0, 1)).compile('exact', sharp=(2, 7)),
           "capa": pyclaw.SharpCellRiemann3D(vc, 4, 2, aux=(0, 1), capa=True).compile('exact', sharp=(2, 5)),
           "classic": pyclaw.CellRiemann3D(vc, 4, 2, aux=(0, 1)).compile(),
           "sharp2d": pyclaw.CellRiemann("s[0] = 1.0; // a 2-D SharpClaw handle of four equations\n", 4, 2, 2,
                                         sharpclaw=True).compile('exact', sharp=(2, 5, 0))}
    yield out
    for rp in out.values():
        rp.release()


def create(cfg, rp):
    s = C.c_void_p()
    rc = _lib.lib().pcl_create_cellrp(C.byref(cfg), rp._rp, C.byref(s))
    if rc == 0:
        _lib.lib().pcl_destroy(s)
    return rc


@pytest.mark.parametrize("which,over", [("w5", dict()), ("w5", dict(maux=5)), ("legacy", dict(lim_type=3)), ("w7", dict(mbc=4)),
                                        ("capa", dict(maux=3, mcapa=3))])
def test_an_accepted_configuration_passes_the_argument_checks(handles, which, over):
    """OK on a machine with a device, ENODEVICE without one: not EINVAL"""
    rc = create(sharp_config(**over), handles[which])
    assert rc in (0, _lib.ENODEVICE), last_error()


@pytest.mark.parametrize("which,over,words", [
    ("classic", dict(), ["3-D", "classic solver only", "pcl_cellrp_compile3_sharp"]),
    ("w5", dict(kind=0, mbc=2), ["3-D", "classic solver only", "SharpClaw kernels"]),
    ("w5", dict(lim_type=3), ["lim_type 2", "cfg.lim_type is 3"]),
    ("legacy", dict(), ["lim_type 3", "cfg.lim_type is 2"]),
    ("w5", dict(mbc=4), ["weno_order 5", "cfg.mbc is 4"]),
    ("w7", dict(), ["weno_order 7", "cfg.mbc is 3"]),
    ("w5", dict(char_decomp=1), ["char_decomp"]),
    ("capa", dict(), ["capacity function", "PCL_CELLRP_FORM_CAPA"]),
    ("w5", dict(maux=3, mcapa=3), ["capacity function", "compiled without one"]),
    ("w5", dict(fwave=1), ["f-waves", "3-D"]),
    ("w5", dict(maux=1), ["aux component 1", "maux = 1"]),
    ("w5", dict(meqn=5), ["meqn=4", "meqn=5"]),
    ("w5", dict(math=1), ["math=0", "math=1"]),
    ("sharp2d", dict(), ["PCL_RP_CELL", "ndim == 3"]),
    ("w5", dict(ndim=2), ["ndim=3", "ndim=2"]),
])
def test_pcl_create_cellrp_refuses_with_the_reason(handles, which, over, words):
    """EINVAL from the host-only checks, not ENODEVICE"""
    rc = create(sharp_config(**over), handles[which])
    assert rc == _lib.EINVAL, (rc, last_error())
    for w in words:
        assert w in last_error(), (w, last_error())


def test_pcl_create_keeps_refusing_a_builtin_solver_and_names_the_handle_route():
    L = _lib.lib()
    s = C.c_void_p()
    cfg = sharp_config(rp=20)
    assert L.pcl_create(C.byref(cfg), C.byref(s)) == _lib.EINVAL
    assert "3-D" in last_error() and "classic solver only" in last_error() and "pcl_cellrp_compile3_sharp" in last_error()
    assert L.pcl_create(C.byref(sharp_config()), C.byref(s)) == _lib.EINVAL and "PCL_RP_CELL" in last_error()
    info = (C.c_int * 10)()
    _lib.check(L.pcl_rp_info(20, info))
    assert info[7] == 0         # vc_acoustics_3d has no SharpClaw kernel of its own


# ---- the Python surface ---------------------------------------------------------------------------------------------------------
TINY = "wave[0][0] = qr[0] - ql[0];\ns[0] = p[ixy - 1];\namdq[0] = dmin(s[0], 0.0) * wave[0][0];\n" \
       "apdq[0] = dmax(s[0], 0.0) * wave[0][0];\n// sharp3 surface test\n"


def make_solution(ndim, meqn=1, maux=0, mcapa=None):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xyz"[:ndim]]
    state = pyclaw.State(pyclaw.Grid(dims), meqn, maux)
    state.q[...] = 1.0
    if maux:
        state.aux[...] = 1.0
    if mcapa is not None:
        state.mcapa = mcapa
    return pyclaw.Solution(state)


def solver3(cls=None, rp=None, **kw):
    s = (cls or pyclaw.SharpClawSolver3D)()
    s.rp = rp if rp is not None else pyclaw.SharpCellRiemann3D(TINY, 1, 1, params=[1.0, 0.5, 0.25], **kw)
    s.mwaves = 1
    return s


def accepted(solver, solution):
    try:
        solver.setup(solution)
    except _lib.PclError as e:
        assert e.code == _lib.ENODEVICE, e
    else:
        solver.teardown()


def test_sharpclaw_solver_3d_has_the_2d_defaults_and_takes_a_sharp_cell_riemann_3d():
    s3, s2 = pyclaw.SharpClawSolver3D(), pyclaw.SharpClawSolver2D()
    assert s3.ndim == 3
    for attr in ("lim_type", "weno_order", "time_integrator", "char_decomp", "cfl_max", "cfl_desired", "mbc", "fwave", "math",
                 "tfluct_solver", "dq_src", "limiters"):
        assert getattr(s3, attr) == getattr(s2, attr), attr
    s = solver3()
    accepted(s, make_solution(3))
    assert s.rp._rp is not None and _lib.lib().pcl_cellrp_check(s.rp._rp, 1, 1, 3, 0) == 0 and s.mbc == 3
    n1, _ = stats()
    s.rp.params = [2.0, 1.0, 0.5]
    accepted(s, make_solution(3))           # a second setup() compiles nothing
    assert stats()[0] == n1
    s.weno_order = 7
    accepted(s, make_solution(3))
    assert stats()[0] == n1 + 1 and s.mbc == 4
    for ti in ("Euler", "SSP33", "RK44"):
        s = solver3()
        s.time_integrator = ti
        accepted(s, make_solution(3))
    accepted(solver3(aux=(1,)), make_solution(3, maux=2))
    accepted(solver3(capa=True), make_solution(3, maux=1, mcapa=0))


def test_the_app_setups_take_solver_type_sharpclaw():
    claw = problems.acoustics3D(pyclaw, mx=8, my=8, mz=8, run=False, solver_type='sharpclaw', lim_type=3)
    assert isinstance(claw.solver, pyclaw.SharpClawSolver3D) and isinstance(claw.solver.rp, pyclaw.SharpCellRiemann3D)
    assert claw.solver.lim_type == 3 and claw.solver.rp.aux == (0, 1)
    accepted(claw.solver, claw.solution)
    claw = problems.euler3D(pyclaw, n=8, run=False, solver_type='sharpclaw', time_integrator='SSP33')
    assert isinstance(claw.solver, pyclaw.SharpClawSolver3D) and claw.solver.time_integrator == 'SSP33' and claw.solver.rp.meqn == 5
    accepted(claw.solver, claw.solution)
    assert isinstance(problems.acoustics3D(pyclaw, run=False).solver, pyclaw.ClawSolver3D)
    assert isinstance(problems.euler3D(pyclaw, run=False).solver, pyclaw.ClawSolver3D)


def test_the_python_surface_refuses_what_3d_sharpclaw_does_not_serve(monkeypatch):
    # a built-in solver: the refusal names the body that restates it
    s = pyclaw.SharpClawSolver3D()
    s.rp, s.mwaves = pyclaw.riemann.rp_vc_acoustics_3d, 2
    with pytest.raises(NotImplementedError, match="VC_ACOUSTICS_3D_RP"):
        s.setup(make_solution(3, meqn=4, maux=2))
    # a CellRiemann3D, a 2-D CellRiemann
    with pytest.raises(NotImplementedError, match="SharpCellRiemann3D"):
        solver3(rp=pyclaw.CellRiemann3D(TINY, 1, 1)).setup(make_solution(3))
    with pytest.raises(NotImplementedError, match="SharpCellRiemann3D"):
        solver3(rp=pyclaw.CellRiemann(TINY, 1, 1, 2, sharpclaw=True)).setup(make_solution(3))
    for attr, value, words in [("char_decomp", 1, "char_decomp"), ("char_decomp", 2, "char_decomp"),
                               ("tfluct_solver", True, "tfluct_solver"), ("fwave", True, "fwave")]:
        s = solver3()
        setattr(s, attr, value)
        with pytest.raises(NotImplementedError, match=words):
            s.setup(make_solution(3))
    # a decomposed run
    sol = make_solution(3)
    sol.states[0].decomp = object()
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="decomposed run"):
        solver3().setup(sol)
    monkeypatch.undo()
    # a SharpCellRiemann3D on any other solver class
    for cls, nd in [(pyclaw.SharpClawSolver2D, 2), (pyclaw.SharpClawSolver1D, 1)]:
        with pytest.raises(NotImplementedError, match="SharpClawSolver3D alone"):
            solver3(cls).setup(make_solution(nd))
    s = solver3(pyclaw.ClawSolver3D)
    s.limiters = 4
    with pytest.raises(NotImplementedError, match="sharpclaw=True"):
        s.setup(make_solution(3))
    # the form and the aux list
    with pytest.raises(NotImplementedError, match="capacity function"):
        solver3().setup(make_solution(3, maux=1, mcapa=0))
    with pytest.raises(ValueError, match="capa=True"):
        solver3(capa=True).setup(make_solution(3, maux=1))
    with pytest.raises(ValueError, match="aux component 2"):
        solver3(aux=(2,)).setup(make_solution(3, maux=2))
    # no keyword for what 3-D SharpClaw does not have; the plane limit; compile() without the reconstruction
    for kw in (dict(transverse="bmasdq[0] = 0.0;"), dict(fwave=True), dict(sharpclaw=True), dict(ndim=3), dict(rpt3="")):
        with pytest.raises(TypeError, match="unexpected keyword"):
            pyclaw.SharpCellRiemann3D(TINY, 1, 1, **kw)
    with pytest.raises(ValueError, match="meqn \\+ capa \\+ len\\(aux\\) = 9"):
        pyclaw.SharpCellRiemann3D(TINY, 4, 1, aux=(0, 1, 2, 3), capa=True)
    with pytest.raises(ValueError, match="sharp="):
        pyclaw.SharpCellRiemann3D(TINY, 1, 1).compile()
    with pytest.raises(NotImplementedError, match="char_decomp must be 0"):
        pyclaw.SharpCellRiemann3D(TINY, 1, 1).compile('exact', sharp=(2, 5, 1))
    # weno_order and lim_type, as in 1-D and 2-D
    s = solver3()
    s.weno_order, s.lim_type = 7, 3
    with pytest.raises(NotImplementedError, match="lim_type=2"):
        s.setup(make_solution(3))
