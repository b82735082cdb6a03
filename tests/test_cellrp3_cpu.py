"""
CPU: user-written Riemann solvers in the dimension-split 3-D step (pyclaw.CellRiemann3D, pcl_cellrp_compile3; DESIGN.md
4.4d) as far as they go without a device -- the run-time compile of the three passes of the library's 3-D sweep kernel
around the body, the cache, the plane limit of its tile, and every refusal of the compile call, of pcl_create_cellrp and of
the Python surface, each of which comes before any device call (a machine without a GPU answers ENODEVICE once the
argument checks are through).
"""
import ctypes as C

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from apps import problems
from pyclaw_amd import _lib, parallel

PCL_RP_CELL = 100
FWAVE, CAPA = 1, 2
MAX3 = 7        # planes of the 3-D sweep's tile; the library's own figure is read from its messages below


def stats():
    n, h = C.c_long(), C.c_long()
    _lib.check(_lib.lib().pcl_cellfn_stats(C.byref(n), C.byref(h)))
    return n.value, h.value


def last_error():
    return _lib.lib().pcl_last_error().decode()


def compile3(body, meqn, mwaves, aux=(), form=0, math=0):
    h, size = C.c_void_p(), C.c_long()
    rc = _lib.lib().pcl_cellrp_compile3(body.encode(), b"", meqn, mwaves, math, (C.c_int * len(aux))(*aux) if aux else None,
                                        len(aux), form, C.byref(h), C.byref(size))
    return rc, h, size.value


def form_of(h):
    f = C.c_int(-1)
    _lib.check(_lib.lib().pcl_cellrp_form(h, C.byref(f)))
    return f.value


def aux_of(h):
    n, idx = C.c_int(-1), (C.c_int * 8)()
    _lib.check(_lib.lib().pcl_cellrp_aux(h, C.byref(n), idx))
    return tuple(idx[:n.value])


# ---- the compile call ----------------------------------------------------------------------------------------------------
def test_the_restated_solver_compiles_and_the_handle_says_what_it_is():
    L = _lib.lib()
    assert L.pcl_version() >= 111
    body = problems.VC_ACOUSTICS_3D_RP + "// 3-D cpu test\n"
    n0, h0 = stats()
    rc, h, size = compile3(body, 4, 2, aux=(0, 1))
    assert rc == 0 and size > 0, last_error()
    assert stats() == (n0 + 1, h0)
    assert L.pcl_cellrp_check(h, 4, 2, 3, 0) == 0
    for other in [(4, 2, 2, 0), (4, 2, 1, 0), (3, 2, 3, 0), (4, 3, 3, 0), (4, 2, 3, 1)]:
        assert L.pcl_cellrp_check(h, *other) == _lib.EINVAL
        assert "compiled for meqn=4 mwaves=2 ndim=3 math=0" in last_error()
    assert form_of(h) == 0 and aux_of(h) == (0, 1)
    has = C.c_int(-1)
    _lib.check(L.pcl_cellrp_transverse(h, C.byref(has), None))
    lim, order, cd = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _lib.check(L.pcl_cellrp_sharp(h, C.byref(lim), C.byref(order), C.byref(cd)))
    assert has.value == 0 and (lim.value, order.value, cd.value) == (0, 0, 0)
    # the same text again compiles nothing
    rc, h2, size2 = compile3(body, 4, 2, aux=(0, 1))
    assert rc == 0 and h2.value == h.value and size2 == size and stats() == (n0 + 1, h0 + 1)
    # another aux list, another form: other programs
    rc, h3, _ = compile3(body, 4, 2, aux=(1, 0))
    assert rc == 0 and h3.value != h.value and aux_of(h3) == (1, 0) and stats() == (n0 + 2, h0 + 1)
    rc, h4, _ = compile3(body, 4, 2, aux=(0, 1), form=CAPA)
    assert rc == 0 and h4.value not in (h.value, h3.value) and form_of(h4) == CAPA and stats() == (n0 + 3, h0 + 1)
    for k in (h, h2, h3, h4):
        L.pcl_cellrp_release(k)


@pytest.mark.parametrize("math", ["exact", "fast", "strict"])
@pytest.mark.parametrize("name,meqn,mwaves,aux", [("VC_ACOUSTICS_3D_RP", 4, 2, (0, 1)), ("ACOUSTICS_3D_RP", 4, 2, ()),
                                                  ("ADVECTION_3D_RP", 1, 1, ()), ("BURGERS_3D_RP", 1, 1, ()),
                                                  ("EULER_3D_RP", 5, 3, ())])
def test_every_3d_body_compiles_in_every_mode(name, meqn, mwaves, aux, math):
    rp = pyclaw.CellRiemann3D(getattr(problems, name), meqn, mwaves, aux=aux).compile(math)
    assert rp.code_size > 0 and rp.ndim == 3 and _lib.lib().pcl_cellrp_check(rp._rp, meqn, mwaves, 3,
                                                                              ["exact", "fast", "strict"].index(math)) == 0


def test_ixy_is_1_2_or_3_and_diagnostics_carry_the_bodys_lines():
    rc, h, size = compile3('static_assert(ixy >= 1 && ixy <= 3, "");\ns[0] = p[ixy - 1];\n', 1, 1)
    assert rc == 0 and size > 0, last_error()
    # (a direction that is never instantiated would let this one through: all three are)
    rc, h, _ = compile3('static_assert(ixy != 3, "no z sweep");\ns[0] = 1.0;\n', 1, 1)
    assert rc == _lib.EINVAL and "no z sweep" in last_error() and "riemann:1" in last_error()
    rc, h, _ = compile3("wave[0][0] = qr[0] - ql[0];\ns[0] = 1.0;\namdq[0] = no_such_name;\n", 1, 1)
    assert rc == _lib.EINVAL and "no_such_name" in last_error() and "riemann:3" in last_error()
    with pytest.raises(_lib.PclError) as e:
        pyclaw.CellRiemann3D("s[0] = 1.0;\ns[0] = other_name;\n", 1, 1).compile()
    assert "other_name" in str(e.value) and "riemann:2" in str(e.value)


@pytest.mark.parametrize("meqn,aux,form", [(MAX3, (), 0), (MAX3 - 1, (), CAPA), (MAX3 - 2, (3, 0), 0), (4, (0, 1), CAPA)])
def test_a_spec_at_the_plane_limit_compiles(meqn, aux, form):
    if meqn + len(aux) + (form == CAPA) < MAX3:
        aux = aux + tuple(range(4, 4 + MAX3 - meqn - len(aux) - (form == CAPA)))
    assert meqn + len(aux) + (form == CAPA) == MAX3
    rc, h, size = compile3("s[0] = 1.0; // plane limit\n", meqn, 1, aux=aux, form=form)
    assert rc == 0 and size > 0, last_error()


@pytest.mark.parametrize("meqn,aux,form,what", [(4, (0, 1, 2, 3), 0, "one more aux component"), (4, (0, 1, 2), CAPA, "capa"),
                                                (5, (0, 1, 2), 0, "one more equation"), (8, (), 0, "meqn alone")])
def test_one_more_plane_is_refused_with_the_sum_and_the_limit(meqn, aux, form, what):
    capa = form == CAPA
    assert meqn + len(aux) + capa == MAX3 + 1
    n0, h0 = stats()
    rc, h, _ = compile3("s[0] = 1.0; // never compiled\n", meqn, 1, aux=aux, form=form)
    assert rc == _lib.EINVAL and h.value is None, what
    msg = last_error()
    assert "meqn + naux + capa = %d" % (MAX3 + 1) in msg and "at most %d planes" % MAX3 in msg, msg
    assert stats() == (n0, h0)
    # the Python object refuses the same before any compile
    with pytest.raises(ValueError, match="= %d, the tile of the 3-D sweeps holds at most %d planes" % (MAX3 + 1, MAX3)):
        pyclaw.CellRiemann3D("s[0] = 1.0;", meqn, 1, aux=aux, capa=capa)
    assert stats() == (n0, h0) and pyclaw.CellRiemann3D.MAX_PLANES == MAX3


def test_the_fwave_bit_and_unknown_bits_are_refused():
    n0, h0 = stats()
    for form in (FWAVE, FWAVE | CAPA):
        rc, h, _ = compile3("s[0] = 1.0;", 1, 1, form=form)
        assert rc == _lib.EINVAL and "f-wave" in last_error() and "pcl_cellrp_compile3" in last_error()
    rc, h, _ = compile3("s[0] = 1.0;", 1, 1, form=4)
    assert rc == _lib.EINVAL and "form = 4" in last_error()
    assert stats() == (n0, h0)


def test_the_other_compile_calls_keep_refusing_ndim_3():
    L = _lib.lib()
    h = C.c_void_p()
    one = (C.c_int * 1)(0)
    calls = [lambda: L.pcl_cellrp_compile(b"s[0] = 1.0;", b"", 1, 1, 3, 0, C.byref(h), None),
             lambda: L.pcl_cellrp_compile_aux(b"s[0] = 1.0;", b"", 1, 1, 3, 0, one, 1, C.byref(h), None),
             lambda: L.pcl_cellrp_compile_form(b"s[0] = 1.0;", None, b"", 1, 1, 3, 0, None, 0, CAPA, C.byref(h), None),
             lambda: L.pcl_cellrp_compile_sharp(b"s[0] = 1.0;", b"", 1, 1, 3, 0, None, 0, 0, 2, 5, 0, C.byref(h), None)]
    for call in calls:
        assert call() == _lib.EINVAL and "ndim must be 1 or 2" in last_error()
    assert L.pcl_cellrp_compile_t(b"s[0] = 1.0;", b"bmasdq[0] = 0.0;", b"", 1, 1, 3, 0, None, 0, C.byref(h), None) == _lib.EINVAL
    assert "ndim must be 2" in last_error()
    with pytest.raises(ValueError, match="ndim must be 1 or 2"):
        pyclaw.CellRiemann("s[0] = 1.0;", 1, 1, 3)
    assert L.pcl_cellrp_compile3(None, b"", 1, 1, 0, None, 0, 0, C.byref(h), None) == _lib.EINVAL
    assert L.pcl_cellrp_compile3(b"s[0] = 1.0;", b"", 1, 1, 7, None, 0, 0, C.byref(h), None) == _lib.EINVAL      # no such math mode
    assert L.pcl_cellrp_compile3(b"s[0] = 1.0;", b"", 9, 1, 0, None, 0, 0, C.byref(h), None) == _lib.EINVAL
    assert L.pcl_cellrp_compile3(b"s[0] = 1.0;", b"", 1, 1, 0, None, 1, 0, C.byref(h), None) == _lib.EINVAL      # a list of one, not given
    neg = (C.c_int * 1)(-1)
    assert L.pcl_cellrp_compile3(b"s[0] = 1.0;", b"", 1, 1, 0, neg, 1, 0, C.byref(h), None) == _lib.EINVAL and "negative" in last_error()


# ---- pcl_create_cellrp ----------------------------------------------------------------------------------------------------
def cell_config(ndim=3, meqn=4, mwaves=2, maux=2, **over):
    cfg = _lib.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k] = 8
        cfg.d[k] = 0.1
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = 2, meqn, mwaves, maux
    for k, v in enumerate([1, 2, -1 if ndim > 1 else 0, 0, 0, 0, maux]):
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


@pytest.fixture(scope="module")
def handles():
    """'vc': aux (0, 1); 'plain': no aux; 'capa': aux (0, 1) with a capacity function; '2d': a 2-D handle of four equations"""
    out = {"vc": pyclaw.CellRiemann3D(problems.VC_ACOUSTICS_3D_RP, 4, 2, aux=(0, 1)).compile(),
           "plain": pyclaw.CellRiemann3D(problems.ACOUSTICS_3D_RP, 4, 2, params=[1.0, 1.0]).compile(),
           "capa": pyclaw.CellRiemann3D(problems.VC_ACOUSTICS_3D_RP, 4, 2, aux=(0, 1), capa=True).compile(),
           "2d": pyclaw.CellRiemann("s[0] = 1.0; // a 2-D handle of four equations\n", 4, 2, 2).compile()}
    yield out
    for rp in out.values():
        rp.release()


def create(cfg, rp):
    s = C.c_void_p()
    rc = _lib.lib().pcl_create_cellrp(C.byref(cfg), rp._rp, C.byref(s))
    if rc == 0:
        _lib.lib().pcl_destroy(s)
    return rc


@pytest.mark.parametrize("which,over", [("vc", dict()), ("vc", dict(maux=5)), ("plain", dict(maux=0)), ("plain", dict(maux=2)),
                                        ("capa", dict(maux=3, mcapa=3)), ("capa", dict(maux=2, mcapa=1))])
def test_a_3d_configuration_with_a_3d_handle_passes_the_argument_checks(handles, which, over):
    """OK on a machine with a device, ENODEVICE without one: not EINVAL"""
    rc = create(cell_config(**over), handles[which])
    assert rc in (0, _lib.ENODEVICE), last_error()


@pytest.mark.parametrize("which,over,words", [
    ("vc", dict(order_trans=0), ["rpt3", "rptt3"]),
    ("vc", dict(order_trans=22), ["rpt3", "method[2]"]),
    ("vc", dict(fwave=1), ["f-waves", "3-D"]),
    ("vc", dict(mbc=3), ["mbc == 2"]),
    ("vc", dict(kind=1, mbc=3, lim_type=2), ["3-D", "classic solver only"]),
    ("vc", dict(ndim=2, meqn=4), ["ndim=3", "ndim=2"]),
    ("vc", dict(ndim=1, meqn=4), ["ndim=3", "ndim=1"]),
    ("vc", dict(maux=1), ["aux component 1", "maux = 1"]),
    ("vc", dict(maux=0), ["aux component 1", "maux = 0"]),
    ("capa", dict(maux=2), ["capacity function", "PCL_CELLRP_FORM_CAPA"]),
    ("vc", dict(maux=3, mcapa=3), ["capacity function", "compiled without one"]),
    ("plain", dict(meqn=5), ["meqn=4", "meqn=5"]),
    ("2d", dict(), ["PCL_RP_CELL", "ndim == 3", "pcl_cellrp_compile3"]),
])
def test_pcl_create_cellrp_refuses_with_the_reason(handles, which, over, words):
    """EINVAL from the host-only checks, not ENODEVICE"""
    rc = create(cell_config(**over), handles[which])
    assert rc == _lib.EINVAL, (rc, last_error())
    for w in words:
        assert w in last_error(), (w, last_error())


def test_pcl_create_keeps_refusing_a_user_solver_in_3d_and_a_dead_handle_is_one():
    L = _lib.lib()
    s = C.c_void_p()
    assert L.pcl_create(C.byref(cell_config()), C.byref(s)) == _lib.EINVAL
    assert "PCL_RP_CELL" in last_error() and "ndim == 3" in last_error()
    assert L.pcl_create_cellrp(C.byref(cell_config()), None, C.byref(s)) == _lib.EINVAL and "not a live" in last_error()


# ---- the Python surface ---------------------------------------------------------------------------------------------------
TINY = "wave[0][0] = qr[0] - ql[0];\ns[0] = p[ixy - 1];\namdq[0] = dmin(s[0], 0.0) * wave[0][0];\n" \
       "apdq[0] = dmax(s[0], 0.0) * wave[0][0];\n// 3-D surface test\n"


def make_solution(ndim, maux=0, mcapa=None):
    dims = [pyclaw.Dimension(n, 0.0, 1.0, 8) for n in "xyz"[:ndim]]
    state = pyclaw.State(pyclaw.Grid(dims), 1, maux)
    state.q[...] = 1.0
    if maux:
        state.aux[...] = 1.0
    if mcapa is not None:
        state.mcapa = mcapa
    return pyclaw.Solution(state)


def solver3(cls=None, **kw):
    s = (cls or pyclaw.ClawSolver3D)()
    s.rp = pyclaw.CellRiemann3D(TINY, 1, 1, params=[1.0, 0.5, 0.25], **kw)
    s.mwaves = 1
    s.limiters = 4
    return s


def accepted(solver, solution):
    """setup() up to the device: on a machine without one the library answers ENODEVICE behind every argument check"""
    try:
        solver.setup(solution)
    except _lib.PclError as e:
        assert e.code == _lib.ENODEVICE, e
    else:
        solver.teardown()


def test_claw_solver_3d_takes_a_cell_riemann_3d():
    n0, _ = stats()
    s = solver3()
    accepted(s, make_solution(3))
    assert s.rp._rp is not None and _lib.lib().pcl_cellrp_check(s.rp._rp, 1, 1, 3, 0) == 0
    n1, _ = stats()
    assert n1 <= n0 + 1
    # reassigning the parameters and setting up again compiles nothing
    s.rp.params = [2.0, 1.0, 0.5]
    accepted(s, make_solution(3))
    assert stats()[0] == n1
    accepted(solver3(aux=(1,)), make_solution(3, maux=2))
    accepted(solver3(capa=True), make_solution(3, maux=1, mcapa=0))


def test_the_python_surface_refuses_what_3d_does_not_serve(monkeypatch):
    s = solver3()
    s.dim_split = False
    with pytest.raises(NotImplementedError, match="rpt3"):
        s.setup(make_solution(3))
    for cls, nd in [(pyclaw.ClawSolver2D, 2), (pyclaw.ClawSolver1D, 1)]:
        with pytest.raises(NotImplementedError, match="ClawSolver3D alone"):
            solver3(cls).setup(make_solution(nd))
    s = solver3(pyclaw.SharpClawSolver2D)
    with pytest.raises(NotImplementedError, match="SharpClaw"):
        s.setup(make_solution(2))
    # a 1-D or 2-D solver on ClawSolver3D
    s = pyclaw.ClawSolver3D()
    s.rp = pyclaw.CellRiemann(TINY, 1, 1, 2)
    s.mwaves = 1
    with pytest.raises(NotImplementedError, match="ClawSolver3D"):
        s.setup(make_solution(3))
    # no keyword for what 3-D does not have
    for kw in (dict(transverse="bmasdq[0] = 0.0;"), dict(fwave=True), dict(sharpclaw=True), dict(ndim=3)):
        with pytest.raises(TypeError, match="unexpected keyword"):
            pyclaw.CellRiemann3D(TINY, 1, 1, **kw)
    # the form, the aux list, f-waves on the solver
    with pytest.raises(NotImplementedError, match="capacity function"):
        solver3().setup(make_solution(3, maux=1, mcapa=0))
    with pytest.raises(ValueError, match="capa=True"):
        solver3(capa=True).setup(make_solution(3, maux=1))
    with pytest.raises(ValueError, match="aux component 2"):
        solver3(aux=(2,)).setup(make_solution(3, maux=2))
    s = solver3()
    s.fwave = True
    with pytest.raises(NotImplementedError, match="fwave"):
        s.setup(make_solution(3))
    # a decomposed state
    sol = make_solution(3)
    sol.states[0].decomp = object()         # only looked at as "decomposed"; the refusal comes before it is used
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        solver3().setup(sol)


# ---- the Roe formulas of EULER_3D_RP restated in numpy (tests/test_gpu_cellrp3.py compares the device with them) ------------
def euler_roe(ql, qr, ixy, gamma):
    """apps/problems.py: EULER_3D_RP, formula by formula, on arrays (5, ...) of left and right cells; returns wave (3, 5, ...),
    s (3, ...), amdq and apdq (5, ...)"""
    mu, mv, mw = ixy, ixy % 3 + 1, (ixy + 1) % 3 + 1
    g1 = gamma - 1.0
    rsl, rsr = np.sqrt(ql[0]), np.sqrt(qr[0])
    rsq2 = rsl + rsr
    pl = g1 * (ql[4] - 0.5 * (ql[mu] * ql[mu] + ql[mv] * ql[mv] + ql[mw] * ql[mw]) / ql[0])
    pr = g1 * (qr[4] - 0.5 * (qr[mu] * qr[mu] + qr[mv] * qr[mv] + qr[mw] * qr[mw]) / qr[0])
    u = (ql[mu] / rsl + qr[mu] / rsr) / rsq2
    v = (ql[mv] / rsl + qr[mv] / rsr) / rsq2
    w = (ql[mw] / rsl + qr[mw] / rsr) / rsq2
    enth = ((ql[4] + pl) / rsl + (qr[4] + pr) / rsr) / rsq2
    uvw2 = u * u + v * v + w * w
    a2 = g1 * (enth - 0.5 * uvw2)
    a = np.sqrt(a2)
    g1a2, euv = g1 / a2, enth - uvw2
    d1, d2, d3, d4, d5 = qr[0] - ql[0], qr[mu] - ql[mu], qr[mv] - ql[mv], qr[mw] - ql[mw], qr[4] - ql[4]
    b4 = g1a2 * (euv * d1 + u * d2 + v * d3 + w * d4 - d5)
    b2 = d3 - v * d1
    b3 = d4 - w * d1
    b5 = (d2 + (a - u) * d1 - a * b4) / (2.0 * a)
    b1 = d1 - b4 - b5
    wave = np.zeros((3, 5) + ql.shape[1:])
    wave[0, 0], wave[0, mu], wave[0, mv], wave[0, mw], wave[0, 4] = b1, b1 * (u - a), b1 * v, b1 * w, b1 * (enth - u * a)
    wave[1, 0], wave[1, mu], wave[1, mv], wave[1, mw] = b4, b4 * u, b4 * v + b2, b4 * w + b3
    wave[1, 4] = b4 * 0.5 * uvw2 + b2 * v + b3 * w
    wave[2, 0], wave[2, mu], wave[2, mv], wave[2, mw], wave[2, 4] = b5, b5 * (u + a), b5 * v, b5 * w, b5 * (enth + u * a)
    s = np.stack([u - a, u, u + a])
    amdq = sum(np.minimum(s[k], 0.0) * wave[k] for k in range(3))
    apdq = sum(np.maximum(s[k], 0.0) * wave[k] for k in range(3))
    return wave, s, amdq, apdq


def euler_flux(q, ixy, gamma):
    """the flux of the 3-D Euler equations in direction ixy"""
    un = q[ixy] / q[0]
    pres = (gamma - 1.0) * (q[4] - 0.5 * (q[1] ** 2 + q[2] ** 2 + q[3] ** 2) / q[0])
    f = np.stack([q[ixy], q[1] * un, q[2] * un, q[3] * un, (q[4] + pres) * un])
    f[ixy] = f[ixy] + pres
    return f


def test_the_numpy_restatement_of_the_euler_body_is_self_consistent():
    """a uniform state gives zero waves, and amdq + apdq = f(qr) - f(ql) to the project's relative gate (1e-12 of the
    largest value), in every direction"""
    rng = np.random.default_rng(8)
    n = 500
    ql, qr = (np.empty((5, n)) for _ in range(2))
    for q in (ql, qr):
        q[0] = rng.uniform(0.5, 2.0, n)
        q[1:4] = q[0] * rng.uniform(-1.0, 1.0, (3, n))
        q[4] = rng.uniform(1.0, 3.0, n) / 0.4 + 0.5 * (q[1:4] ** 2).sum(axis=0) / q[0]
    for ixy in (1, 2, 3):
        wave, s, amdq, apdq = euler_roe(ql, ql.copy(), ixy, 1.4)
        assert not wave.any() and not amdq.any() and not apdq.any() and np.isfinite(s).all()
        assert np.allclose(s[1], ql[ixy] / ql[0], rtol=1e-14, atol=1e-15)
        wave, s, amdq, apdq = euler_roe(ql, qr, ixy, 1.4)
        df = euler_flux(qr, ixy, 1.4) - euler_flux(ql, ixy, 1.4)
        scale = max(np.abs(euler_flux(qr, ixy, 1.4)).max(), np.abs(euler_flux(ql, ixy, 1.4)).max())
        err = np.abs(amdq + apdq - df).max()
        print("ixy %d: |amdq + apdq - df| <= %g, largest flux %g" % (ixy, err, scale))
        assert err <= 1e-12 * scale
        # the waves sum to the jump
        assert np.abs(wave.sum(axis=0) - (qr - ql)).max() <= 1e-12 * np.abs(qr).max()
