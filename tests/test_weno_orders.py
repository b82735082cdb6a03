"""
SharpClaw reconstruction of order 7 .. 17 (weno.f90: weno7 ... weno17, `solver.weno_order`, lim_type = 2).

PINNING.  (1) tools/gen_weno.py derives every coefficient from first principles in rational arithmetic; where the
reference tree is present its 15-digit literals are compared with the ones in the reference's generated Fortran (read
as text): all 1792 agree; everywhere else with that literal sequence as pinned in tests/golden/ref_pins.json.  (2) tests/golden/ref_sharp_weno_orders.npz holds flux2.f90 outputs of the reference's own
Fortran (flang build) for every order: the C oracle (CPU) and the HIP path (GPU) reproduce them bit for bit.  (3) The
reference's regression test_1D_acoustics_with_weno17 (test/test_examples.py:160-170: one-period L1 error
0.000163221216565, gate 1e-5) is replayed by the oracle driver and by the product.
"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_pins as P
from oracle import driver as D
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("make_ref_goldens", os.path.join(HERE, "golden", "make_ref_goldens.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
ORDERS = [7, 9, 11, 13, 15, 17]
REF_WENO = "/root/reference/src/fortran/1d/sharpclaw/weno.f90"


@pytest.fixture(autouse=True)
def _reset_order(coracle):
    yield
    coracle.set_weno_order(5)


def test_committed_tables_are_what_the_generator_writes(tmp_path):
    spec = importlib.util.spec_from_file_location("gen_weno", os.path.join(ROOT, "tools", "gen_weno.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.emit(str(tmp_path / "a.hpp"), None, "static __device__ const")
    gen.emit(str(tmp_path / "b.h"), "ORC_WENO_TABLES_H", "static const")
    assert open(tmp_path / "a.hpp").read() == open(os.path.join(ROOT, "pyclaw_amd", "csrc", "weno_tables.hpp")).read()
    assert open(tmp_path / "b.h").read() == open(os.path.join(ROOT, "oracle", "weno_tables.h")).read()


def test_derived_literals_equal_the_reference_files():
    """the literal sequence of every wenoN subroutine of the reference's weno.f90 is pinned (tests/ref_pins.py); the
    file itself is read as well where the reference tree is present"""
    spec = importlib.util.spec_from_file_location("gen_weno", os.path.join(ROOT, "tools", "gen_weno.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for k in gen.KS:
        P.check("weno%d_literals" % (2 * k - 1), gen.derived_literals(k))
    if os.path.exists(REF_WENO):
        txt = open(REF_WENO).read()
        for k in gen.KS:
            P.record("weno%d_literals" % (2 * k - 1), gen.reference_literals(txt, k))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_weno.py"), "--check", REF_WENO],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count(" 0 textual differences, 0 differ as REAL*4") == 7, r.stdout


def test_generic_form_with_k3_is_weno5(coracle):
    rng = np.random.default_rng(3)
    q = np.asfortranarray(rng.standard_normal((4, 80)))
    a, b = coracle.weno5(2, 3, q), coracle.weno_k(5, q)
    assert np.array_equal(a[0][:, 2:-2], b[0][:, 2:-2]) and np.array_equal(a[1][:, 2:-2], b[1][:, 2:-2])


@pytest.mark.parametrize("order", ORDERS)
def test_polynomials_are_reproduced(coracle, order):
    """a polynomial of degree 2k-2 has equal smoothness on... no: every candidate stencil reproduces degree k-1
    exactly, so for data that ARE cell averages of a degree k-1 polynomial ql / qr are its edge values (to rounding of
    the float32-rounded coefficients: ~1e-6 relative)."""
    k = (order + 1) // 2
    x = np.arange(60, dtype=np.float64)
    c = np.random.default_rng(order).standard_normal(k) / np.array([10.0 ** j for j in range(k)])
    P = np.polynomial.Polynomial(c).integ()
    avg = (P(x + 0.5) - P(x - 0.5))[None, :]
    ql, qr = coracle.weno_k(order, np.asfortranarray(avg))
    p = np.polynomial.Polynomial(c)
    i = np.arange(k, 60 - k)
    scale = np.abs(avg).max()
    assert np.abs(ql[0, i] - p(x[i] - 0.5)).max() < 2e-5 * scale
    assert np.abs(qr[0, i] - p(x[i] + 0.5)).max() < 2e-5 * scale


@pytest.mark.parametrize("order", ORDERS)
def test_oracle_reproduces_the_reference_golden(coracle, order):
    z = np.load(os.path.join(HERE, "golden", "ref_sharp_weno_orders.npz"), allow_pickle=False)
    mx, my, g = int(z["mx"]), int(z["my"]), (order + 1) // 2
    q0 = G.euler_state_mild(60 + order, (mx + 2 * g, my + 2 * g))
    coracle.set_weno_order(order)
    dq, cfl = coracle.sharp_flux2(O.RP_EULER5_2D, G.PAR, 2, 5, 0, g, mx, my, q0, None, float(z["dx"]), float(z["dy"]),
                                  float(z["dt"]))
    assert np.array_equal(dq[:, g:-g, g:-g], z["dq_order%d" % order]) and cfl == float(z["cfl_order%d" % order])


@pytest.mark.parametrize("order", ORDERS)
def test_oracle_equals_the_reference_build(coracle, order):
    """the reference build's result is pinned (tests/ref_pins.py); compared with the live build where it is present"""
    ref = O.RefSharp2DEuler() if O.RefSharp2DEuler.available() else None
    g, mx, my = (order + 1) // 2, 23, 41
    q0 = G.euler_state_mild(order, (mx + 2 * g, my + 2 * g))
    coracle.set_weno_order(order)
    a, ca = coracle.sharp_flux2(O.RP_EULER5_2D, G.PAR, 2, 5, 0, g, mx, my, q0, None, 0.03, 0.02, 0.002)
    assert not np.isnan(a[:, g:-g, g:-g]).any()
    P.check("sharp_flux2_weno%d" % order, a[:, g:-g, g:-g], ca)
    if ref is not None:
        b, cb = ref.sharp_flux2(O.RP_EULER5_2D, G.PAR, 2, 5, 0, g, mx, my, q0, None, 0.03, 0.02, 0.002,
                                weno_order=order)
        P.record("sharp_flux2_weno%d" % order, b[:, g:-g, g:-g], cb)
        assert np.array_equal(a[:, g:-g, g:-g], b[:, g:-g, g:-g]) and ca == cb


def test_oracle_acoustics1d_weno17_scalar(coracle):
    """test/test_examples.py:160-170"""
    p = D.acoustics1d_problem(solver_type='sharpclaw', weno_order=17, cfl_max=2.5, cfl_desired=2.45)
    q0 = p.q.copy()
    D.run(p, coracle, 1.0, 5)
    err = p.d[0] * np.sum(np.abs(p.q.reshape(-1) - q0.reshape(-1)))
    assert abs(err - 0.000163221216565) < 1e-5, err


# ------------------------------------------------------------------------------------------- GPU
def _make(L, ndim, n, rp, meqn, mwaves, par, d, mbc, math=0):
    cfg = L.Config()
    cfg.ndim = ndim
    for k in range(ndim):
        cfg.n[k] = n[k]
        cfg.d[k] = d[k]
    cfg.mbc = mbc
    cfg.meqn, cfg.mwaves, cfg.rp = meqn, mwaves, rp
    cfg.method[1] = 2
    for k, v in enumerate(par):
        cfg.rp_params[k] = v
    cfg.kind = 1
    cfg.lim_type = 2
    cfg.math = math
    h = C.c_void_p()
    L.check(L.lib().pcl_create(C.byref(cfg), C.byref(h)))
    return h


def _device_dq(L, h, q, dt):
    try:
        L.check(L.lib().pcl_put_q(h, L.d(q), 1))
        cfl = C.c_double()
        L.check(L.lib().pcl_sharp_dq(h, dt, C.cast(C.byref(cfl), L.dp)))
        L.check(L.lib().pcl_select(h, 3))
        out = np.zeros_like(q)
        L.check(L.lib().pcl_get_q(h, L.d(out), 1))
    finally:
        L.lib().pcl_destroy(h)
    return out, cfl.value


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_hip_reproduces_the_reference_golden(order):
    from pyclaw_amd import _lib as L
    z = np.load(os.path.join(HERE, "golden", "ref_sharp_weno_orders.npz"), allow_pickle=False)
    mx, my, g = int(z["mx"]), int(z["my"]), (order + 1) // 2
    dx, dy, dt = float(z["dx"]), float(z["dy"]), float(z["dt"])
    q0 = G.euler_state_mild(60 + order, (mx + 2 * g, my + 2 * g))
    dq = np.zeros_like(q0)
    cfl = C.c_double()
    L.check(L.lib().pcl_sharp_flux2(O.RP_EULER5_2D, L.d(np.array(G.PAR + [0.0] * 6)), 2, 5, 5, 0, 0, g, mx, my,
                                    L.d(q0), L.d(dq), None, dx, dy, dt, C.cast(C.byref(cfl), L.dp)))
    assert np.array_equal(dq[:, g:-g, g:-g], z["dq_order%d" % order]) and cfl.value == float(z["cfl_order%d" % order])


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mx,my", [(1, 1), (47, 46), (46, 50), (100, 33), (131, 17)])
def test_hip_flux2_euler_bitexact(coracle, order, mx, my):
    """strips of 64 - 2k cells: sizes around one and two strips of every order"""
    from pyclaw_amd import _lib as L
    g = (order + 1) // 2
    q = G.euler_state_mild(1000 * order + mx, (mx + 2 * g, my + 2 * g))
    dx, dy, dt = 1.0 / mx, 0.8 / my, 0.01 / max(mx, my)
    coracle.set_weno_order(order)
    ref, cfl_ref = coracle.sharp_flux2(O.RP_EULER5_2D, G.PAR, 2, 5, 0, g, mx, my, q, None, dx, dy, dt)
    out, cfl = _device_dq(L, _make(L, 2, (mx, my), 11, 5, 5, G.PAR, (dx, dy), g), q, dt)
    inner = (slice(None), slice(g, -g), slice(g, -g))
    assert np.array_equal(out[inner], ref[inner]), np.abs(out[inner] - ref[inner]).max()
    assert cfl == cfl_ref


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mx", [1, 45, 46, 47, 300])
def test_hip_flux1_acoustics1d_bitexact(coracle, order, mx):
    from pyclaw_amd import _lib as L
    g = (order + 1) // 2
    q = np.asfortranarray(np.random.default_rng(order * 7 + mx).standard_normal((2, mx + 2 * g)))
    par = [1.0, 1.0, 1.0, 1.0]
    dx, dt = 1.0 / mx, 0.5 / mx
    coracle.set_weno_order(order)
    ref, cfl_ref = coracle.sharp_flux1(O.RP_ACOUSTICS_1D, par, 2, 2, 0, g, mx, q, None, dx, dt)
    out, cfl = _device_dq(L, _make(L, 1, (mx,), 2, 2, 2, par, (dx,), g), q, dt)
    assert np.array_equal(out[:, g:-g], ref[:, g:-g]), np.abs(out - ref)[:, g:-g].max()
    assert cfl == cfl_ref


def _small_case(name, g):
    """ndim, rp, meqn, mwaves, par, q, aux of one solver at 9 (x 5) cells with g ghost layers"""
    rng = np.random.default_rng(sum(ord(c) for c in name))
    n1, n2 = (9 + 2 * g,), (9 + 2 * g, 5 + 2 * g)
    if name == "advection_1d":
        return 1, O.RP_ADVECTION_1D, 1, 1, [0.7], rng.standard_normal((1,) + n1), None
    if name == "burgers_1d":
        return 1, O.RP_BURGERS_1D, 1, 1, [], rng.standard_normal((1,) + n1), None        # both signs: transonic fix
    if name == "advection_color_1d":
        return 1, O.RP_ADVECTION_COLOR_1D, 1, 1, [], rng.random((1,) + n1), 1.5 * (rng.random((1,) + n1) - 0.3)
    if name == "shallow_1d":
        h = 0.5 + rng.random(n1)
        return 1, O.RP_SHALLOW_1D, 2, 2, [9.81], np.stack([h, h * 0.3 * rng.standard_normal(n1)]), None
    if name == "euler_1d":
        rho, u, p = 0.5 + rng.random(n1), 0.3 * rng.standard_normal(n1), 0.5 + rng.random(n1)
        return 1, O.RP_EULER_1D, 3, 3, [1.4, 0.4], np.stack([rho, rho * u, p / 0.4 + 0.5 * rho * u * u]), None
    if name == "advection_2d":
        return 2, O.RP_ADVECTION_2D, 1, 1, [0.8, -0.6], rng.random((1,) + n2), None
    assert name == "acoustics_2d"
    return 2, O.RP_ACOUSTICS_2D, 3, 2, [1.0, 4.0, 2.0, 2.0], rng.standard_normal((3,) + n2), None


@pytest.mark.gpu
@pytest.mark.parametrize("name,order", [("advection_1d", 5)] + [(n, 7) for n in (
    "advection_1d", "burgers_1d", "advection_color_1d", "shallow_1d", "euler_1d", "advection_2d", "acoustics_2d")])
def test_hip_flux_of_the_solvers_not_run_elsewhere(coracle, name, order):
    """The solvers whose weno_order 7..17 kernels the two tests above do not run (they take euler_5wave_2d and
    acoustics_1d), at order 7 (mbc 4), and advection_1d at order 5, which no other test takes through the component-wise
    kernel: 9 (x 5) cells == the oracle, bit for bit, Courant number included."""
    from pyclaw_amd import _lib as L
    g, mx, my = (order + 1) // 2, 9, 5
    ndim, rp, meqn, mwaves, par, q, aux = _small_case(name, g)
    q = np.asfortranarray(q)
    aux = None if aux is None else np.asfortranarray(aux)
    maux = 0 if aux is None else aux.shape[0]
    p8 = np.array(list(par) + [0.0] * (8 - len(par)))
    dx, dy, dt = 1.0 / mx, 0.8 / my, 0.01 / mx
    dq = np.zeros_like(q)
    cfl = C.c_double()
    coracle.set_weno_order(order)
    if ndim == 1:
        ref, cfl_ref = coracle.sharp_flux1(rp, p8, 2, mwaves, 0, g, mx, q, aux, dx, dt)
        L.check(L.lib().pcl_sharp_flux1(rp, L.d(p8), 2, meqn, mwaves, maux, 0, g, mx, L.d(q), L.d(dq),
                                        None if aux is None else L.d(aux), dx, dt, C.cast(C.byref(cfl), L.dp)))
        inner = (slice(None), slice(g, -g))
    else:
        ref, cfl_ref = coracle.sharp_flux2(rp, p8, 2, mwaves, 0, g, mx, my, q, aux, dx, dy, dt)
        L.check(L.lib().pcl_sharp_flux2(rp, L.d(p8), 2, meqn, mwaves, maux, 0, g, mx, my, L.d(q), L.d(dq), None, dx, dy,
                                        dt, C.cast(C.byref(cfl), L.dp)))
        inner = (slice(None), slice(g, -g), slice(g, -g))
    assert np.isfinite(ref[inner]).all() and np.abs(ref[inner]).max() > 0
    assert np.array_equal(dq[inner], ref[inner]), np.abs(dq[inner] - ref[inner]).max()
    assert cfl.value == cfl_ref and cfl.value > 0


@pytest.mark.gpu
def test_order7_is_refused_for_a_weno5_only_solver():
    """shallow_2d has the SharpClaw kernels of weno_order 5 alone: mbc 4 passes pcl_create and ends in the launch code's
    refusal, before anything is launched (dq stays as it was)."""
    from pyclaw_amd import _lib as L
    g, mx, my = 4, 9, 5
    rng = np.random.default_rng(13)
    h = 0.5 + rng.random((mx + 2 * g, my + 2 * g))
    q = np.asfortranarray(np.stack([h, 0.1 * h, -0.2 * h]))
    dq = np.full_like(q, 7.0)
    cfl = C.c_double()
    rc = L.lib().pcl_sharp_flux2(O.RP_SHALLOW_2D, L.d(np.array([9.81] + [0.0] * 7)), 2, 3, 3, 0, 0, g, mx, my, L.d(q),
                                 L.d(dq), None, 1.0 / mx, 1.0 / my, 0.001, C.cast(C.byref(cfl), L.dp))
    assert rc == L.EINVAL
    assert L.lib().pcl_last_error() == (b"SharpClaw: this Riemann solver is built for weno_order 5 (mbc 3) only; orders 7..17 "
                                        b"exist for the 1-D solvers and for advection_2d, acoustics_2d, euler_5wave_2d")
    assert np.all(dq == 7.0)


@pytest.mark.gpu
def test_acoustics1d_weno17_app(coracle):
    """the reference's weno17 regression through SharpClawSolver1D on the GPU: the gate, and the oracle replay bit for bit"""
    import pyclaw_amd as pyclaw
    from apps import problems
    err, claw = problems.acoustics1D(pyclaw, solver_type='sharpclaw', weno_order=17)
    assert abs(err - 0.000163221216565) < 1e-5, err
    p = D.acoustics1d_problem(solver_type='sharpclaw', weno_order=17, cfl_max=2.5, cfl_desired=2.45)
    D.run(p, coracle, 1.0, 5)
    assert np.array_equal(claw.frames[5].state.q, p.q)


@pytest.mark.gpu
def test_weno_order_validation():
    import pyclaw_amd as pyclaw
    from apps import problems
    with pytest.raises(Exception, match="odd number between 5 and 17"):
        problems.acoustics1D(pyclaw, solver_type='sharpclaw', weno_order=8)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [9, 17])
def test_fast_mode_high_order(coracle, order):
    """fast arithmetic, one right-hand side: the increment dq differs from the oracle's by less than 1e-12 of the
    solution it is added to (dq itself is a small difference of O(1) fluctuations)"""
    from pyclaw_amd import _lib as L
    g, mx, my = (order + 1) // 2, 70, 41
    q = G.euler_state_mild(order, (mx + 2 * g, my + 2 * g))
    dx, dy, dt = 1.0 / mx, 0.8 / my, 1e-4
    coracle.set_weno_order(order)
    ref, _ = coracle.sharp_flux2(O.RP_EULER5_2D, G.PAR, 2, 5, 0, g, mx, my, q, None, dx, dy, dt)
    out, _ = _device_dq(L, _make(L, 2, (mx, my), 11, 5, 5, G.PAR, (dx, dy), g, math=1), q, dt)
    inner = (slice(None), slice(g, -g), slice(g, -g))
    assert np.abs(out[inner] - ref[inner]).max() < 1e-12 * np.abs(q).max()
    assert np.abs(out[inner] - ref[inner]).max() < 1e-10 * np.abs(ref[inner]).max()


@pytest.mark.gpu
def test_fast_mode_weno17_app(coracle):
    """The weno17 regression in fast mode passes the reference's own gate (1e-5 on the one-period error).  It is NOT
    within rtol 1e-12 of the exact-mode result, and cannot be: on this smooth pulse the order-17 smoothness indicators
    (float32 coefficients up to 1e5, alternating signs) are rounding noise, the weights w/(sigma+1e-36)^2 follow that
    noise, and a last-digit difference in any input re-weights the stencils -- measured 8e-5 after one period.  The
    same holds between two builds of the reference itself, which is why its gate is 1e-5."""
    import pyclaw_amd as pyclaw
    from apps import problems
    err, claw = problems.acoustics1D(pyclaw, solver_type='sharpclaw', weno_order=17, math='fast')
    assert abs(err - 0.000163221216565) < 1e-5, err
    p = D.acoustics1d_problem(solver_type='sharpclaw', weno_order=17, cfl_max=2.5, cfl_desired=2.45)
    D.run(p, coracle, 1.0, 5)
    assert np.abs(claw.frames[5].state.q - p.q).max() < 1e-3
