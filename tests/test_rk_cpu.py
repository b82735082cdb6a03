"""
CPU: explicit Runge-Kutta schemes from a Butcher tableau (pyclaw_amd/rk_tableaus.py, SharpClawSolver.time_integrator =
'RK' / 'SSP22' / 'RK44' / 'DP5'): what setup() refuses, the order conditions of the named tableaus evaluated from the
table itself, the scheme's arithmetic restated in numpy on the oracle (tests/rk_reference.py, the expected value of
tests/test_gpu_rk.py) with its temporal order observed by Richardson differences, and the three C entry points in header,
library and binding table.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rk_reference as RK
from oracle import driver as D
from oracle import oracle as O
from pyclaw_amd import rk_tableaus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- 1: validation ----------------------------------------------------------------------------------------------------------
def solver_with(**attrs):
    import pyclaw_amd as pyclaw
    s = pyclaw.SharpClawSolver1D()
    s.time_integrator = 'RK'
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


HEUN = dict(a=[[0., 0.], [1., 0.]], b=[0.5, 0.5], c=[0., 1.])


@pytest.mark.parametrize("change,words", [
    (dict(a=None), "solver.a is not set"),
    (dict(b=None), "solver.b is not set"),
    (dict(c=None), "solver.c is not set"),
    (dict(b=[0.5, 0.25, 0.25]), "shapes do not agree"),
    (dict(c=[0.]), "shapes do not agree"),
    (dict(a=[[0., 0.], [1., 0.], [0., 0.]]), "shapes do not agree"),
    (dict(a=[[0.5, 0.], [1., 0.]]), "implicit tableau"),
    (dict(a=[[0., 0.25], [1., 0.]]), "implicit tableau"),
    (dict(a=np.tril(np.ones((17, 17)), -1), b=np.ones(17) / 17, c=np.arange(17) / 17.), "17 stages; 1 to 16"),
    (dict(a=[[0., 0.], [float('nan'), 0.]]), "not finite"),
    (dict(b=[0.5, float('inf')]), "not finite"),
    (dict(c=[0.25, 1.]), "c[0] must be 0"),
])
def test_malformed_tableau_is_refused_with_its_reason(change, words):
    """setup(None) raises while it validates: before the solution is looked at and before any library call"""
    attrs = dict(HEUN)
    attrs.update(change)
    with pytest.raises(ValueError) as e:
        solver_with(**{k: v for k, v in attrs.items() if v is not None}).setup(None)
    assert words in str(e.value), str(e.value)


def test_messages_are_distinct_and_unknown_name_keeps_the_old_one():
    import pyclaw_amd as pyclaw
    cases = [dict(a=None), dict(b=[1.]), dict(a=[[0.5, 0.], [1., 0.]]), dict(a=[[0., 0.], [float('nan'), 0.]]),
             dict(a=np.tril(np.ones((17, 17)), -1), b=np.ones(17) / 17, c=np.arange(17) / 17.)]
    seen = set()
    for change in cases:
        attrs = dict(HEUN)
        attrs.update(change)
        with pytest.raises(ValueError) as e:
            solver_with(**{k: v for k, v in attrs.items() if v is not None}).setup(None)
        seen.add(str(e.value))
    assert len(seen) == len(cases)
    s = pyclaw.SharpClawSolver1D()
    s.time_integrator = 'RK45'
    with pytest.raises(Exception) as e:
        s.setup(None)
    assert str(e.value) == 'Unrecognized time integrator' and not isinstance(e.value, ValueError)


def test_c_is_taken_as_given():
    a, b, c = rk_tableaus.validate([[0., 0.], [1., 0.]], [0.5, 0.5], [0., 0.75])
    assert c[1] == 0.75 and a.dtype == b.dtype == c.dtype == np.float64


def test_named_tableaus_pass_validation():
    assert set(rk_tableaus.TABLEAUS) == {'SSP22', 'RK44', 'DP5'}
    for name, tab in rk_tableaus.TABLEAUS.items():
        a, b, c = rk_tableaus.validate(tab['a'], tab['b'], tab['c'])
        assert len(b) == {'SSP22': 2, 'RK44': 4, 'DP5': 6}[name]
        # the stage times of the named schemes are the row sums, to rounding
        assert np.abs(a.sum(axis=1) - c).max() <= 8 * EPS * np.abs(a).sum(axis=1).max()


# ---- 2: order conditions ----------------------------------------------------------------------------------------------------
def trees(A, b):
    """(order, name, value, 1 / gamma) of the rooted trees up to order 5, with c = A 1"""
    c = A.sum(axis=1)
    Ac = A @ c
    return [
        (1, "b.1", b.sum(), 1.),
        (2, "b.c", b @ c, 1. / 2.),
        (3, "b.c^2", b @ c ** 2, 1. / 3.),
        (3, "b.Ac", b @ Ac, 1. / 6.),
        (4, "b.c^3", b @ c ** 3, 1. / 4.),
        (4, "b.(c*Ac)", b @ (c * Ac), 1. / 8.),
        (4, "b.Ac^2", b @ (A @ c ** 2), 1. / 12.),
        (4, "b.AAc", b @ (A @ Ac), 1. / 24.),
        (5, "b.c^4", b @ c ** 4, 1. / 5.),
        (5, "b.(c^2*Ac)", b @ (c ** 2 * Ac), 1. / 10.),
        (5, "b.(c*Ac^2)", b @ (c * (A @ c ** 2)), 1. / 15.),
        (5, "b.(c*AAc)", b @ (c * (A @ Ac)), 1. / 30.),
        (5, "b.(Ac*Ac)", b @ (Ac * Ac), 1. / 20.),
        (5, "b.Ac^3", b @ (A @ c ** 3), 1. / 20.),
        (5, "b.A(c*Ac)", b @ (A @ (c * Ac)), 1. / 40.),
        (5, "b.AAc^2", b @ (A @ (A @ c ** 2)), 1. / 60.),
        (5, "b.AAAc", b @ (A @ (A @ Ac)), 1. / 120.),
    ]


@pytest.mark.parametrize("name", ['SSP22', 'RK44', 'DP5'])
def test_order_conditions(name):
    """Every tree up to the stated order, residual <= 64 eps sum|terms|: the sum of the absolute values of the expanded
    products is the same expression in |a| and |b| (c its row sums), computed here.  The first tree of the next order
    fails by far more than that: the stated order is not an understatement either."""
    tab = rk_tableaus.TABLEAUS[name]
    A, b, p = tab['a'], tab['b'], tab['order']
    checked = 0
    for (order, what, value, rhs), (_, _, mag, _) in zip(trees(A, b), trees(np.abs(A), np.abs(b))):
        if order <= p:
            print("%s order %d %-12s residual %.3e bound %.3e" % (name, order, what, abs(value - rhs), 64 * EPS * mag))
            assert abs(value - rhs) <= 64 * EPS * mag, (name, what, value, rhs)
            checked += 1
    assert checked == {2: 2, 4: 8, 5: 17}[p]
    if p < 5:
        worst = max(abs(value - rhs) for order, _, value, rhs in trees(A, b) if order == p + 1)
        assert worst > 1e-3


# ---- 3: the arithmetic of the step, and its temporal order ------------------------------------------------------------------
def advection_problem(mx=64):
    x = D.centers(0.0, 1.0, mx)
    q = np.empty((1, mx), order="F")
    q[0] = np.sin(2 * np.pi * x) + 0.5 * np.cos(4 * np.pi * x)
    p = D.Problem(q=q, d=(1.0 / float(mx),), rp=O.RP_ADVECTION_1D, rp_params=[1.0], mwaves=1, limiters=[1],
                  bc_lower=[D.PERIODIC], bc_upper=[D.PERIODIC], solver_type='sharpclaw', cfl_max=2.5, cfl_desired=2.45)
    D.setup(p)
    return p


def advance(coracle, name, nsteps, T=0.25):
    tab = rk_tableaus.TABLEAUS[name]
    p = advection_problem()
    p.dt = T / nsteps
    for n in range(nsteps):
        cfls = RK.rk_step(p, coracle, tab['a'], tab['b'], tab['c'])
        assert len(cfls) == len(tab['b']) and max(cfls) <= 0.5 + 1e-12
    return p.q


@pytest.mark.parametrize("name", ['SSP22', 'RK44', 'DP5'])
def test_temporal_order_by_richardson_differences(coracle, name):
    """WENO5 advection on ONE grid (64 cells), T = 0.25 in 32, 64 and 128 equal steps: the spatial error is the same in all
    three and cancels in the differences, which shrink with the scheme's temporal order.  A wrong coefficient costs at
    least one order, so the gate is the midpoint p - 0.5."""
    u32, u64, u128 = (advance(coracle, name, n) for n in (32, 64, 128))
    d1, d2 = np.abs(u32 - u64).max(), np.abs(u64 - u128).max()
    observed = np.log2(d1 / d2)
    print("%s: |u32-u64| = %.3e, |u64-u128| = %.3e, observed order %.3f" % (name, d1, d2, observed))
    assert d2 > 1e-10                   # far above round-off
    assert observed >= rk_tableaus.TABLEAUS[name]['order'] - 0.5


def test_reference_step_with_euler_tableau_is_the_drivers_euler(coracle):
    """a = [[0]], b = [1]: the restated step is q + dq, the driver's 'Euler' bit for bit"""
    p1, p2 = advection_problem(), advection_problem()
    p1.dt = p2.dt = 0.2 / 64
    p2.time_integrator = 'Euler'
    for n in range(3):
        RK.rk_step(p1, coracle, [[0.]], [1.], [0.])
        D.sharp_step(p2, coracle)
    assert np.array_equal(p1.q, p2.q) and np.abs(p1.q - advection_problem().q).max() > 0


def test_reference_combination_skips_zeros_and_goes_left_to_right():
    K = [np.array([1e16]), np.array([np.nan]), np.array([-1e16]), np.array([3.0])]
    got = RK.lincomb(np.array([1.0]), [1.0, 0.0, 1.0, 1.0], K)
    assert got[0] == ((1.0 + 1e16) - 1e16) + 3.0          # K[1] is not read; the order is left to right


# ---- 4: ABI -----------------------------------------------------------------------------------------------------------------
def test_new_entry_points_in_header_library_and_bindings():
    from pyclaw_amd import _lib
    text = open(os.path.join(ROOT, "include", "pyclaw_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("pcl_rk_stages", "pcl_rk_take", "pcl_rk_lincomb"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert hasattr(L, name)
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == len(m.group(1).split(","))
        # pointer arguments in the header are pointer types in the table, the others are not
        for decl, ty in zip(m.group(1).split(","), argtypes):
            assert ("*" in decl) == (ty is C.c_void_p or hasattr(ty, "contents") or ty in (_lib.ip, _lib.dp)), (name, decl, ty)
    assert re.search(r"#define\s+PCL_RK_MAX_STAGES\s+16\b", text) and rk_tableaus.MAX_STAGES == 16


def test_entry_points_refuse_a_null_handle():
    from pyclaw_amd import _lib
    L = _lib.lib()
    assert L.pcl_rk_stages(None, 2, None) == _lib.EINVAL
    assert L.pcl_rk_take(None, 0) == _lib.EINVAL
    assert L.pcl_rk_lincomb(None, 0, 0, 0, None, None) == _lib.EINVAL
