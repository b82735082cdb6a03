"""
The step of a Runge-Kutta scheme given by its Butcher tableau, restated in numpy on the oracle driver's Problem record: the
expected value of tests/test_rk_cpu.py and tests/test_gpu_rk.py.  TEST INFRASTRUCTURE ONLY.

    y_i = q + sum_{j<i} a_ij K_j,   K_i = dt L(y_i, t + c_i dt),   q <- q + sum_j b_j K_j

K_i is oracle.driver.sharp_dq: the ghost fill of the stage at the stage time, the oracle's sharp_flux1 / sharp_flux2, and
the problem's dq_src added on.  A combination starts from its first operand and adds the terms from left to right, each
product rounded before its sum; a coefficient of exactly 0.0 is no term, every other one is multiplied, 1.0 included.
"""
import numpy as np

from oracle import driver as D


def lincomb(A, coef, K):
    r = A
    for j, cj in enumerate(coef):
        if cj != 0.0:
            r = r + cj * K[j]
    return r


def rk_step(p, backend, a, b, c, times=None):
    """One step of the Problem p (set up by driver.setup) from p.t with p.dt.  Returns the stages' Courant numbers; p.q
    and p.t are advanced unless a stage exceeded p.cfl_max, in which case the list ends with that stage's number and p is
    as it was.  times(t, dt, i) replaces the stage time t + c[i] dt (to state what a wrong one would give)."""
    q, t, dt = p.q, p.t, p.dt
    K, cfls = [], []
    for i in range(len(b)):
        y = q if i == 0 else lincomb(q, a[i][:i], K)
        ti = t + c[i] * dt if times is None else times(t, dt, i)
        try:
            K.append(D.sharp_dq(p, backend, y, ti))
        except D.CFLError:
            cfls.append(p.cfl)
            return cfls
        cfls.append(p.cfl)
    p.q = lincomb(q, b, K)
    p.t = t + dt
    return cfls
