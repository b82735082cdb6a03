r"""
Explicit Runge-Kutta schemes as Butcher tableaus, for ``SharpClawSolver.time_integrator``.

A scheme with ``s`` stages is ``(a, b, c)``: ``a`` strictly lower triangular ``s x s``, ``b`` and ``c`` of length ``s``,

    y_i = q + sum_{j<i} a_ij K_j,    K_i = dt L(y_i, t + c_i dt),    q <- q + sum_j b_j K_j.

``TABLEAUS`` is the one table of the named schemes; ``time_integrator = 'RK'`` takes ``solver.a``, ``solver.b`` and
``solver.c`` (the spelling of upstream PyClaw) through ``validate``.  Both run through the same step.  The coefficients
are written as the quotients of their sources, so that each is the correctly rounded double of its rational.
"""
import numpy as np

MAX_STAGES = 16


def _tableau(a, b, c, order):
    s = len(b)
    A = np.zeros((s, s))
    for i, row in enumerate(a):
        A[i, :len(row)] = row
    return {'a': A, 'b': np.array(b, dtype=np.float64), 'c': np.array(c, dtype=np.float64), 'order': order}


TABLEAUS = {
    # Heun's method, the two-stage second-order SSP scheme
    'SSP22': _tableau([[], [1.]], [1. / 2., 1. / 2.], [0., 1.], 2),
    # the classical fourth-order method
    'RK44': _tableau([[], [1. / 2.], [0., 1. / 2.], [0., 0., 1.]],
                     [1. / 6., 1. / 3., 1. / 3., 1. / 6.], [0., 1. / 2., 1. / 2., 1.], 4),
    # the six stages of Dormand and Prince's fifth-order solution (J. Comput. Appl. Math. 6 (1980), 19-26); the seventh,
    # which only feeds the embedded fourth-order estimate, is not evaluated: no step-size control
    'DP5': _tableau([[],
                     [1. / 5.],
                     [3. / 40., 9. / 40.],
                     [44. / 45., -56. / 15., 32. / 9.],
                     [19372. / 6561., -25360. / 2187., 64448. / 6561., -212. / 729.],
                     [9017. / 3168., -355. / 33., 46732. / 5247., 49. / 176., -5103. / 18656.]],
                    [35. / 384., 0., 500. / 1113., 125. / 192., -2187. / 6784., 11. / 84.],
                    [0., 1. / 5., 3. / 10., 4. / 5., 8. / 9., 1.], 5),
}


def validate(a, b, c):
    """The tableau of ``time_integrator = 'RK'`` as float64 arrays ``(a, b, c)``, or a ``ValueError`` that says what is wrong
    with it.  ``c`` is taken as given: it need not equal the row sums of ``a``."""
    for name, v in (('a', a), ('b', b), ('c', c)):
        if v is None:
            raise ValueError("time_integrator = 'RK' needs solver.a, solver.b and solver.c: solver.%s is not set" % name)
    try:
        a, b, c = (np.array(v, dtype=np.float64) for v in (a, b, c))
    except (TypeError, ValueError):
        raise ValueError("time_integrator = 'RK': solver.a, solver.b and solver.c must be arrays of numbers")
    if b.ndim != 1 or a.ndim != 2 or c.ndim != 1 or a.shape != (b.size, b.size) or c.shape != b.shape:
        raise ValueError("time_integrator = 'RK': shapes do not agree: solver.a is %s, solver.b %s, solver.c %s; "
                         "s stages need (s, s), (s,) and (s,)" % (a.shape, b.shape, c.shape))
    s = b.size
    if s < 1 or s > MAX_STAGES:
        raise ValueError("time_integrator = 'RK': %d stages; 1 to %d are served" % (s, MAX_STAGES))
    if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
        raise ValueError("time_integrator = 'RK': the tableau has an entry that is not finite")
    if np.triu(a).any():
        i, j = np.argwhere(np.triu(a))[0]
        raise ValueError("time_integrator = 'RK': solver.a[%d, %d] = %r is on or above the diagonal: an implicit tableau; "
                         "only explicit schemes (strictly lower triangular a) are served" % (i, j, a[i, j]))
    if c[0] != 0.0:
        raise ValueError("time_integrator = 'RK': solver.c[0] = %r; the first stage of an explicit scheme is evaluated at "
                         "t, so c[0] must be 0" % c[0])
    return a, b, c
