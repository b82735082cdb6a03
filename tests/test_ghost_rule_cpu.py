"""
CPU: the ghost-cell rule (csrc/ghost_rule.hpp: vbc_map) through its pure-host entry point pcl_ghost_map, against the rule
restated in numpy slices as the reference's solver.py:404-452 applies it -- the lower side, then the upper side.

pcl_ghost_map(k, n, mbc, lo, hi, out) answers for cell k of a dimension of n cells (ghosts included): out = (source
cell, negate the normal momentum, constant state, side).  A side's answers are applied the way qbc_lower / qbc_upper
assign: gathered from the array as the side before left it, then stored.  (Where the interior is shorter than mbc an
upper reflecting side reads lower ghost cells, so the order of the sides shows; from mbc interior cells on a single
gather from the unfilled array gives the same, which is how the kernels evaluate the rule while loading.)
"""
import itertools

import numpy as np
import pytest

CUSTOM, OUTFLOW, PERIODIC, REFLECTING = 0, 1, 2, 3
TYPES = [-1, CUSTOM, OUTFLOW, PERIODIC, REFLECTING]


def fill_side(qbc, idim, mbc, side, bctype, cst=None, negate=True):
    """solver.py:404-452 for one side of dimension idim of qbc[m, i(, j(, k))], in place.  bctype < 0: nothing;
    CUSTOM: the constant state cst[m]; negate=False: the aux rule (reflecting copies, solver.py:497-548)."""
    q = np.moveaxis(qbc, idim + 1, 1)       # a view, like solver.py's rollaxis
    g = mbc
    if bctype < 0:
        return
    if bctype == CUSTOM:
        sl = slice(0, g) if side == 0 else slice(q.shape[1] - g, q.shape[1])
        q[:, sl, ...] = np.asarray(cst).reshape((-1,) + (1,) * (q.ndim - 1))[:q.shape[0]]
    elif bctype == OUTFLOW:
        if side == 0:
            q[:, :g, ...] = q[:, g:g + 1, ...]
        else:
            q[:, -g:, ...] = q[:, -g - 1:-g, ...]
    elif bctype == PERIODIC:
        if side == 0:
            q[:, :g, ...] = q[:, -2 * g:-g, ...].copy()
        else:
            q[:, -g:, ...] = q[:, g:2 * g, ...].copy()
    elif bctype == REFLECTING:
        if side == 0:
            src = q[:, 2 * g - 1:g - 1:-1, ...].copy()
        else:
            src = q[:, -g - 1:-2 * g - 1:-1, ...].copy()
        if negate and idim + 1 < q.shape[0]:
            src[idim + 1] = -src[idim + 1]
        if side == 0:
            q[:, :g, ...] = src
        else:
            q[:, -g:, ...] = src
    else:
        raise ValueError(bctype)


def ghost_map(L, k, n, mbc, lo, hi):
    out = np.zeros(4, dtype=np.int32)
    L.check(L.lib().pcl_ghost_map(k, n, mbc, lo, hi, L.i(out)))
    return tuple(int(v) for v in out)


def apply_map(L, q, mbc, lo, hi, cst):
    """q[m, n] through pcl_ghost_map: lower side's cells, then the upper side's; component 1 is the normal momentum"""
    n = q.shape[1]
    out = q.copy()
    for cells in (range(0, mbc), range(n - mbc, n)):
        before = out.copy()
        for k in cells:
            src, neg, is_cst, side = ghost_map(L, k, n, mbc, lo, hi)
            if is_cst:
                out[:, k] = cst[side][:q.shape[0]]
            else:
                out[:, k] = before[:, src]
                if neg and q.shape[0] > 1:
                    out[1, k] = -before[1, src]
    return out


@pytest.mark.parametrize("mbc", [2, 3, 5])
@pytest.mark.parametrize("interior", [1, 2, 3, 7])
def test_ghost_map_equals_numpy_rule(mbc, interior):
    from pyclaw_amd import _lib as L
    n = interior + 2 * mbc
    cst = np.array([[1000.0, 1001.0], [2000.0, 2001.0]])
    for ncomp in (1, 2):            # distinct values; the two-component twin carries the sign
        q = np.arange(1.0, 1.0 + ncomp * n).reshape(ncomp, n)
        for lo, hi in itertools.product(TYPES, TYPES):
            want = q.copy()
            fill_side(want, 0, mbc, 0, lo, cst[0])
            fill_side(want, 0, mbc, 1, hi, cst[1])
            got = apply_map(L, q, mbc, lo, hi, cst)
            assert np.array_equal(got, want), (ncomp, lo, hi, got, want)
            # interior cells, and every cell of a side without a fill, map to themselves
            for k in range(n):
                src, neg, is_cst, side = ghost_map(L, k, n, mbc, lo, hi)
                ghost = (k < mbc and lo >= 0) or (k >= n - mbc and hi >= 0)
                if not ghost:
                    assert (src, neg, is_cst) == (k, 0, 0), (k, lo, hi)
                else:
                    assert side == (0 if k < mbc else 1)
                    assert is_cst == ((lo if side == 0 else hi) == CUSTOM)
                    assert neg == ((lo if side == 0 else hi) == REFLECTING)
            if interior >= mbc:
                # one gather from the unfilled array (the kernels' evaluation while loading) is the same fill
                once = q.copy()
                for k in range(n):
                    src, neg, is_cst, side = ghost_map(L, k, n, mbc, lo, hi)
                    once[:, k] = cst[side][:ncomp] if is_cst else q[:, src]
                    if neg and ncomp > 1:
                        once[1, k] = -q[1, src]
                assert np.array_equal(once, want), (ncomp, lo, hi)


def test_numpy_rule_is_the_reference_loop():
    """the slices above against solver.py's own cell loops (:406-415, :441-450), written out for one dimension"""
    rng = np.random.default_rng(0)
    for mbc, interior in itertools.product([2, 3, 5], [1, 2, 3, 7]):
        n = interior + 2 * mbc
        for bctype, side in itertools.product([OUTFLOW, PERIODIC, REFLECTING], [0, 1]):
            q = rng.standard_normal((2, n))
            want = q.copy()
            for i in range(mbc):
                if bctype == OUTFLOW and side == 0:
                    want[:, i] = want[:, mbc]
                elif bctype == OUTFLOW:
                    want[:, -i - 1] = want[:, -mbc - 1]
                elif bctype == REFLECTING and side == 0:
                    want[:, i] = want[:, 2 * mbc - 1 - i]
                    want[1, i] = -want[1, 2 * mbc - 1 - i]
                elif bctype == REFLECTING:
                    want[:, -i - 1] = want[:, -2 * mbc + i]
                    want[1, -i - 1] = -want[1, -2 * mbc + i]
            if bctype == PERIODIC and side == 0:
                want[:, :mbc] = q[:, -2 * mbc:-mbc]
            elif bctype == PERIODIC:
                want[:, -mbc:] = q[:, mbc:2 * mbc]
            got = q.copy()
            fill_side(got, 0, mbc, side, bctype)
            assert np.array_equal(got, want), (mbc, interior, bctype, side)


def test_ghost_map_rejects_bad_arguments():
    from pyclaw_amd import _lib as L
    out = np.zeros(4, dtype=np.int32)
    f = L.lib().pcl_ghost_map
    assert f(0, 9, 2, OUTFLOW, OUTFLOW, None) == L.EINVAL
    assert f(-1, 9, 2, OUTFLOW, OUTFLOW, L.i(out)) == L.EINVAL
    assert f(9, 9, 2, OUTFLOW, OUTFLOW, L.i(out)) == L.EINVAL
    assert f(0, 4, 2, OUTFLOW, OUTFLOW, L.i(out)) == L.EINVAL       # no interior cell
    assert f(0, 9, 0, OUTFLOW, OUTFLOW, L.i(out)) == L.EINVAL
    assert f(0, 9, 2, 4, OUTFLOW, L.i(out)) == L.EINVAL             # the sphere mirror is no index rule of one dimension
    assert f(0, 9, 2, OUTFLOW, 7, L.i(out)) == L.EINVAL
