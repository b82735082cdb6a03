"""
CPU: the host recomputation of the row-reuse count of the one-kernel dimension-split step (classic_fused.hpp, DESIGN.md
4.1a, round 13), which tests/test_gpu_row_reuse.py holds pcl_tile_rowreuse_stats against.  A tile owns 60 x 12 cells of a
64 x 16 window; wavefront w of a tile sweeps the window rows 2w, 2w+1, 8+2w, 9+2w in that order and reuses a sweep whose
row -- all components, all 64 columns, halo columns included -- holds the same BITS as the row before it in that order.
Rows at or past the array's end are not swept; columns past it repeat the last one.  These tests pin the recomputation
itself on states whose counts can be written down by hand.
"""
import numpy as np

OWN_C, OWN_R, COLS, ROWS, MBC = 60, 12, 64, 16, 2
WAVES = 4


def wave_rows(w):
    return (2 * w, 2 * w + 1, 8 + 2 * w, 9 + 2 * w)


def fill_ghosts(q, bc, const=None):
    """q (meqn, mx, my) -> the array with two ghost cells per side as the step sees it: x sides first, then y sides over
    the x-filled array.  bc = (x lower, x upper, y lower, y upper), each 'periodic', 'outflow', 'reflecting' (mirror,
    the normal momentum -- component 1 in x, 2 in y -- negated: +0 becomes -0) or 'const' (the state `const`)."""
    meqn, mx, my = q.shape
    a = np.zeros((meqn, mx + 2 * MBC, my + 2 * MBC))
    a[:, MBC:-MBC, MBC:-MBC] = q
    for dim in (0, 1):
        v = a if dim == 0 else a.swapaxes(1, 2)          # v[m, k, :]: k runs along the dimension being filled
        n = v.shape[1]
        for side, kind in ((0, bc[2 * dim]), (1, bc[2 * dim + 1])):
            for g in range(MBC):
                k = g if side == 0 else n - MBC + g
                if kind == 'const':
                    v[:, k, :] = np.asarray(const, dtype=float).reshape(meqn, 1)
                    continue
                if kind == 'outflow':
                    src = MBC if side == 0 else n - MBC - 1
                elif kind == 'periodic':
                    src = n - 2 * MBC + k if side == 0 else k - (n - 2 * MBC)
                elif kind == 'reflecting':
                    src = 2 * MBC - 1 - k if side == 0 else 2 * (n - MBC) - 1 - k
                else:
                    raise ValueError(kind)
                v[:, k, :] = v[:, src, :]
                if kind == 'reflecting':
                    v[1 + dim, k, :] = -v[1 + dim, k, :]
    return a


def reuse_count(qbc, bitwise=True):
    """x sweeps a launch that computes every tile reuses on the ghost-filled array qbc (meqn, mx + 4, my + 4);
    bitwise=False compares with == instead (+0 equals -0, a NaN nothing): NOT the kernel's rule, for contrast"""
    I, J = qbc.shape[1:]
    mx, my = I - 2 * MBC, J - 2 * MBC
    ntx, nty = (mx + OWN_C - 1) // OWN_C, (my + OWN_R - 1) // OWN_R
    v = np.ascontiguousarray(qbc).view(np.uint64) if bitwise else qbc
    n = 0
    for ty in range(nty):
        for tx in range(ntx):
            x0, y0 = tx * OWN_C, ty * OWN_R
            cols = np.minimum(x0 + np.arange(COLS), I - 1)
            for w in range(WAVES):
                rows = wave_rows(w)
                for k in range(1, len(rows)):
                    if y0 + rows[k] >= J:
                        continue
                    n += bool((v[:, cols, y0 + rows[k]] == v[:, cols, y0 + rows[k - 1]]).all())
    return n


def planar(mx, my, period=60):
    """a Sod-type jump in x every period / 2 cells (one inside every tile column), no variation in y"""
    left, right = (1.0, 0.0, 0.0, 2.5, 0.0), (0.125, 0.0, 0.0, 0.25, 1.0)
    q = np.empty((5, mx, my))
    half = period // 2
    hi = ((np.arange(mx) + half // 2) // half) % 2 == 1
    for m in range(5):
        q[m] = np.where(hi, right[m], left[m])[:, None]
    return q


PER = ('periodic',) * 4


def test_wave_rows_cover_the_window_once():
    assert sorted(r for w in range(WAVES) for r in wave_rows(w)) == list(range(ROWS))


def test_planar_front_full_tiles():
    q = planar(120, 48)
    assert (q[:, :60] != q[:, 1:61]).any(axis=(0, 2)).sum() >= 2          # jumps inside tile column 0
    assert reuse_count(fill_ghosts(q, PER)) == 2 * 4 * WAVES * 3


def test_one_odd_row_positions():
    """row j of the grid is window row j + 2 - 12 ty of tile row ty (and of its neighbours' halo): every position in a
    wavefront's order breaks one or two links of one chain per tile that holds it"""
    base = planar(120, 48)
    for j in range(24):
        q = base.copy()
        q[4, :, j] += 0.25
        links = 0                     # links broken: (row, row before it in the wavefront's order) pairs that hold row j
        for ty in range(4):
            for w in range(WAVES):
                rows = [12 * ty + r - 2 for r in wave_rows(w)]          # grid rows, -2 .. 49 (periodic)
                rows = [r % 48 for r in rows]
                links += sum(1 for k in range(1, 4) if (rows[k] == j) != (rows[k - 1] == j))
        assert reuse_count(fill_ghosts(q, PER)) == 96 - 2 * links, j    # two tile columns


def test_signed_zero_is_another_row():
    q = planar(120, 48)
    q[2, :, 17] = -0.0
    g = fill_ghosts(q, PER)
    assert reuse_count(g, bitwise=False) == 96 and reuse_count(g) < 96
    r = np.zeros((5, 120, 48))
    r[0], r[3] = 1.0, 2.5
    r[4, 30:90] = 1.0
    r[1, :, 5] = -0.0
    g = fill_ghosts(r, PER)
    assert reuse_count(g, bitwise=False) == 96 and reuse_count(g) < 96


def test_equal_nan_bits_are_equal_rows():
    q = planar(120, 48)
    q[4, 7, :] = np.nan
    g = fill_ghosts(q, PER)
    assert reuse_count(g) == 96 and reuse_count(g, bitwise=False) == 48    # == fails in tile column 0 only


def test_halo_columns_count():
    """a cell of the neighbour tile that the window reads: rows equal in the 60 owned columns still differ"""
    base = planar(120, 48)
    full = reuse_count(fill_ghosts(base, PER))
    for x, tiles in ((58, 2), (59, 2), (60, 2), (61, 2), (57, 1), (62, 1), (30, 1)):
        q = base.copy()
        q[0, x, 17] += 0.5
        # grid row 17 is window row 7 of tile row 1 alone: wavefront 3's rows 6, 7, 14, 15 lose two links per tile
        assert reuse_count(fill_ghosts(q, PER)) == full - 2 * tiles, x


def test_reflecting_wall_ghost_rows():
    """zero normal momentum: the mirrored ghost rows hold -0 and chain with each other, not with the +0 rows"""
    q = planar(120, 48)
    g = fill_ghosts(q, ('periodic', 'periodic', 'reflecting', 'outflow'))
    assert np.signbit(g[2, :, :2]).all() and not np.signbit(g[2, :, 2:]).any()
    assert reuse_count(g, bitwise=False) == 96
    assert reuse_count(g) == 96 - 2                     # tile row 0, wavefront 0: the link from row 1 to row 8, two tiles
    q[2] = -0.3
    g = fill_ghosts(q, ('periodic', 'periodic', 'reflecting', 'outflow'))
    assert reuse_count(g) == 96 - 2 and reuse_count(g, bitwise=False) == 96 - 2


def test_partial_tiles():
    """427 x 197: 8 x 17 tiles; the last tile row owns 5 rows, its window rows 9.. lie past the array's 201 rows"""
    q = planar(427, 197)
    g = fill_ghosts(q, ('outflow',) * 4)
    swept = 0
    for ty in range(17):
        for w in range(WAVES):
            swept += max(0, sum(1 for r in wave_rows(w) if 12 * ty + r < 201) - 1)
    assert swept == 16 * 12 + (2 + 1 + 1 + 1)
    assert reuse_count(g) == 8 * swept


def test_const_inflow_fill():
    q = planar(120, 48)
    inflow = (1.2, 0.5, 0.0, 3.0, 0.0)
    g = fill_ghosts(q, ('const', 'outflow', 'outflow', 'outflow'), inflow)
    assert (g[:, :2, :] == np.array(inflow).reshape(5, 1, 1)).all()          # corners: the y fill copies the x-filled rows
    assert reuse_count(g) == 96
