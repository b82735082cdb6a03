"""
CPU: the host recomputation of the column-shortcut count of the one-kernel dimension-split step (classic_fused.hpp,
DESIGN.md 4.1a, round 14), which tests/test_gpu_ycol.py holds pcl_tile_ycol_stats against.  A tile owns 60 x 12 cells of
a 64 x 16 window.  Behind the x sweeps the window holds q* (the x-swept array) in its 60 inner columns, where those are
interior columns of the grid and the row lies inside the array, and the launch's input everywhere else: in its halo
columns, in ghost columns (which the x sweep copies through) and in the rows and columns past the array, which repeat the
last one.  A y sweep takes four columns (a group) into one wavefront, 16 lanes per column, lane = window row.  The group

  is skipped     when none of its columns holds q* (window columns 0-1 / 62-63 hold it only where they are ghost columns);
  is wave-uniform when every lane but lane 0 compares equal (==, all components) to the lane on its left -- today's
                  shortcut, not counted;
  qualifies      when every lane but the first of each column does, the group is not wave-uniform, and no lane whose
                  result is stored (window rows 2-13 and columns 2-61 that are interior cells of the grid) holds a -0 or
                  a non-finite component (bit patterns).

The kernel also sends a wavefront with a non-finite wave speed down the full path; the states of these tests have none.
These tests pin the recomputation itself on states whose counts can be written down by hand, and anchor the reason for
the -0 guard on the oracle alone.
"""
import numpy as np

from oracle import oracle as O

from test_row_reuse_cpu import fill_ghosts, planar, PER

OWN_C, OWN_R, COLS, ROWS, MBC = 60, 12, 64, 16, 2
GROUP = 4
SIGN = np.uint64(0x8000000000000000)
EXPO = np.uint64(0x7ff0000000000000)


def guarded(v):
    """cells (meqn, ...) that hold a -0 or a non-finite component, by their bits"""
    b = np.ascontiguousarray(v).view(np.uint64)
    return ((b == SIGN) | ((b & EXPO) == EXPO)).any(axis=0)


def window(qbc, qx, tx, ty):
    """the 64 x 16 window of tile (tx, ty) as the y sweeps find it, (meqn, 64, 16), with the masks `qstar` (64: the
    column holds q*) and `stored` (64 x 16: the y sweep puts the lane's result back)"""
    I, J = qbc.shape[1:]
    x0, y0 = tx * OWN_C, ty * OWN_R
    c, r = np.arange(COLS), np.arange(ROWS)
    gx, gy = np.minimum(x0 + c, I - 1), np.minimum(y0 + r, J - 1)
    interior_x = (x0 + c >= MBC) & (x0 + c < I - MBC)
    inner = (c >= MBC) & (c < COLS - MBC)
    swept = (inner & interior_x)[:, None] & (y0 + r < J)[None, :]
    w = np.where(swept[None], qx[:, gx][:, :, gy], qbc[:, gx][:, :, gy])
    qstar = (x0 + c < I) & (inner | ~interior_x)
    row_owned = (y0 + r >= MBC) & (y0 + r < J - MBC) & (r >= MBC) & (r < ROWS - MBC)
    stored = (inner & interior_x)[:, None] & row_owned[None, :]
    return w, qstar, stored


def group_kinds(w, qstar, stored):
    """for the 16 groups of a window: 's' skipped, 'u' wave-uniform, 'c' column shortcut, 'g' column-uniform but
    guarded (a -0 or non-finite stored cell: full path), 'f' full path"""
    down = (w[:, :, 1:] == w[:, :, :-1]).all(axis=0)           # (64, 15): row r + 1 equals row r of its column
    across = (w[:, 1:, 0] == w[:, :-1, ROWS - 1]).all(axis=0)  # (63): row 0 equals row 15 of the column before
    bad = guarded(w) & stored
    out = []
    for p in range(COLS // GROUP):
        cs = slice(GROUP * p, GROUP * p + GROUP)
        if not qstar[cs].any():
            out.append('s')
        elif not down[cs].all():
            out.append('f')
        elif across[GROUP * p:GROUP * p + GROUP - 1].all():
            out.append('u')
        else:
            out.append('g' if bad[cs].any() else 'c')
    return out


def ycol_count(qbc, qx):
    """y-sweep calls that take the column shortcut in a launch that computes every tile: qbc the ghost-filled input
    (meqn, mx + 4, my + 4), qx the same array behind the x sweeps (step2ds with idir = 1)"""
    I, J = qbc.shape[1:]
    mx, my = I - 2 * MBC, J - 2 * MBC
    n = 0
    for ty in range((my + OWN_R - 1) // OWN_R):
        for tx in range((mx + OWN_C - 1) // OWN_C):
            n += group_kinds(*window(qbc, qx, tx, ty)).count('c')
    return n


GAMMA = 1.4
PAR = np.array([GAMMA, GAMMA - 1.0])
MTH = np.array([4, 4, 4, 4, 2], dtype=np.int32)
METHOD = np.array([1, 2, -1, 0, 0, 0, 0], dtype=np.int32)


def x_swept(coracle, qbc, dx, dy, dt, both=False):
    """the oracle's dimension-split x sweeps of the ghost-filled array (both: the y sweeps of that as well)"""
    mx, my = qbc.shape[1] - 2 * MBC, qbc.shape[2] - 2 * MBC
    a = np.asfortranarray(qbc)
    out = a.copy("F")
    coracle.step2ds(O.RP_EULER5_2D, PAR, max(mx, my), MBC, mx, my, a, out, None, dx, dy, dt, METHOD, MTH, 1)
    if both:
        coracle.step2ds(O.RP_EULER5_2D, PAR, max(mx, my), MBC, mx, my, out, out, None, dx, dy, dt, METHOD, MTH, 2)
    return out


# ---- the recomputation on arrays written down by hand (qx = qbc: no x sweep needed) ----------------------------------
def ramp(mx, my):
    """every column differs from its neighbours, no variation in y"""
    q = np.empty((5, mx, my))
    i = np.arange(mx, dtype=float)[:, None]
    q[0], q[1], q[2], q[3], q[4] = 1.0 + i / 256.0, 0.25, 0.0, 2.5 + i / 128.0, i / 512.0
    return q


def kinds_of(q, bc=PER, tile=(0, 0), const=None):
    g = fill_ghosts(q, bc, const)
    return "".join(group_kinds(*window(g, g, *tile)))


def test_ramp_every_group_takes_the_shortcut():
    q = ramp(180, 36)
    g = fill_ghosts(q, PER)
    assert kinds_of(q) == "c" * 16 and kinds_of(q, tile=(2, 2)) == "c" * 16
    assert ycol_count(g, g) == 9 * 16


def test_uniform_and_planar_states():
    """one state: wave-uniform everywhere, nothing counted; planar jumps: only the groups that hold a jump between two
    of their columns, or whose first column differs from ... nothing: a group of equal columns is wave-uniform"""
    q = np.broadcast_to(np.array([1.0, 0.0, 0.0, 2.5, 0.0]).reshape(5, 1, 1), (5, 120, 48)).copy()
    g = fill_ghosts(q, PER)
    assert ycol_count(g, g) == 0 and kinds_of(q) == "u" * 16
    q = planar(120, 48)                    # jumps between grid columns 14|15 and 44|45: window columns 16|17 and 46|47
    k = kinds_of(q)
    assert k == "uuuucuuuuuucuuuu", k
    g = fill_ghosts(q, PER)
    assert ycol_count(g, g) == 2 * 4 * 2


def test_halo_columns_are_skipped_off_the_frame_only():
    """window columns 0-3: columns 0-1 hold q* only as ghost columns, but the group runs for columns 2-3 either way;
    past the array's end whole groups are skipped"""
    q = ramp(200, 50)
    out = ('outflow',) * 4
    assert kinds_of(q, out, (0, 0))[0] == "c"
    # tile column 3 of 200 cells: array columns 180 .. 243, the array has 204: window columns 24 .. hold its last column
    k = kinds_of(q, out, (3, 0))
    # ghost columns 202, 203 are window columns 22, 23 (equal to column 21 under outflow; column 20 differs); 24 ..
    # repeat column 203 and hold no q*
    assert k == "c" * 6 + "s" * 10, k


def test_one_odd_cell_only_its_group_computes():
    for row in (0, 1, 2, 13, 14, 15):
        for col in (3, 4, 59, 60, 61, 62):            # window columns 5, 6 | 61, 62, 63 of tile 0 and 1, 2, 3, 4 of tile 1
            q = ramp(180, 36)
            gx, gy = col, 12 + row - MBC              # window row `row` of tile row 1
            q[4, gx, gy] += 0.5
            for tx in (0, 1):
                k = kinds_of(q, tile=(tx, 1))
                wc = gx + MBC - OWN_C * tx
                want = ["c"] * 16
                if 0 <= wc < COLS:
                    want[wc // GROUP] = "f"
                assert k == "".join(want), (row, col, tx, k)


def test_wave_uniform_groups_are_not_counted():
    q = ramp(180, 36)
    q[:, 8:16] = q[:, 8:9]                 # grid columns 8 .. 15 equal: window columns 10 .. 17 of tile 0
    k = kinds_of(q)
    assert k[2] == "c" and k[3] == "u" and k[4] == "c", k      # groups 8-11 (8|9 differ... 10, 11 equal), 12-15, 16-19


def test_guard_minus_zero_and_non_finite_in_stored_lanes_only():
    q = ramp(180, 36)
    q[2, 30, :] = -0.0                     # a whole column, stored rows included
    assert kinds_of(q)[8] == "g" and kinds_of(q).count("c") == 15
    q = ramp(180, 36)
    q[4, 30, :] = np.inf
    assert kinds_of(q)[8] == "g"
    q = ramp(180, 36)
    q[4, 30, :] = np.nan                   # a NaN equals nothing: a jump, not a guarded column
    assert kinds_of(q)[8] == "f"
    # a reflecting lower wall mirrors v = +0 into -0 ghost rows: halo lanes, not stored -- the shortcut stays
    q = ramp(180, 36)
    wall = ('periodic', 'periodic', 'reflecting', 'outflow')
    g = fill_ghosts(q, wall)
    assert np.signbit(g[2, :, :2]).all()
    assert kinds_of(q, wall) == "c" * 16
    # the tracer -0 in the halo columns of a tile is not stored there, but it is in the neighbour
    q = ramp(180, 36)
    q[4, 58:60, :] = -0.0                  # window columns 60, 61 of tile 0 (stored), 0, 1 of tile 1 (halo)
    assert kinds_of(q)[15] == "g" and kinds_of(q, tile=(1, 0))[0] == "c"


def test_rows_past_the_array_repeat_the_last_row():
    """427 x 197: the last tile row's window rows 9 .. 15 repeat row 200; the x-swept rows above differ from it where
    the x sweep changed something"""
    q = ramp(427, 197)
    g = fill_ghosts(q, ('outflow',) * 4)
    qx = g.copy()
    qx[0, MBC:-MBC, :] += 0.125            # stands for an x sweep that changes every interior column
    k = group_kinds(*window(g, qx, 0, 16))
    assert k[0] == "f" and set(k[1:15]) == {"f"}, k
    k = group_kinds(*window(g, qx, 0, 3))
    assert "".join(k) == "c" * 16


# ---- with the oracle -------------------------------------------------------------------------------------------------
def test_planar_front_behind_the_oracles_x_sweep(coracle):
    """the x sweep of equal rows gives equal rows: behind it every group is wave-uniform or takes the shortcut, and the
    smeared jumps reach at least the groups the sharp ones did"""
    mx, my = 180, 36
    q = planar(mx, my)
    g = fill_ghosts(q, PER)
    qx = x_swept(coracle, g, 2.0 / mx, 2.0 / mx, 0.2 / mx)
    assert (qx[:, :, :1] == qx).all() and (qx != g).any()
    for ty in range(3):
        for tx in range(3):
            assert set(group_kinds(*window(g, qx, tx, ty))) == {"u", "c"}, (tx, ty)
    n0, n1 = ycol_count(g, g), ycol_count(g, qx)
    assert n0 == 3 * 3 * 2 and n1 >= n0, (n0, n1)


def test_oracle_full_solve_turns_minus_zero_into_plus_zero(coracle):
    """why the shortcut needs its guard: a state with q[2] = q[4] = -0 comes back all +0 from the reference's step, in
    columns that are constant in y as well -- keeping the cell's bits there would not be the reference's answer"""
    mx, my = 64, 16
    q = ramp(mx, my)
    q[2], q[4] = -0.0, -0.0
    g = fill_ghosts(q, PER)
    assert np.signbit(g[2]).all() and np.signbit(g[4]).all()
    out = x_swept(coracle, g, 2.0 / mx, 2.0 / mx, 0.2 / mx, both=True)[:, MBC:-MBC, MBC:-MBC]
    assert (out[2] == 0.0).all() and not np.signbit(out[2]).any()
    assert not np.signbit(out[4]).any()
