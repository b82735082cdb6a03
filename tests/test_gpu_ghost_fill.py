"""
GPU: the ghost-fill launches of the stateful ABI (pcl_bc, pcl_bc_const, pcl_bc_aux, PCL_BC_SPHERE_MIRROR) against the
rule of solver.py:404-452 restated in numpy slices (tests/test_ghost_rule_cpu.py: fill_side), bit for bit, every
other cell untouched.  1-D, 2-D and 3-D grids whose interior extents are at least mbc, so that the in-place periodic
fill never reads a cell another thread writes.

The aux array's ghost cells cannot be read back through the ABI (pcl_get_cells takes interior cells only), so
pcl_bc_aux is checked through what it feeds: one sweep along the filled dimension after pcl_put_aux of unfilled data +
pcl_bc_aux equals the oracle's sweep over the aux array filled by the numpy rule (reflecting does NOT negate an aux
component), and the oracle's sweep over the unfilled aux array gives something else.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from test_ghost_rule_cpu import CUSTOM, OUTFLOW, PERIODIC, REFLECTING, fill_side

pytestmark = pytest.mark.gpu

SPHERE_MIRROR = 4
# (Riemann solver, meqn, mwaves) with a momentum component in every direction; the grids of the three dimensions
PLAIN = {1: (O.RP_ACOUSTICS_1D, 2, 2), 2: (O.RP_ACOUSTICS_2D, 3, 2), 3: (O.RP_VC_ACOUSTICS_3D, 4, 2)}
GRID = {1: (7,), 2: (7, 5), 3: (5, 4, 3)}
CASES = [(1, 2), (1, 3), (2, 2), (2, 3), (3, 2)]            # (ndim, mbc): 3-D accepts mbc = 2 only


def make_solver(L, ndim, mbc, rp, meqn, mwaves, maux=0, fwave=0):
    cfg = L.Config()
    cfg.ndim = ndim
    for k, n in enumerate(GRID[ndim]):
        cfg.n[k] = n
        cfg.d[k] = 1.0 / n
    cfg.mbc = mbc
    cfg.meqn, cfg.mwaves, cfg.rp = meqn, mwaves, rp
    cfg.maux = maux
    cfg.fwave = fwave
    cfg.method[1] = 2
    cfg.method[2] = -1 if ndim > 1 else 0
    cfg.method[6] = maux
    for k in range(mwaves):
        cfg.mthlim[k] = 4
    cfg.rp_params[:4] = [1.0, 4.0, 2.0, 2.0]                # rho, bulk, cc, zz of the constant-coefficient acoustics
    h = C.c_void_p()
    L.check(L.lib().pcl_create(C.byref(cfg), C.byref(h)))
    return h


def full_shape(ndim, mbc):
    return tuple(n + 2 * mbc for n in GRID[ndim])


def filled_by(L, h, q, call):
    """put q with its ghost cells, run one fill call, read everything back"""
    lib = L.lib()
    L.check(lib.pcl_put_q(h, L.d(q), 1))
    L.check(call())
    out = np.zeros_like(q)
    L.check(lib.pcl_get_q(h, L.d(out), 1))
    return out


@pytest.mark.parametrize("ndim,mbc", CASES)
def test_pcl_bc_equals_numpy_rule(ndim, mbc):
    from pyclaw_amd import _lib as L
    lib = L.lib()
    rp, meqn, mwaves = PLAIN[ndim]
    h = make_solver(L, ndim, mbc, rp, meqn, mwaves, maux=2 if ndim == 3 else 0)
    rng = np.random.default_rng(10 * ndim + mbc)
    try:
        for idim in range(ndim):
            for side in (0, 1):
                for bctype in (OUTFLOW, PERIODIC, REFLECTING):
                    q = np.asfortranarray(rng.standard_normal((meqn,) + full_shape(ndim, mbc)))
                    want = q.copy("F")
                    fill_side(want, idim, mbc, side, bctype)
                    got = filled_by(L, h, q, lambda: lib.pcl_bc(h, idim, side, bctype))
                    assert np.array_equal(got, want), (idim, side, bctype)
                    assert not np.array_equal(got, q)
    finally:
        lib.pcl_destroy(h)


@pytest.mark.parametrize("ndim,mbc", [c for c in CASES if c[0] < 3])
def test_pcl_bc_const_equals_numpy_rule(ndim, mbc):
    from pyclaw_amd import _lib as L
    lib = L.lib()
    rp, meqn, mwaves = PLAIN[ndim]
    h = make_solver(L, ndim, mbc, rp, meqn, mwaves)
    rng = np.random.default_rng(20 * ndim + mbc)
    try:
        for idim in range(ndim):
            for side in (0, 1):
                q = np.asfortranarray(rng.standard_normal((meqn,) + full_shape(ndim, mbc)))
                state = 100.0 + rng.standard_normal(meqn)
                want = q.copy("F")
                fill_side(want, idim, mbc, side, CUSTOM, cst=state)
                got = filled_by(L, h, q, lambda: lib.pcl_bc_const(h, idim, side, L.d(state)))
                assert np.array_equal(got, want), (idim, side)
    finally:
        lib.pcl_destroy(h)


def test_pcl_bc_const_is_refused_in_3d():
    from pyclaw_amd import _lib as L
    lib = L.lib()
    rp, meqn, mwaves = PLAIN[3]
    h = make_solver(L, 3, 2, rp, meqn, mwaves, maux=2)
    try:
        q = np.asfortranarray(np.random.default_rng(3).standard_normal((meqn,) + full_shape(3, 2)))
        state = np.arange(1.0, 1.0 + meqn)
        L.check(lib.pcl_put_q(h, L.d(q), 1))
        for idim in range(3):
            for side in (0, 1):
                assert lib.pcl_bc_const(h, idim, side, L.d(state)) == L.EINVAL
                assert lib.pcl_last_error() == b"constant-state BC is implemented for 1-D/2-D"
        out = np.zeros_like(q)
        L.check(lib.pcl_get_q(h, L.d(out), 1))
        assert np.array_equal(out, q)
    finally:
        lib.pcl_destroy(h)


@pytest.mark.parametrize("mbc", [2, 3])
def test_sphere_mirror_equals_numpy_rule(mbc):
    """shallow_4_Rossby_Haurwitz_wave.py:295-313: the ghost row mirrors the interior row and reverses the x index over the
    whole ghosted width"""
    from pyclaw_amd import _lib as L
    lib = L.lib()
    rp, meqn, mwaves = PLAIN[2]
    h = make_solver(L, 2, mbc, rp, meqn, mwaves)
    rng = np.random.default_rng(40 + mbc)
    try:
        for side in (0, 1):
            q = np.asfortranarray(rng.standard_normal((meqn,) + full_shape(2, mbc)))
            want = q.copy("F")
            J = q.shape[2]
            for j in range(mbc):
                if side == 0:
                    want[:, :, j] = q[:, ::-1, 2 * mbc - 1 - j]
                else:
                    want[:, :, J - mbc + j] = q[:, ::-1, J - mbc - 1 - j]
            got = filled_by(L, h, q, lambda: lib.pcl_bc(h, 1, side, SPHERE_MIRROR))
            assert np.array_equal(got, want), side
    finally:
        lib.pcl_destroy(h)


# solvers that read aux components 0 and 1 of both cells of an interface: (rp, meqn, mwaves, maux, fwave)
AUX = {1: (O.RP_ELASTICITY_FWAVE_1D, 2, 2, 3, 1), 2: (O.RP_VC_ACOUSTICS_2D, 3, 2, 2, 0), 3: (O.RP_VC_ACOUSTICS_3D, 4, 2, 2, 0)}


def aux_state(rng, ndim, mbc):
    rp, meqn, mwaves, maux, fwave = AUX[ndim]
    full = full_shape(ndim, mbc)
    q = np.asfortranarray(0.1 * rng.standard_normal((meqn,) + full))
    aux = np.ones((maux,) + full, order="F")        # (the elasticity solver's third component: 1 = linear stress law)
    aux[0] = 0.5 + 2.0 * rng.random(full)
    aux[1] = 0.5 + 1.5 * rng.random(full)
    return q, aux


def oracle_sweep(coracle, ndim, mbc, q, aux, idim, dt):
    """one sweep along idim of the classic dimension-split step (1-D: the step) -> (q with ghosts, cfl)"""
    rp, meqn, mwaves, maux, fwave = AUX[ndim]
    n = GRID[ndim]
    d = [1.0 / v for v in n]
    mthlim = np.array([4] * mwaves, dtype=np.int32)
    method = np.array([1, 2, -1 if ndim > 1 else 0, 0, 0, 0, maux], dtype=np.int32)
    out = q.copy("F")
    if ndim == 1:
        return coracle.step1(rp, [0.0], mbc, n[0], out, aux, d[0], dt, method, mthlim, fwave=bool(fwave))
    if ndim == 2:
        return coracle.step2ds(rp, [0.0], max(n), mbc, n[0], n[1], q.copy("F"), out, aux, d[0], d[1], dt, method, mthlim,
                               idim + 1, fwave=bool(fwave))
    return coracle.step3ds(rp, max(n), mbc, n[0], n[1], n[2], q.copy("F"), out, aux, d[0], d[1], d[2], dt, method, mthlim,
                           idim + 1)


@pytest.mark.parametrize("ndim,mbc", CASES)
def test_pcl_bc_aux_feeds_the_sweep_like_the_numpy_rule(coracle, ndim, mbc):
    from pyclaw_amd import _lib as L
    lib = L.lib()
    rp, meqn, mwaves, maux, fwave = AUX[ndim]
    h = make_solver(L, ndim, mbc, rp, meqn, mwaves, maux=maux, fwave=fwave)
    rng = np.random.default_rng(30 * ndim + mbc)
    inner = (slice(None),) + (slice(mbc, -mbc),) * ndim
    dt = 0.02
    try:
        for idim in range(ndim):
            for side in (0, 1):
                for bctype in (OUTFLOW, PERIODIC, REFLECTING):
                    q, aux = aux_state(rng, ndim, mbc)
                    filled = aux.copy("F")
                    fill_side(filled, idim, mbc, side, bctype, negate=False)
                    want, cfl_o = oracle_sweep(coracle, ndim, mbc, q, filled, idim, dt)
                    unfilled, _ = oracle_sweep(coracle, ndim, mbc, q, aux, idim, dt)
                    assert not np.array_equal(unfilled[inner], want[inner])         # the fill decides the result
                    L.check(lib.pcl_put_q(h, L.d(q), 1))
                    L.check(lib.pcl_put_aux(h, L.d(aux)))
                    L.check(lib.pcl_bc_aux(h, idim, side, bctype))
                    cfl = C.c_double()
                    L.check(lib.pcl_sweep(h, idim + 1, dt, C.cast(C.byref(cfl), L.dp)))
                    got = np.zeros_like(q)
                    L.check(lib.pcl_get_q(h, L.d(got), 1))
                    assert np.array_equal(got[inner], want[inner]), (idim, side, bctype)
                    assert cfl.value == cfl_o and cfl.value > 0
    finally:
        lib.pcl_destroy(h)
