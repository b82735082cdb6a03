"""
The SharpClaw right-hand side dq = dt * L(q) restated in numpy for any number of dimensions: the expected value of
tests/test_sharp3_cpu.py and tests/test_gpu_sharp3.py.  TEST INFRASTRUCTURE ONLY.

The reference has a 1-D and a 2-D SharpClaw and no flux3.f90, so the 3-D right-hand side the device is held to is the
extension of the 2-D one by one more transverse index:

  * flux1.f90:59-188 on one line (char_decomp = 0, no tfluct), restated here as `flux1` in the operation order of the
    frozen oracle's C restatement (oracle/sharpclaw_oracle.c: flux1), which is pinned to the Fortran;
  * the slice driver of flux2.f90:32-94, generic in ndim (`dq_reference`): a line is swept if and only if ALL of its
    transverse indices lie in 0 .. m+1 (one ghost layer: flux2.f90:38,70), directions in the order x, y, z, every line's
    dq1d added to dq, the Courant number the maximum over exactly those lines.

What is NOT restated: the reconstructions come from the oracle's exported orc_weno5 (variant 2: PyWENO weno5, 3: legacy
weno5) and orc_weno_k (orders 7..17), and the Riemann solver is a callable -- the oracle's orc_rpn2_ptr in the 2-D
self-check, its orc_rpn3 in 3-D.  tvd2 (reconstruct.f90:568-625) is restated in numpy, since the oracle does not export it.
tests/test_sharp3_cpu.py holds this glue in two dimensions to orc_sharp_flux2 bit for bit, cfl included.

The glue fixes the order: the in-cell swap, dtdx = dt / (dx * capa), the four-term sum, the CFL expression, lines 0..m+1,
x then y then z.  Lines are handed to the C routines as one long line (n cells each, one after the other): a stencil or an
interface that crosses from one line into the next lies in cells flux1 never reads (the outermost ghost cells).

Arrays: q (meqn, N0, N1, ...) with ghost cells, Fortran order; aux (maux, N0, N1, ...) or None; a Riemann callable
    rpn(idir, ql, qr, auxl, auxr) -> s (mwaves, n), amdq (meqn, n), apdq (meqn, n)
over a line of n cells in Clawpack's convention: interface i lies between qr(:, i-1) and ql(:, i), with auxr(:, i-1) and
auxl(:, i); idir is 1, 2 or 3.
"""
import ctypes as C

import numpy as np

_dp = C.POINTER(C.c_double)


def _d(a):
    return a.ctypes.data_as(_dp)


def _F(a):
    return np.asfortranarray(a, dtype=np.float64)


# ---- the Riemann callables: the oracle's exported solvers -------------------------------------------------------------------
def oracle_rpn2(coracle, rp, par, meqn, mwaves, mbc):
    """orc_rpn2_ptr (a 2-D solver without aux arrays) as a callable"""
    par = np.ascontiguousarray(par, dtype=np.float64)
    fn = coracle.lib.orc_rpn2_ptr
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, _dp] + [C.c_int] * 5 + [_dp] * 6

    def rpn(idir, ql, qr, auxl, auxr):
        n = ql.shape[1]
        wave = np.zeros((meqn, mwaves, n), order="F")
        s = np.zeros((mwaves, n), order="F")
        amdq, apdq = np.zeros((meqn, n), order="F"), np.zeros((meqn, n), order="F")
        assert fn(rp, _d(par), idir, meqn, mwaves, mbc, n - 2 * mbc, _d(_F(ql)), _d(_F(qr)), _d(wave), _d(s), _d(amdq), _d(apdq)) == 0
        return s, amdq, apdq
    return rpn


def oracle_rpn3(coracle, rp, meqn, mwaves, maux, mbc):
    """orc_rpn3 (rpn3_vc_acoustics) as a callable"""
    fn = coracle.lib.orc_rpn3
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 7 + [_dp] * 8

    def rpn(idir, ql, qr, auxl, auxr):
        n = ql.shape[1]
        wave = np.zeros((meqn, mwaves, n), order="F")
        s = np.zeros((mwaves, n), order="F")
        amdq, apdq = np.zeros((meqn, n), order="F"), np.zeros((meqn, n), order="F")
        assert fn(rp, idir, meqn, mwaves, maux, mbc, n - 2 * mbc, _d(_F(ql)), _d(_F(qr)), _d(_F(auxl)), _d(_F(auxr)),
                  _d(wave), _d(s), _d(amdq), _d(apdq)) == 0
        return s, amdq, apdq
    return rpn


# ---- reconstruction ---------------------------------------------------------------------------------------------------------
def tvd2(q, mthlim):
    """reconstruct.f90:568-625 on q (meqn, n): ql, qr at the slice indices 3 .. n-2 (1-based; the routine's hard-wired
    mbc = 2), zero elsewhere.  mthlim is indexed by COMPONENT; dqm of the first index is q(3) - q(2) (the Fortran reads it
    uninitialised there: ghost cell 0 only, see oracle/sharpclaw_oracle.c).  MAX / MIN drop a NaN operand like gfortran's
    (0/0 on constant data).  Limiter id 0 (no entry: the configuration holds mwaves of them) is qlimitr = 0."""
    meqn, n = q.shape
    ql, qr = np.zeros((meqn, n), order="F"), np.zeros((meqn, n), order="F")
    k = np.arange(2, n - 2)                  # 0-based slice indices 3 .. n-2
    with np.errstate(all="ignore"):
        for m in range(meqn):
            dqm = q[m, k] - q[m, k - 1]
            dqp = q[m, k + 1] - q[m, k]
            r = dqp / dqm
            meth = mthlim[m] if m < len(mthlim) else 0
            if meth == 1:
                lim = np.fmax(0.0, np.fmin(1.0, r))
            elif meth == 2:
                lim = np.fmax(np.fmax(0.0, np.fmin(1.0, 2.0 * r)), np.fmin(2.0, r))
            elif meth == 3:
                lim = (r + np.abs(r)) / (1.0 + np.abs(r))
            elif meth == 4:
                c = (1.0 + r) / 2.0
                lim = np.fmax(0.0, np.fmin(np.fmin(c, 2.0), 2.0 * r))
            elif meth == 5:
                alpha = 1.0 / 3.0
                pp = (2.0 + r) / 3.0
                amax = np.fmax(np.fmax(-alpha * r, 0.0), np.fmin(np.fmin(2.0 * r, pp), 2.0))
                lim = np.fmax(0.0, np.fmin(pp, amax))
            else:
                lim = np.zeros_like(r)
            qr[m, k] = q[m, k] + 0.5 * lim * dqm
            ql[m, k] = q[m, k] - 0.5 * lim * dqm
    return ql, qr


def reconstruction(coracle, lim_type, weno_order, mbc, mthlim=()):
    """q (meqn, n) -> ql, qr (meqn, n), as flux1.f90 picks it from lim_type and weno_order"""
    def recon(q):
        if lim_type == 1:
            return tvd2(q, mthlim)
        if lim_type == 2 and weno_order == 5:
            return coracle.weno5(2, mbc, q)
        if lim_type == 2:
            return coracle.weno_k(weno_order, q)
        assert lim_type == 3 and weno_order == 5
        return coracle.weno5(3, mbc, q)
    return recon


# ---- flux1.f90:59-188 on L lines at once ------------------------------------------------------------------------------------
def flux1(rpn, recon, idir, q, aux, dtdx, mbc):
    """q (meqn, n, L), aux (maux, n, L) or None, dtdx (n, L): L lines of n = mx + 2 mbc cells.  Returns dq1d (meqn, n, L),
    nonzero in the interior cells only, and the Courant number over all of them."""
    meqn, n, L = q.shape
    mx = n - 2 * mbc

    def flat(a):            # (k, n, L) -> (k, n * L): the lines one after the other
        return np.asfortranarray(a).reshape((a.shape[0], n * L), order="F")

    def lines(a):
        return np.asfortranarray(a).reshape((a.shape[0], n, L), order="F")
    if aux is None:
        aux = np.zeros((1, n, L), order="F")
    ql, qr = (lines(a) for a in recon(flat(q)))
    s, amdq, apdq = (lines(a) for a in rpn(idir, flat(ql), flat(qr), flat(aux), flat(aux)))       # interface i
    # flux1.f90:134-141: cfl = max(cfl, dtdx(i) * s(mw, i), -dtdx(i-1) * s(mw, i)), i = 1 .. mx+1
    k = np.arange(mbc, mbc + mx + 1)
    cfl = 0.0
    for mw in range(s.shape[0]):
        cfl = max(cfl, float((dtdx[k] * s[mw, k]).max()), float((-dtdx[k - 1] * s[mw, k]).max()))
    # flux1.f90:166-171: qr(i-1) = ql(i); ql(i) = qr(i), i = 2-mbc .. mx+mbc -- the problem inside cell i at interface i
    ql2, qr2 = ql.copy(), qr.copy()
    qr2[:, :-1] = ql[:, 1:]
    ql2[:, 1:] = qr[:, 1:]
    # flux1.f90:173-178: auxr(:, i-1) = aux(:, i), auxl(:, i) = aux(:, i): both edge states of a cell see its own aux
    auxr2 = np.zeros_like(aux)
    auxr2[:, :-1] = aux[:, 1:]
    _, amdq2, apdq2 = (lines(a) for a in rpn(idir, flat(ql2), flat(qr2), flat(aux), flat(auxr2)))
    dq = np.zeros((meqn, n, L), order="F")
    k = np.arange(mbc, mbc + mx)
    dq[:, k] = 0.0 - dtdx[k] * (amdq[:, k + 1] + apdq[:, k] + amdq2[:, k] + apdq2[:, k])
    return dq, cfl


# ---- the slice driver, generic in ndim --------------------------------------------------------------------------------------
def dq_reference(rpn, recon, q, aux, mcapa, mbc, d, dt):
    """dq (the shape of q: nonzero where a swept line has interior cells, i.e. also in the one ghost layer of the transverse
    directions, as flux2.f90 leaves it) and cfl.  mcapa: 0 = none, else the 1-based aux component; d = (dx, dy, ...)."""
    ndim = q.ndim - 1
    dq = np.zeros(q.shape, order="F")
    cfl = 0.0
    for idim in range(ndim):
        # this direction first, then the transverse ones restricted to the lines 0 .. m+1
        def gather(a):
            a = np.moveaxis(a, 1 + idim, 1)
            sel = (slice(None), slice(None)) + (slice(mbc - 1, -(mbc - 1)),) * (ndim - 1)
            return a[sel]
        ql = gather(q)
        shape = ql.shape
        L = int(np.prod(shape[2:])) if ndim > 1 else 1
        q3 = np.asfortranarray(ql).reshape((shape[0], shape[1], L), order="F")
        a3 = None
        if aux is not None:
            al = gather(aux)
            a3 = np.asfortranarray(al).reshape((al.shape[0], shape[1], L), order="F")
        dtdx = np.full((shape[1], L), dt / d[idim]) if mcapa <= 0 else dt / (d[idim] * a3[mcapa - 1])
        dq1, cfl1 = flux1(rpn, recon, idim + 1, q3, a3, dtdx, mbc)
        cfl = max(cfl, cfl1)
        view = gather(dq)          # a view of dq: the swept lines
        view += dq1.reshape(shape, order="F")
    return dq, cfl


# ---- ghost cells and the Runge-Kutta schemes over dq_reference ---------------------------------------------------------------
PERIODIC, EXTRAP, WALL = 2, 1, 3     # pyclaw.BC.periodic / outflow / reflecting


def fill_ghosts(q, mbc, bc_lower, bc_upper, is_aux=False):
    """q (meqn, m0, m1, ...) interior -> the array with mbc ghost layers, filled per dimension, lower then upper
    (solver.py:384-452): periodic, zero-order extrapolation, or a solid wall (mirror image, normal velocity negated)"""
    ndim = q.ndim - 1
    qb = np.zeros((q.shape[0],) + tuple(n + 2 * mbc for n in q.shape[1:]), order="F")
    qb[(slice(None),) + (slice(mbc, -mbc),) * ndim] = q
    for idim in range(ndim):
        v = np.moveaxis(qb, 1 + idim, 1)        # a view
        n = v.shape[1]
        for side, t in ((0, bc_lower[idim]), (1, bc_upper[idim])):
            for g in range(mbc):
                k = g if side == 0 else n - 1 - g
                if t == PERIODIC:
                    src = k + (n - 2 * mbc) if side == 0 else k - (n - 2 * mbc)
                elif t == EXTRAP:
                    src = mbc if side == 0 else n - mbc - 1
                else:
                    src = 2 * mbc - 1 - k if side == 0 else 2 * (n - mbc) - 1 - k
                v[:, k] = v[:, src]
                if t == WALL and not is_aux and 1 + idim < v.shape[0]:
                    v[1 + idim, k] = -v[1 + idim, k]
    return qb


def ssp104(q, dq):
    """sharpclaw.py:176-206 on interior arrays; dq(y) -> (dt L(y), cfl) raises nothing: the caller checks the numbers"""
    cfls = []

    def f(y):
        d, c = dq(y)
        cfls.append(c)
        return d
    s1 = q + f(q) / 6.
    for _ in range(4):
        s1 = s1 + f(s1) / 6.
    s2 = q / 25. + 9. / 25 * s1
    s1 = 15. * s2 - 5. * s1
    for _ in range(4):
        s1 = s1 + f(s1) / 6.
    return s2 + 0.6 * s1 + 0.1 * f(s1), cfls


def ssp33(q, dq):
    cfls = []

    def f(y):
        d, c = dq(y)
        cfls.append(c)
        return d
    s1 = q + f(q) / 1.0
    s1 = 0.75 * q + 0.25 * (s1 + f(s1))
    return 1. / 3. * q + 2. / 3. * (s1 + f(s1)), cfls


def tableau(q, dq, a, b, c):
    """tests/rk_reference.py's step over this dq: y_i = q + sum a_ij K_j, q + sum b_j K_j, terms left to right, a zero
    coefficient no term"""
    def lincomb(A, coef, K):
        r = A
        for j, cj in enumerate(coef):
            if cj != 0.0:
                r = r + cj * K[j]
        return r
    K, cfls = [], []
    for i in range(len(b)):
        y = q if i == 0 else lincomb(q, a[i][:i], K)
        d, cf = dq(y)
        K.append(d)
        cfls.append(cf)
    return lincomb(q, b, K), cfls
