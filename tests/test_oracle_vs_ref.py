"""
CPU: the oracle's C restatement against the REFERENCE'S OWN FORTRAN (oracle/_ref, flang build of
step2ds.f/step2.f/flux2.f/limiter.f/philim.f + the vendored Euler 5-wave solvers) on seeded
random inputs -- bit for bit.  What the reference build returns for every case is pinned in
tests/golden/ref_pins.json (tests/ref_pins.py), so the comparison runs where oracle/_ref has not
been built (it needs the reference tree); where it has, the live build is compared as well.

The vendored Euler pair is the one solver whose source lies in the reference tree, and that build carries no aux rows.
The last three tests run every other solver the oracle restates -- 1-D, 2-D with aux rows and capa, 3-D with all six
transverse modes -- through the reference's own step and flux Fortran linked against the RESTATED solvers
(oracle/ref_rp_shim.c, libref_classic*.so; cases in tests/ref_cases.py).  They pin the step around the solver; the
third-party solver formulas are the oracle's on both sides and stay unpinned.
"""
import numpy as np
import pytest

import ref_cases as RC
import ref_pins as P
from oracle import oracle as O


def euler_state(rng, shape, strong=False):
    q = np.empty((5,) + shape, order="F")
    if strong:
        rho = 0.2 + 2.0 * rng.random(shape)
        u = 3.0 * (rng.random(shape) - 0.5)
        v = 3.0 * (rng.random(shape) - 0.5)
        p = 0.1 + 2.0 * rng.random(shape)
    else:
        rho = 1.0 + 0.1 * rng.random(shape)
        u = 0.1 * rng.random(shape)
        v = 0.05 * rng.random(shape)
        p = 1.0 + 0.1 * rng.random(shape)
    q[0] = rho
    q[1] = rho * u
    q[2] = rho * v
    q[3] = p / 0.4 + 0.5 * rho * (u * u + v * v)
    q[4] = rng.random(shape)
    return q


@pytest.fixture(scope="module")
def ref():
    return O.RefEuler2D() if O.RefEuler2D.available() else None


@pytest.mark.parametrize("mx,my", [(5, 3), (40, 23), (97, 64)])
@pytest.mark.parametrize("strong", [False, True])
@pytest.mark.parametrize("order,mth", [(2, [4, 4, 4, 4, 2]), (2, [1, 2, 3, 5, 0]), (1, [4] * 5)])
def test_step2ds_matches_reference(coracle, ref, mx, my, strong, order, mth):
    rng = np.random.default_rng(mx * 1000 + my)
    mbc = 2
    q0 = euler_state(rng, (mx + 2 * mbc, my + 2 * mbc), strong)
    par = [1.4, 0.4]
    method = np.array([1, order, -1, 0, 0, 0, 0], dtype=np.int32)
    dx, dy, dt = 1.0 / mx, 1.0 / my, 0.1 / max(mx, my)
    for ids in (1, 2):
        key = "step2ds/%dx%d/strong%d/order%d/mth%s/ids%d" % (mx, my, strong, order, "".join(map(str, mth)), ids)
        a = q0.copy("F")
        b = q0.copy("F")
        _, ca = coracle.step2ds(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), a, None, dx,
                                dy, dt, method, mth, ids)
        assert not np.isnan(a).any()
        P.check(key, a, ca)
        if ref is not None:
            _, cb = ref.step2ds(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), b, None, dx, dy,
                                dt, method, mth, ids)
            P.record(key, b, cb)
            assert np.array_equal(a, b) and ca == cb


@pytest.mark.parametrize("mx,my", [(6, 4), (33, 50)])
@pytest.mark.parametrize("trans", [0, 1, 2])
@pytest.mark.parametrize("strong", [False, True])
def test_step2_unsplit_matches_reference(coracle, ref, mx, my, trans, strong):
    rng = np.random.default_rng(mx + 7 * my + trans)
    mbc = 2
    q0 = euler_state(rng, (mx + 2 * mbc, my + 2 * mbc), strong)
    par = [1.4, 0.4]
    mth = [4, 4, 4, 4, 2]
    method = np.array([1, 2, trans, 0, 0, 0, 0], dtype=np.int32)
    dx, dy, dt = 1.0 / mx, 1.0 / my, 0.05 / max(mx, my)
    key = "step2/%dx%d/trans%d/strong%d" % (mx, my, trans, strong)
    a = q0.copy("F")
    b = q0.copy("F")
    _, ca = coracle.step2(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), a, None, dx, dy, dt,
                          method, mth)
    assert not np.isnan(a).any()
    P.check(key, a, ca)
    if ref is not None:
        _, cb = ref.step2(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), b, None, dx, dy, dt,
                          method, mth)
        P.record(key, b, cb)
        assert np.array_equal(a, b) and ca == cb


@pytest.mark.parametrize("unsplit", [False, True])
def test_capa_matches_reference(coracle, ref, unsplit):
    rng = np.random.default_rng(3)
    mx, my, mbc = 31, 18, 2
    shape = (mx + 2 * mbc, my + 2 * mbc)
    q0 = euler_state(rng, shape)
    aux = np.asfortranarray(0.5 + rng.random((2,) + shape))
    par = [1.4, 0.4]
    mth = [4, 4, 4, 4, 2]
    method = np.array([1, 2, 2 if unsplit else -1, 0, 0, 2, 2], dtype=np.int32)
    dx, dy, dt = 1.0 / mx, 1.0 / my, 0.03 / mx
    a = q0.copy("F")
    b = q0.copy("F")
    if unsplit:
        _, ca = coracle.step2(O.RP_EULER5_2D, par, mx, mbc, mx, my, q0.copy("F"), a, aux, dx, dy, dt, method, mth)
        assert not np.isnan(a).any()
        P.check("capa/unsplit", a, ca)
        if ref is not None:
            _, cb = ref.step2(O.RP_EULER5_2D, par, mx, mbc, mx, my, q0.copy("F"), b, aux, dx, dy, dt, method, mth)
            P.record("capa/unsplit", b, cb)
            assert np.array_equal(a, b) and ca == cb
    else:
        for ids in (1, 2):
            _, ca = coracle.step2ds(O.RP_EULER5_2D, par, mx, mbc, mx, my, q0.copy("F"), a, aux, dx, dy, dt,
                                    method, mth, ids)
            assert not np.isnan(a).any()
            P.check("capa/dimsplit/ids%d" % ids, a, ca)
            if ref is not None:
                _, cb = ref.step2ds(O.RP_EULER5_2D, par, mx, mbc, mx, my, q0.copy("F"), b, aux, dx, dy, dt,
                                    method, mth, ids)
                P.record("capa/dimsplit/ids%d" % ids, b, cb)
                assert np.array_equal(a, b) and ca == cb


@pytest.mark.parametrize("mx,my", [(7, 5), (37, 29), (64, 90)])
@pytest.mark.parametrize("lim", [2, 3])
def test_sharpclaw_flux2_matches_reference(coracle, mx, my, lim):
    """C restatement of flux2/flux1/weno5 == the reference's SharpClaw modules (flang), bit for bit"""
    ref = O.RefSharp2DEuler() if O.RefSharp2DEuler.available() else None
    rng = np.random.default_rng(mx + my)
    mbc = 3
    q = euler_state(rng, (mx + 2 * mbc, my + 2 * mbc), strong=(mx == 37))
    par = [1.4, 0.4]
    dx, dy, dt = 1.0 / mx, 1.0 / my, 0.01
    key = "sharp_flux2/%dx%d/lim%d" % (mx, my, lim)
    a, ca = coracle.sharp_flux2(O.RP_EULER5_2D, par, lim, 5, 0, mbc, mx, my, q, None, dx, dy, dt)
    inner = (slice(None), slice(mbc, -mbc), slice(mbc, -mbc))
    # a strong random state makes WENO overshoot into negative pressure at some edges: NaNs, in the same places
    # (the pin's digest reads every NaN as one NaN, like equal_nan=True)
    P.check(key, a[inner], ca)
    if ref is not None:
        b, cb = ref.sharp_flux2(O.RP_EULER5_2D, par, lim, 5, 0, mbc, mx, my, q, None, dx, dy, dt)
        P.record(key, b[inner], cb)
        assert np.array_equal(a[inner], b[inner], equal_nan=True) and ca == cb


@pytest.mark.parametrize("mx,my", [(7, 5), (41, 30)])
@pytest.mark.parametrize("strong", [False, True])
@pytest.mark.parametrize("mth", [[4, 4, 4, 4, 2], [1, 2, 3, 5, 0]])
def test_fwave_form_matches_reference_flux2fw(coracle, mx, my, strong, mth):
    """the oracle's fwave=1 path against the reference's classic2fw link (flux2fw.f), dim-split and unsplit, on random
    Euler states: flux2fw.f:145-152 bit for bit"""
    reffw = O.RefEuler2D(fwave=True) if O.RefEuler2D.available(fwave=True) else None
    case = "fwave/%dx%d/strong%d/mth%s" % (mx, my, strong, "".join(map(str, mth)))
    rng = np.random.default_rng(3 * mx + my)
    mbc = 2
    q0 = euler_state(rng, (mx + 2 * mbc, my + 2 * mbc), strong)
    par = [1.4, 0.4]
    dx, dy, dt = 1.0 / mx, 1.0 / my, 0.05 / max(mx, my)
    method = np.array([1, 2, -1, 0, 0, 0, 0], dtype=np.int32)
    for ids in (1, 2):
        a, b = q0.copy("F"), q0.copy("F")
        _, ca = coracle.step2ds(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), a, None, dx, dy, dt, method,
                                mth, ids, fwave=True)
        assert not np.isnan(a).any()
        P.check(case + "/ids%d" % ids, a, ca)
        if reffw is not None:
            _, cb = reffw.step2ds(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), b, None, dx, dy, dt,
                                  method, mth, ids, fwave=True)
            P.record(case + "/ids%d" % ids, b, cb)
            assert np.array_equal(a, b) and ca == cb
    for trans in (0, 1, 2):
        method = np.array([1, 2, trans, 0, 0, 0, 0], dtype=np.int32)
        a, b = q0.copy("F"), q0.copy("F")
        _, ca = coracle.step2(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), a, None, dx, dy, dt, method, mth,
                              fwave=True)
        assert not np.isnan(a).any()
        P.check(case + "/trans%d" % trans, a, ca)
        if reffw is not None:
            _, cb = reffw.step2(O.RP_EULER5_2D, par, max(mx, my), mbc, mx, my, q0.copy("F"), b, None, dx, dy, dt, method,
                                mth, fwave=True)
            P.record(case + "/trans%d" % trans, b, cb)
            assert np.array_equal(a, b) and ca == cb


class _RefClassic:
    """the three libref_classic builds behind the call surface of COracle"""

    def __init__(self):
        r1, r2, r3 = O.RefClassic1D(), O.RefClassic2D(), O.RefClassic3D()
        self.step1, self.step2ds, self.step2, self.step3ds, self.step3 = r1.step1, r2.step2ds, r2.step2, r3.step3ds, r3.step3

    @staticmethod
    def available():
        return all([O.RefClassic1D.available(), O.RefClassic1D.available(fwave=True), O.RefClassic2D.available(),
                    O.RefClassic2D.available(fwave=True), O.RefClassic3D.available()])


@pytest.fixture(scope="module")
def refclassic():
    return _RefClassic() if _RefClassic.available() else None


def _check_block(coracle, refclassic, dim, block):
    """every group of the block: the oracle equals the pin, and the live reference build where there is one"""
    failed = []
    for key, g in RC.groups(dim, block):
        a, ca = RC.run_host(coracle, g)
        assert not np.isnan(a).any() and (ca > 0).all(), key
        if refclassic is not None:
            b, cb = RC.run_host(refclassic, g)
            assert not np.isnan(b).any(), key
            P.record(key, b, cb)
            if not (np.array_equal(a, b) and np.array_equal(ca, cb)):
                failed.append(key + " (live build)")
        try:
            P.check(key, a, ca)
        except AssertionError:
            failed.append(key)
    assert not failed, "%d groups differ from the reference: %s" % (len(failed), ", ".join(failed[:8]))


@pytest.mark.parametrize("block", RC.blocks(1), ids=RC.block_id)
def test_step1_matches_reference_step(coracle, refclassic, block):
    """step1.f / step1fw.f around the restated 1-D solvers: every limiter, order 1 and 2, with and without capa"""
    _check_block(coracle, refclassic, 1, block)


@pytest.mark.parametrize("block", RC.blocks(2), ids=RC.block_id)
def test_step2_aux_rows_match_reference_step(coracle, refclassic, block):
    """step2ds.f / step2.f with flux2.f or flux2fw.f around the restated 2-D solvers: aux1 / aux2 / aux3 rows handed to
    rpn2 / rpt2 with imp, capa as component maux+1, dimension-split ids 1, 2 and unsplit trans 0, 1, 2"""
    _check_block(coracle, refclassic, 2, block)


@pytest.mark.parametrize("block", RC.blocks(3), ids=RC.block_id)
def test_step3_matches_reference_step(coracle, refclassic, block):
    """step3.f + flux3.f in all six transverse modes and step3ds.f in its three directions (with mcapa too) around the
    restated 3-D solvers"""
    _check_block(coracle, refclassic, 3, block)
