"""
Shallow water on the sphere (BASELINE configs[4]): the oracle's restatement of the absent third-party
Riemann solvers (rpn2/rpt2_shallow_sphere) + the app's own step2qcor.f / qcor.f / src2.f / setaux.f / qinit.f.

PINNING.  The two Riemann solvers have no source in the reference tree; what pins them is the reference's golden
test/swsphere_height (classic unsplit + qcor, 40 x 20, t = 10), gate 2-norm < 1e-4 (test/test_examples.py:456-472).
The replay below reproduces it to ~1e-17, i.e. to the digits the golden file holds.  The app-local Fortran IS in the
tree: its restatement is compared bit for bit with arrays made by the reference's own files
(tests/golden/ref_sphere_setup.npz <- tests/golden/make_ref_goldens.py <- oracle/_ref/libref_sphere_problem.so).
"""
import os

import numpy as np
import pytest

import ref_pins as P
from oracle import driver as D
from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture():
    return np.load(os.path.join(HERE, "golden", "ref_sphere_setup.npz"), allow_pickle=False)


def test_oracle_replays_swsphere_height(coracle, golden_dir):
    p = D.shallow_sphere_problem(coracle)
    st = D.run(p, coracle, 10.0, 10)
    gold = np.loadtxt(os.path.join(golden_dir, "swsphere_height"))
    diff = np.linalg.norm(p.q[0] - gold)
    assert diff < 1.e-4                 # the reference's gate
    assert diff < 1.e-14, diff          # what the restatement actually achieves (2e-17)
    assert sum(s["numsteps"] for s in st) == 764 and p.nrejected == 1


def test_c_setup_equals_reference_fortran(coracle):
    z = fixture()
    mx, my = int(z["mx"]), int(z["my"])
    dx, dy = 4.0 / mx, 2.0 / my
    aux = coracle.sphere_setaux(2, mx, my, -3.0, -1.0, dx, dy)
    assert np.array_equal(aux, z["aux"])
    q0 = coracle.sphere_qinit(2, mx, my, -3.0, -1.0, dx, dy)[:, 2:-2, 2:-2]
    assert np.array_equal(q0, z["q0"])
    qs = np.array(z["q0"], order="F")
    coracle.sphere_src2(qs, np.array(z["aux"][:, 2:-2, 2:-2], order="F"), -3.0, -1.0, dx, dy, float(z["dt_src2"]))
    assert np.array_equal(qs, z["q_src2"])
    qfull = coracle.sphere_qinit(2, mx, my, -3.0, -1.0, dx, dy)
    for ixy in (1, 2):
        for k in range(8):
            if ixy == 1:
                a1, q1 = np.array(aux[:, :, 7], order="F"), np.array(qfull[:, :, 7], order="F")
            else:
                a1, q1 = np.array(aux[:, 9, :], order="F"), np.array(qfull[:, 9, :], order="F")
            qc = coracle.qcor(ixy, 3 + k, a1, q1, 2, 11489.57219, dx, dy)
            assert np.array_equal(qc, z["qcor"][ixy - 1, :, k]), (ixy, k)


def test_numpy_app_setup_matches_reference_fortran():
    """apps/shallow_sphere.py (the product-side data generators, vectorised numpy).  Everything but the capacity
    function is bit-equal; kappa (aux[0]) goes through acos/tan of nearly degenerate arguments (setaux.f:166-211) and
    amplifies a 1-ulp difference between numpy's and the Fortran runtime's elementary functions to ~1e-8."""
    from apps import shallow_sphere as S
    z = fixture()
    mx, my = int(z["mx"]), int(z["my"])
    dx, dy = 4.0 / mx, 2.0 / my
    aux = S.setaux(mx, my, 2, -3.0, -1.0, dx, dy)
    assert np.abs(aux[1:] - z["aux"][1:]).max() < 1e-14
    assert np.abs(aux[0] - z["aux"][0]).max() < 1e-6
    q0 = S.qinit(mx, my, -3.0, -1.0, dx, dy)
    assert np.abs(q0 - z["q0"]).max() < 1e-14 * np.abs(z["q0"]).max()


@pytest.mark.parametrize("mx,my", [(24, 12), (64, 48)])
def test_c_setup_equals_reference_build(coracle, mx, my):
    """the reference build's results are pinned (tests/ref_pins.py); compared with the live build where it is present"""
    r = O.RefSphereProblem() if O.RefSphereProblem.available() else None
    dx, dy = 4.0 / mx, 2.0 / my
    aux = coracle.sphere_setaux(2, mx, my, -3.0, -1.0, dx, dy)
    q0 = coracle.sphere_qinit(2, mx, my, -3.0, -1.0, dx, dy)
    assert not np.isnan(aux).any() and not np.isnan(q0).any()
    P.check("sphere_setaux/%dx%d" % (mx, my), aux)
    P.check("sphere_qinit/%dx%d" % (mx, my), q0)
    if r is not None:
        raux, rq0 = r.sphere_setaux(2, mx, my, -3.0, -1.0, dx, dy), r.sphere_qinit(2, mx, my, -3.0, -1.0, dx, dy)
        P.record("sphere_setaux/%dx%d" % (mx, my), raux)
        P.record("sphere_qinit/%dx%d" % (mx, my), rq0)
        assert np.array_equal(aux, raux)
        assert np.array_equal(q0, rq0)
