"""
GPU: the one-kernel form of the dimension-split 2-D step (classic_fused.hpp) for Riemann solvers that read aux arrays
(vc_acoustics_2d, vc_advection_2d, psystem_fwave_2d with the linear stress law) and for states with a capacity function
(acoustics_2d, advection_2d, euler_5wave_2d, shallow_2d and vc_acoustics_2d with aux(mcapa)).
  PCL_TUNE_FUSED_STEP=1   both sweeps of a step in one kernel: the aux planes and the capacity function are staged in
                          the LDS tile next to q
  PCL_TUNE_FUSED_STEP=0   x pass + y pass (classic.hpp)
  PCL_TUNE_FUSED_STEP=2   the default: timed trials choose (trial steps 64 .. 71 of a window)
The switch is read once per process: one child process per mode (tests/fused_aux_worker.py), one at a time.  The three
modes must agree bit for bit (states and the Courant number of every step), mode 1 must run every step in the
one-kernel form, and mode 1 must equal the C oracle (orc_step2ds: boundary conditions, x pass, y pass) -- and through
tests/golden/ref_step2ds_capa.npz the reference's own step2ds.f.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("fused_aux_worker", os.path.join(HERE, "fused_aux_worker.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)


def run_worker(mode, dump):
    env = dict(os.environ)
    env["PCL_TUNE_FUSED_STEP"] = str(mode)
    p = subprocess.run([sys.executable, os.path.join(HERE, "fused_aux_worker.py"), dump], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """mode -> (the worker's line, its final states); one child at a time"""
    d = tmp_path_factory.mktemp("fused_aux")
    out = {}
    for mode in (1, 0, 2):
        f = str(d / ("mode%d.npz" % mode))
        out[mode] = (run_worker(mode, f), np.load(f, allow_pickle=False))
    return out


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in W.cases()}


def test_every_step_runs_in_one_kernel(runs, cases):
    """PCL_TUNE_FUSED_STEP=1: every step of every case in the one-kernel form, none in two passes (before these
    solvers had the one-kernel form, every step here was two-pass)"""
    one = runs[1][0]
    assert set(one) == set(cases) and len(one) >= 30
    for k in sorted(one):
        assert one[k]["forms"] == [cases[k].steps, 0], (k, one[k]["forms"])
    for k in sorted(runs[0][0]):
        assert runs[0][0][k]["forms"] == [0, cases[k].steps], (k, runs[0][0][k]["forms"])
    # the default mode ran its trial steps of the 80-step case in both forms
    fa = runs[2][0]["vc_acoustics_window_200x90"]["forms"]
    assert fa[0] >= 4 and fa[1] >= 4 and fa[0] + fa[1] == 80, fa


def test_three_modes_agree(runs):
    one, two, auto = runs[1][0], runs[0][0], runs[2][0]
    assert set(one) == set(two) == set(auto)
    for k in sorted(one):
        assert one[k]["finite"], k
        for other in (two, auto):
            assert one[k]["hash"] == other[k]["hash"], k
            assert one[k]["cfl"] == other[k]["cfl"], (k, one[k]["cfl"], other[k]["cfl"])
        assert 0.0 < max(float(v) for v in one[k]["cfl"]) < 1.0, (k, one[k]["cfl"])


def test_one_kernel_equals_oracle(runs, cases, coracle):
    """every case: interior cells and the Courant number of every step equal the oracle's (the aux + capa, capa-Euler and
    vc-acoustics cases among them)"""
    line, states = runs[1]
    assert {"vc_acoustics_capa_130x75", "euler_capa_130x75", "vc_acoustics_layered_300x100"} <= set(cases)
    for k in sorted(cases):
        ref, cfls = W.oracle_run(coracle, cases[k])
        assert np.array_equal(states[k], ref), "%s: max diff %g" % (k, np.abs(states[k] - ref).max())
        assert [float(v) for v in line[k]["cfl"]] == cfls, (k, line[k]["cfl"], cfls)
        assert not np.array_equal(ref, cases[k].q[:, 2:-2, 2:-2]), k


def test_one_kernel_equals_reference_fortran_chain(runs, cases, coracle):
    """tests/golden/ref_step2ds_capa.npz holds single passes of the reference's step2ds.f.  From its ids = 1 input: the
    oracle's x pass is that golden, its y pass of the x-swept array completes the step -- the one-kernel step equals it"""
    c = cases["golden_capa"]
    z = np.load(os.path.join(HERE, "golden", "ref_step2ds_capa.npz"), allow_pickle=False)
    assert c.mcapa == 2 and c.dt == float(z["dt"]) and (c.mx, c.my) == (int(z["mx"]), int(z["my"]))
    mth = np.array(c.mthlim, dtype=np.int32)
    qx = c.q.copy("F")
    _, cfl_x = coracle.step2ds(c.rp, c.par, max(c.mx, c.my), 2, c.mx, c.my, c.q.copy("F"), qx, c.aux, c.dx, c.dy, c.dt,
                               c.method(), mth, 1)
    assert np.array_equal(qx, z["q_ids1"]) and cfl_x == float(z["cfl_ids1"])
    _, cfl_y = coracle.step2ds(c.rp, c.par, max(c.mx, c.my), 2, c.mx, c.my, qx, qx, c.aux, c.dx, c.dy, c.dt, c.method(), mth, 2)
    line, states = runs[1]
    assert line["golden_capa"]["forms"] == [1, 0]
    assert np.array_equal(states["golden_capa"], qx[:, 2:-2, 2:-2])
    assert [float(v) for v in line["golden_capa"]["cfl"]] == [max(cfl_x, cfl_y)]


def test_capacity_function_matters(runs):
    """the same Euler problem without the capacity function gives another state: CAPA is not silently ignored"""
    one = runs[1][0]
    assert one["euler_capa_130x75"]["hash"] != one["euler_capa_off_130x75"]["hash"]
    assert one["euler_capa_130x75"]["cfl"] != one["euler_capa_off_130x75"]["cfl"]
