"""
GPU: the form policy of the dimension-split 2-D step (pclaw.hip: step_hyperbolic) skips a window's timed
trials where the tile count of the last launch settles the form: the launch ran over a list of L tiles and
4 L <= ntx * nty.  Everything else runs the trials as before (steps 64 .. 71 of a window, four of them two-pass steps).
The count is a function of the state, so the forms a run takes are the same every time.

The quiet case: 1200 x 480 Euler cells, periodic, are 20 x 40 = 800 tiles of which 116 lie on the frame (14.5 %: always
listed); uniform flow with momenta that are nowhere zero (the forms cannot differ in the sign of a zero) carries a dense
blob of 24 cells radius along (a contact: nothing else moves).
"""
import ctypes

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib

import test_gpu_quiet_tiles as Q
import test_gpu_tile_handover as T

pytestmark = pytest.mark.gpu

MX, MY, STEPS = 1200, 480, 80
U, V = 0.6, 0.2
PER = (pyclaw.BC.periodic,) * 4


def carried_blob(mx, my):
    """gas moving at (U, V) with p = 1 everywhere and, in the middle, three times as dense within min(mx, my) // 20 cells
    (24 at 1200 x 480): a contact discontinuity moving with the gas"""
    rho = np.ones((mx, my))
    i, j = np.meshgrid(np.arange(mx), np.arange(my), indexing='ij')
    rho[(i - mx // 2) ** 2 + (j - my // 2) ** 2 < (min(mx, my) // 20) ** 2] = 3.0
    return np.stack([rho, rho * U, rho * V, 2.5 + 0.5 * rho * (U * U + V * V), rho - 1.0])


def form_stats(h):
    L = _lib.lib()
    ms, n, one, two = ctypes.c_double(), ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(L.pcl_step_form_stats(h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(one), ctypes.byref(two)))
    return one.value, two.value


def run(make, skip=True, extra=None):
    """-> (hash of the final state's bytes, [(one-kernel steps, two-pass steps) after every step], [(computed, skipped)])"""
    forms = []

    def hook(k, h, rec):
        forms.append(form_stats(h))
        if extra is not None:
            extra(k, h)
    claw = make()
    with Q.Recorder(skip, hook) as rec:
        claw.run()
        digest, finite = Q.final_bytes(claw)
    assert finite
    assert all(e[1] == 0 for e in rec.log), rec.log
    return digest, forms, rec.stats


@pytest.fixture(scope="module")
def quiet():
    return run(T.euler_case(MX, MY, 2.0 * MY / MX, carried_blob, bc=PER, steps=STEPS))


def test_quiet_grid_skips_the_trials(quiet):
    _, forms, stats = quiet
    assert forms[-1] == (STEPS, 0), forms[-1]
    assert max(c for c, _ in stats[3:]) <= 200, stats
    assert all(c + s == 800 for c, s in stats), stats


def test_skipping_off_runs_the_trials_same_bytes(quiet):
    digest, forms, stats = run(T.euler_case(MX, MY, 2.0 * MY / MX, carried_blob, bc=PER, steps=STEPS), skip=False)
    assert forms[-1][1] >= 4 and sum(forms[-1]) == STEPS, forms[-1]
    assert all(s == 0 for _, s in stats)
    assert digest == quiet[0]


def test_dense_state_runs_the_trials():
    _, forms, _ = run(T.euler_case(420, 180, 2.0 * 180 / 420, Q.dense, bc=PER, steps=STEPS))
    assert forms[-1][1] >= 4 and sum(forms[-1]) == STEPS, forms[-1]


def test_gate_follows_the_current_list():
    """quiet for 60 steps, then pcl_put_q writes a dense state: the launches in front of step 64 are a full launch and
    list launches over nearly every tile, so the window's trials run"""
    def put_dense(k, h):
        if k == 59:
            L = _lib.lib()
            buf = np.empty(5 * MX * MY)
            _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
            buf *= 1.0 + 0.05 * np.random.default_rng(11).random(MX * MY).repeat(5)
            _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))
    _, forms, stats = run(T.euler_case(MX, MY, 2.0 * MY / MX, carried_blob, bc=PER, steps=STEPS), extra=put_dense)
    assert forms[59] == (60, 0) and max(c for c, _ in stats[3:60]) <= 200, (forms[59], stats[:60])
    assert stats[60] == (800, 0), stats[60]                 # behind the put: every tile
    assert 4 * stats[63][0] > 800, stats[63]                # the list launch in front of the window: above the bound
    assert forms[63] == (64, 0), forms[63]
    assert forms[-1][1] >= 4 and sum(forms[-1]) == STEPS, forms[-1]
