"""
GPU: the one-kernel dimension-split step hands its Courant number over exactly as the two-pass form does.
  PCL_TUNE_FUSED_STEP=1  every step is one kernel (classic_fused.hpp) with the one-kernel step's hand-over
  PCL_TUNE_FUSED_STEP=0  x pass + y pass with the single-thread hand-over kernel (pclaw.hip: cfl_handover): the reference
  PCL_TUNE_FUSED_STEP=2  the default policy: the 80-step case meets its trial window, two-pass steps between one-kernel steps
For every case the step sequence -- entry point, return code, dt.hex() and cfl.hex() of every step call, every undo --
must be identical, and so must the final state after mapping -0.0 to +0.0.  The switch is read once per process, hence
the worker (tests/inkernel_handover_worker.py), which also describes the cases.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("euler_60x12", "euler_61x13", "euler_130x30", "moving_blob_420x180", "moving_blob_420x180_noskip",
         "shockbubble_160x40", "acoustics_480x240", "vc_acoustics_240x120", "interleaved_600x240")


def run_worker(fused):
    env = dict(os.environ)
    env["PCL_TUNE_FUSED_STEP"] = str(fused)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "inkernel_handover_worker.py")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs():
    return {mode: run_worker(mode) for mode in (1, 0, 2)}


@pytest.mark.parametrize("case", CASES)
def test_step_sequence_equals_two_pass(runs, case):
    one, two, auto = runs[1][case], runs[0][case], runs[2][case]
    assert one["finite"] and two["finite"]
    assert len(two["log"]) >= 8
    assert all(e[1] == 0 for e in one["log"]), one["log"]           # every step call and every undo returned PCL_OK
    assert one["log"] == two["log"]
    assert one["hash"] == two["hash"]
    assert auto["log"] == two["log"]
    assert auto["hash"] == two["hash"]


def test_cases_ran_what_they_are_for(runs):
    one, two, auto = runs[1], runs[0], runs[2]
    assert set(one) == set(two) == set(auto) == set(CASES)
    # the app rejected its first step; the interleaved case took its undos
    assert any(e[0] == "undo" for e in one["shockbubble_160x40"]["log"])
    assert sum(1 for e in one["interleaved_600x240"]["log"] if e[0] == "retaken") == 3
    assert sum(1 for e in one["interleaved_600x240"]["log"] if e[0] == "bc_step") >= 80
    # the aux-carrying solver ran the form it was told to: [one kernel, two passes] from pcl_step_form_stats
    assert one["vc_acoustics_240x120"]["forms"] == [12, 0] and two["vc_acoustics_240x120"]["forms"] == [0, 12]
