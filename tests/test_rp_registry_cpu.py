"""
CPU: the library's own record of the built-in Riemann solvers (pcl_rp_info: read off the solver structs of rp.hpp
through the one solver list of kernels.hip) against the user-facing table of pyclaw_amd/riemann.py, and against the
rows the host layer kept by hand before the record was derived.  No GPU is touched.

Which GPU test runs each (solver, kernel family) the record claims against the oracle (mcs = test_gpu_more_solvers):
  sweep x (1-D) / x and y (2-D): advection_1d, acoustics_1d test_gpu_classic::test_step1_bitexact; burgers_1d
    mcs::test_burgers_step1; euler_1d, shallow_1d mcs::test_{euler1d,shallow1d}_step1_and_sharpclaw; advection_color_1d
    mcs::test_advection_color_1d; elasticity_fwave_1d test_fwave::test_hip_step1fw_elasticity; euler_5wave_2d,
    acoustics_2d test_gpu_classic::test_step2ds_{euler,acoustics}_bitexact; advection_2d
    mcs::test_advection2d_split_and_unsplit; shallow_2d, vc_advection_2d mcs::test_{shallow2d,vc_advection2d}_all_kernel_families;
    vc_acoustics_2d mcs::test_vc_acoustics2d_split_and_sharpclaw; shallow_sphere_2d
    test_gpu_sphere::test_step2ds_sphere_bitexact; psystem_fwave_2d test_fwave::test_hip_psystem_fwave (trans -1)
  one-kernel step: the seven solvers test_gpu_fused_aux::test_one_kernel_equals_oracle (vc_acoustics_*, vc_advection_*,
    psystem_*, {euler,acoustics,advection,shallow}_capa_*); euler_5wave_2d also test_gpu_apps::test_shockbubble_golden
  unsplit step: euler_5wave_2d, acoustics_2d test_gpu_classic::test_step2_unsplit_{euler,acoustics}_bitexact;
    advection_2d, shallow_2d, vc_advection_2d the mcs tests above; vc_acoustics_2d mcs::test_vc_acoustics2d_unsplit;
    shallow_sphere_2d test_gpu_sphere::test_step2qcor_bitexact; psystem_fwave_2d test_fwave::test_hip_psystem_fwave
  SharpClaw weno_order 5: acoustics_1d, euler_5wave_2d test_gpu_sharpclaw::test_flux1_acoustics1d_bitexact,
    ::test_flux2_euler_bitexact; acoustics_2d ::test_acoustics2d_sharpclaw_replay; burgers_1d
    mcs::test_burgers_sharpclaw_flux1; euler_1d, shallow_1d, advection_color_1d, shallow_2d, vc_acoustics_2d,
    vc_advection_2d the mcs tests above; advection_2d mcs::test_advection2d_sharpclaw_flux2; shallow_sphere_2d
    test_gpu_sphere::test_c5_grid_2048x1024_sharpclaw_sphere_spot_parity; psystem_fwave_2d
    test_gpu_sharpclaw_fwave::test_flux2_psystem; advection_1d test_weno_orders::test_hip_flux_of_the_solvers_not_run_elsewhere
  SharpClaw weno_order 7: euler_5wave_2d, acoustics_1d test_weno_orders::test_hip_flux2_euler_bitexact,
    ::test_hip_flux1_acoustics1d_bitexact; the other seven ::test_hip_flux_of_the_solvers_not_run_elsewhere
  wave-based 1-D: the six test_gpu_sharpclaw_fwave::test_flux1_wave_based_aux_capa_bitexact (five of them also
    test_gpu_sharpclaw::test_flux1_wave_based_bitexact)
  3-D: vc_acoustics_3d test_gpu_classic3d::test_step3ds_equals_oracle, test_classic3d_unsplit::test_hip_step3_bitexact
"""

import numpy as np
import pytest

from pyclaw_amd import _lib, riemann

FIELDS = ("ndim", "meqn", "mwaves", "naux", "fwave", "onek", "onek_aux", "sharp", "sharp_high", "sharp_wave")

# the host layer's former hand-kept table, row for row: name -> (ndim, meqn, mwaves, onek, onek_aux)
FORMER_ROWS = {
    "advection_1d": (1, 1, 1, False, False),        "acoustics_1d": (1, 2, 2, False, False),
    "burgers_1d": (1, 1, 1, False, False),          "euler_1d": (1, 3, 3, False, False),
    "shallow_1d": (1, 2, 2, False, False),          "advection_color_1d": (1, 1, 1, False, False),
    "elasticity_fwave_1d": (1, 2, 2, False, False), "psystem_fwave_2d": (2, 3, 2, False, True),
    "advection_2d": (2, 1, 1, True, False),         "shallow_2d": (2, 3, 3, True, False),
    "vc_acoustics_2d": (2, 3, 2, False, True),      "vc_advection_2d": (2, 1, 1, False, True),
    "shallow_sphere_2d": (2, 4, 3, False, False),   "acoustics_2d": (2, 3, 2, True, False),
    "euler_5wave_2d": (2, 5, 5, True, False),       "vc_acoustics_3d": (3, 4, 2, False, False),
}
# which solvers the SharpClaw launch code has kernels for
SHARP_1D = {"advection_1d", "acoustics_1d", "burgers_1d", "euler_1d", "shallow_1d", "advection_color_1d"}
SHARP = SHARP_1D | {"acoustics_2d", "advection_2d", "shallow_2d", "vc_acoustics_2d", "vc_advection_2d",
                    "shallow_sphere_2d", "euler_5wave_2d", "psystem_fwave_2d"}
SHARP_HIGH = SHARP_1D | {"acoustics_2d", "advection_2d", "euler_5wave_2d"}
SHARP_WAVE = SHARP_1D


def rp_info(rp_id):
    """The record of one id as a dict, or None where the library knows no such solver."""
    info = np.full(10, -7, dtype=np.int32)
    rc = _lib.lib().pcl_rp_info(rp_id, _lib.i(info))
    if rc != 0:
        assert rc == _lib.EINVAL
        assert np.all(info == -7)
        return None
    return dict(zip(FIELDS, (int(v) for v in info)))


@pytest.fixture(scope="module")
def records():
    return {rp_id: rec for rp_id in range(64) for rec in [rp_info(rp_id)] if rec is not None}


def test_accepted_ids_are_the_python_table(records):
    assert len(set(r.id for r in riemann._ALL)) == len(riemann._ALL) == 16
    assert set(records) == {r.id for r in riemann._ALL}
    assert rp_info(-1) is None
    assert b"unknown Riemann solver id" in _lib.lib().pcl_last_error()


def test_null_argument_is_refused():
    assert _lib.lib().pcl_rp_info(riemann.rp_euler_5wave_2d.id, None) == _lib.EINVAL


@pytest.mark.parametrize("rp", riemann._ALL, ids=lambda r: r.name)
def test_sizes_equal_the_python_table(records, rp):
    rec = records[rp.id]
    assert (rec["ndim"], rec["meqn"], rec["mwaves"]) == (rp.ndim, rp.meqn, rp.mwaves)


def test_fwave_exactly_for_the_fwave_solvers(records):
    assert {r.name for r in riemann._ALL if records[r.id]["fwave"]} == {"elasticity_fwave_1d", "psystem_fwave_2d"}
    assert {r.name for r in riemann._ALL if "_fwave_" in r.name} == {"elasticity_fwave_1d", "psystem_fwave_2d"}


def test_derived_record_equals_the_former_rows(records):
    assert set(FORMER_ROWS) == set(riemann.BY_NAME)
    for name, row in FORMER_ROWS.items():
        rec = records[riemann.BY_NAME[name].id]
        got = (rec["ndim"], rec["meqn"], rec["mwaves"], bool(rec["onek"]), bool(rec["onek_aux"]))
        assert got == row, name


def test_one_kernel_step_splits_by_aux(records):
    for r in riemann._ALL:
        rec = records[r.id]
        assert not (rec["onek"] and rec["onek_aux"]), r.name
        if rec["onek"]:
            assert rec["naux"] == 0 and rec["ndim"] == 2, r.name
        if rec["onek_aux"]:
            assert rec["naux"] > 0 and rec["ndim"] == 2, r.name


def test_sharpclaw_coverage(records):
    def having(field):
        return {r.name for r in riemann._ALL if records[r.id][field]}
    assert having("sharp") == SHARP
    assert having("sharp_high") == SHARP_HIGH
    assert having("sharp_wave") == SHARP_WAVE
    assert all(records[r.id][f] in (0, 1) for r in riemann._ALL for f in FIELDS[4:])
