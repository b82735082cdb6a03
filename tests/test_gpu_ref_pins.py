"""
GPU: the device held to the reference's recorded results directly, not through the oracle.

Every other GPU parity test asserts HIP == oracle.  These run the cases of tests/ref_cases.py through the f2py-shaped
entries (pcl_step1, pcl_step1fw, pcl_step2ds, pcl_step2, pcl_step3ds, pcl_step3) in the default (exact) arithmetic mode
and check the device's own result and Courant numbers against tests/golden/ref_pins.json: what the flang build of the
reference's step and flux Fortran returned around the restated Riemann solvers (oracle/ref_rp_shim.c).  Bit for bit, no
tolerance, no skip.  Only the pins are read, never the reference tree.  The pins cover the step around the solver; the
third-party solver formulas are restated on both sides and stay unpinned.

A pin holds all limiter vectors of a group at once; when one differs, the message adds, per limiter vector, the largest
difference from the oracle (a diagnostic only: the assertion is the pin).

Left out of the GPU leg (the pins still hold the oracle):
  * elasticity_fwave_exp (1-D) and psystem_fwave_exp (2-D), ref_cases.HOST_ONLY: the exponential stress law calls exp()
    inside the Riemann solver, and the device's exp() differs from glibc's by an ulp (measured here: largest difference
    from the oracle 1.1e-16 .. 2.2e-16 per step, Courant numbers equal).  That is solver arithmetic, which these pins do not
    cover, and this leg is bitwise or absent.  The same entries and kernels run here with the linear stress law
    (elasticity_fwave, psystem_fwave_linear); tests/test_fwave.py holds the exponential law to the oracle to 1e-13.
  * nothing is refused: the one combination pcl_create refuses by design in these dimensions is the UNSPLIT 3-D step with a
    capacity function ("3-D: the capacity function is built for the dimension-split step (step3ds); the unsplit step3 with
    mcapa is not"), and ref_cases.py has no such case (3-D capa runs through step3ds only, which the device serves).  Capa
    together with a solver's own aux components (vc_acoustics, vc_advection, psystem_fwave, advection_color) is served
    and is in.
"""
import ctypes as C

import numpy as np
import pytest

import ref_cases as RC
import ref_pins as P

pytestmark = pytest.mark.gpu


def run_device(g):
    """the group on the device -> (compared results stacked over the limiter vectors, their Courant numbers)"""
    from pyclaw_amd import _lib as L
    lib = L.lib()
    outs, cfls = [], []
    n, d, q0 = g["n"], g["d"], g["q"]
    par = np.zeros(8)
    if g["par"] is not None:
        par[:len(g["par"])] = g["par"]
    aux = L.d(g["aux"]) if g["maux"] > 0 else None
    method, meqn, mwaves, maux = g["method"], g["meqn"], g["mwaves"], g["maux"]
    for mth in g["mthlims"]:
        mth = np.array(mth, dtype=np.int32)
        out = q0.copy("F")
        cfl = C.c_double()
        pc = C.cast(C.byref(cfl), L.dp)
        if g["kind"] == "step1":
            fn = lib.pcl_step1fw if g["fwave"] else lib.pcl_step1
            rc = fn(g["rp"], L.d(par), meqn, mwaves, maux, RC.MBC, n[0], L.d(out), aux, d[0], g["dt"], L.i(method), L.i(mth),
                    pc)
        elif g["kind"] == "step2ds":
            rc = lib.pcl_step2ds(g["rp"], L.d(par), int(g["fwave"]), meqn, mwaves, maux, RC.MBC, n[0], n[1], L.d(q0), L.d(out),
                                 aux, d[0], d[1], g["dt"], L.i(method), L.i(mth), pc, g["arg"])
        elif g["kind"] == "step2":
            rc = lib.pcl_step2(g["rp"], L.d(par), int(g["fwave"]), meqn, mwaves, maux, RC.MBC, n[0], n[1], L.d(q0), L.d(out),
                               aux, d[0], d[1], g["dt"], L.i(method), L.i(mth), pc)
        elif g["kind"] == "step3ds":
            rc = lib.pcl_step3ds(g["rp"], L.d(par), meqn, mwaves, maux, RC.MBC, n[0], n[1], n[2], L.d(q0), L.d(out), aux,
                                 d[0], d[1], d[2], g["dt"], L.i(method), L.i(mth), pc, g["arg"])
        else:
            rc = lib.pcl_step3(g["rp"], L.d(par), meqn, mwaves, maux, RC.MBC, n[0], n[1], n[2], L.d(q0), L.d(out), aux, d[0],
                               d[1], d[2], g["dt"], L.i(method), L.i(mth), pc)
        L.check(rc)
        outs.append(RC.compared(g, out).copy())
        cfls.append(cfl.value)
    return np.stack(outs), np.array(cfls)


def _check_block(coracle, dim, block, kinds):
    failed = []
    for key, g in RC.groups(dim, block):
        if g["kind"] not in kinds:
            continue
        out, cfl = run_device(g)
        try:
            P.check(key, out, cfl)
        except AssertionError:
            want, cfl_o = RC.run_host(coracle, g)
            failed.append("%s: max |device - oracle| per limiter vector %s, CFL equal %s"
                          % (key, [float(np.abs(a - b).max()) for a, b in zip(out, want)], (cfl == cfl_o).tolist()))
    assert not failed, "%d groups differ from the pinned reference result:\n%s" % (len(failed), "\n".join(failed[:12]))


@pytest.mark.parametrize("block", RC.blocks(1, device=True), ids=RC.block_id)
def test_step1_equals_reference_pins(coracle, block):
    """pcl_step1 / pcl_step1fw: every limiter, order 1 and 2, with and without capa"""
    _check_block(coracle, 1, block, ("step1",))


@pytest.mark.parametrize("block", RC.blocks(2, device=True), ids=RC.block_id)
def test_step2ds_equals_reference_pins(coracle, block):
    """pcl_step2ds, ids 1 and 2, the whole array: aux rows and capa as component maux+1"""
    _check_block(coracle, 2, block, ("step2ds",))


@pytest.mark.parametrize("block", RC.blocks(2, device=True), ids=RC.block_id)
def test_step2_equals_reference_pins(coracle, block):
    """pcl_step2, trans 0, 1, 2, interior: aux1 / aux2 / aux3 handed to the transverse solver with imp"""
    _check_block(coracle, 2, block, ("step2",))


@pytest.mark.parametrize("block", RC.blocks(3, device=True), ids=RC.block_id)
def test_step3ds_equals_reference_pins(coracle, block):
    """pcl_step3ds in its three directions, with mcapa = 3 too, limiter pairs beyond [4, 3]"""
    _check_block(coracle, 3, block, ("step3ds",))


@pytest.mark.parametrize("block", RC.blocks(3, device=True), ids=RC.block_id)
def test_step3_equals_reference_pins(coracle, block):
    """pcl_step3 in all six transverse modes of flux3.f"""
    _check_block(coracle, 3, block, ("step3",))
