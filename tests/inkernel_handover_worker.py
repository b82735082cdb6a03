"""
Worker of tests/test_gpu_inkernel_handover.py: the Courant number's hand-over of the one-kernel dimension-split step
(classic_fused.hpp) against the two-pass form's, which keeps the single-thread hand-over kernel
(pclaw.hip: cfl_handover).  The form switch PCL_TUNE_FUSED_STEP is read once per process, so the caller starts one
worker per mode and compares the lines: per case, every step call's (entry point, return code, dt.hex(), cfl.hex()),
every undo, and a hash of the final state with -0.0 mapped to +0.0 (the forms' accepted difference:
tests/fused_step_worker.py).

The cases are the smallest shapes at which a count of finished workgroups can go wrong: one tile, four tiles with three
partial ones, a few tiles, list launches far shorter than the grid, full launches with nothing launched behind the step
(pcl_tile_skip off), the fused source with its rejected first step, a solver with another number of equations, a solver
with aux arrays (no bookkeeping: the hand-over kernel is still taken), and one case with an undo, a put and the default
policy's two-pass trial steps between one-kernel steps.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyclaw_amd as pyclaw                     # noqa: E402
from pyclaw_amd import _lib                     # noqa: E402
from apps import problems                       # noqa: E402
import fused_aux_worker as A                    # noqa: E402
import test_gpu_quiet_tiles as Q                # noqa: E402
import test_gpu_tile_handover as T              # noqa: E402

B = pyclaw.BC


class Steps:
    """Records every step call and undo of the library object the solvers call through (no other call is added between
    the steps: they follow each other as in a plain run); sets pcl_tile_skip once per solver handle; runs
    hook(index of the step call, handle, self) behind each step call."""
    NAMES = ("pcl_bc_step", "pcl_step_hyperbolic", "pcl_undo_step")

    def __init__(self, skip=True, hook=None):
        self.skip, self.hook, self.log, self.seen, self.n = skip, hook, [], set(), 0

    def __enter__(self):
        L = _lib.lib()
        self.orig = {n: getattr(L, n) for n in self.NAMES}

        def first(h):
            key = h.value if hasattr(h, "value") else h
            if key not in self.seen:
                self.seen.add(key)
                _lib.check(L.pcl_tile_skip(h, 1 if self.skip else 0))

        def after(tag, h, rc, dt, cfl):
            self.log.append((tag, rc, float(dt).hex(), float(cfl[0]).hex()))
            self.n += 1
            if self.hook is not None:
                self.hook(self.n - 1, h, self)

        def bc_step(h, bc, cs, dt, cfl):
            first(h)
            self.bc_args = (bc, cs, dt)
            rc = self.orig["pcl_bc_step"](h, bc, cs, dt, cfl)
            after("bc_step", h, rc, dt, cfl)
            return rc

        def step(h, dt, cfl):
            first(h)
            rc = self.orig["pcl_step_hyperbolic"](h, dt, cfl)
            after("step", h, rc, dt, cfl)
            return rc

        def undo(h):
            rc = self.orig["pcl_undo_step"](h)
            self.log.append(("undo", rc))
            return rc

        L.pcl_bc_step, L.pcl_step_hyperbolic, L.pcl_undo_step = bc_step, step, undo
        return self

    def __exit__(self, *exc):
        L = _lib.lib()
        for n, f in self.orig.items():
            setattr(L, n, f)
        return False


def state_hash(q):
    return hashlib.sha256(np.ascontiguousarray(q + 0.0).tobytes()).hexdigest()


def run_case(make, skip=True, hook=None):
    claw = make()
    with Steps(skip, hook) as rec:
        claw.run()
        claw.solver.teardown()
    q = claw.solution.state.q
    return {"log": rec.log, "hash": state_hash(q), "finite": bool(np.isfinite(q).all())}


def shockbubble():
    claw = problems.shockbubble(pyclaw, mx=160, my=40, tfinal=0.02, device_callbacks=True, run=False)
    claw.keep_copy = False
    claw.output_format = None
    return claw


def acoustics():
    claw = problems.acoustics2D(pyclaw, mx=480, my=240, tfinal=0.03, nout=1, dim_split=1, run=False)
    claw.keep_copy = False
    claw.output_format = None
    return claw


def interleave_hook(mx, my):
    """an undo and the step taken again, and the state put back byte for byte (not a read-only call: the next launch
    computes every tile), each once among the first steps, once in mid-run and once inside the default mode's trial
    window (steps 64 .. 71 of the form policy: one-kernel trials up to 67, two-pass trials from 68) -- there the put sits
    between one-kernel steps and the undo between two-pass steps"""
    def hook(k, h, rec):
        L = _lib.lib()
        if k in (5, 40, 69):
            cfl = np.zeros(1)
            _lib.check(rec.orig["pcl_undo_step"](h))
            rc = rec.orig["pcl_bc_step"](h, *rec.bc_args, _lib.d(cfl))
            rec.log.append(("retaken", rc, float(cfl[0]).hex()))
        elif k in (11, 50, 65):
            buf = np.empty(5 * mx * my)
            _lib.check(L.pcl_get_q(h, _lib.d(buf), 0))
            _lib.check(L.pcl_put_q(h, _lib.d(buf), 0))
    return hook


def vc_acoustics():
    c = A.vc_acoustics("vc_acoustics_240x120", 240, 120, "layered", [A.PER, A.PER, A.OUT, A.REF], steps=12, seed=7)
    out, cfls, forms = A.gpu_run(c)           # raises on a non-zero return code
    return {"log": [("bc_step", 0, float(c.dt).hex(), float(v).hex()) for v in cfls], "hash": state_hash(out),
            "finite": bool(np.isfinite(out).all()), "forms": forms}


def main():
    per = [B.periodic] * 4
    res = {}
    for mx, my in ((60, 12), (61, 13), (130, 30)):
        res["euler_%dx%d" % (mx, my)] = run_case(Q.euler_case(mx, my, per, Q.blob, steps=10))
    blob = T.euler_case(420, 180, 0.9, T.moving_blob(0.4, 0.2), steps=30)
    res["moving_blob_420x180"] = run_case(blob)
    res["moving_blob_420x180_noskip"] = run_case(blob, skip=False)
    res["shockbubble_160x40"] = run_case(shockbubble)
    res["acoustics_480x240"] = run_case(acoustics)
    res["vc_acoustics_240x120"] = vc_acoustics()
    res["interleaved_600x240"] = run_case(T.euler_case(600, 240, 1.5, T.moving_blob(0.6, 0.2), steps=80),
                                          hook=interleave_hook(600, 240))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
