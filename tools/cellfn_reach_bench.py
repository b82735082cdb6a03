#!/usr/bin/env python
"""
What a cell function that reads neighbour cells costs per call on the resident 4096^2 Euler (shock-bubble) state:

  (a) pointwise   problems.EULER_RAD_CELL_SRC (reach = 0), the kernel of tools/cellfn_bench.py: the check that neighbour
                  reads cost a pointwise function nothing.  `--pointwise-only` measures this alone and uses nothing a
                  tree without `reach` lacks, so the same file runs in a checkout of the parent commit.
  (b) stencil     the 5-point diffusion of all five components, pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC,
                  reach=1): the whole call (ghost fill + snapshot + kernel), and its parts from device events on the
                  solver stream -- the ghost fill (apply_q_bcs alone), the snapshot (the same device-to-device copy of q
                  through pcl_backup) and snapshot + kernel (CellFunction.launch, which skips the fill); the kernel is
                  the difference of the last two medians.
  (c) python      its numpy twin problems.diffusion_src around a device -> host -> device round trip of q (host clock).

Every figure is ms per call: the median (min - max) of `--reps` segments of `--calls` calls.  The state has noise on every
component, so that (nearly) every value changes and every plane is stored.  Bytes of (b): the snapshot reads and writes
the five q planes; the kernel reads them once (neighbours come from L1 / L2) and writes the planes that changed.  Prints
one JSON line; needs a GPU.

  python tools/cellfn_reach_bench.py [--n 4096] [--calls 50] [--reps 7] [--python-calls 1] [--pointwise-only] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyclaw_amd as pyclaw                  # noqa: E402
from pyclaw_amd import _lib                  # noqa: E402
from apps import problems                   # noqa: E402

COPY_GBPS = 5577.0        # hipMemcpyAsync D2D of five 4096^2 planes, profiles/r02_copy_rates.txt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--python-calls", type=int, default=1)
    ap.add_argument("--nu", type=float, default=1e-6)
    ap.add_argument("--pointwise-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    if L.pcl_device_count() < 1:
        raise SystemExit("cellfn_reach_bench: no HIP device (nothing here can be measured without one)")

    # device boundary conditions: the ghost fill in front of a stencil launch never leaves the device
    claw = problems.shockbubble(pyclaw, mx=args.n, my=args.n, run=False, device_callbacks=True)
    solver, state = claw.solver, claw.solution.state
    point = pyclaw.CellSource(problems.EULER_RAD_CELL_SRC, params=[problems.gamma1, 2])
    solver.step_src = point
    solver.setup(claw.solution)
    dt = 1e-8
    ms = ctypes.c_float()
    plane = 8.0 * args.n * args.n

    def stat(v):
        return {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": v}

    def segment(call):
        call()                                            # warm: the first launch loads the code object / allocates
        _lib.check(L.pcl_sync(solver._h))
        _lib.check(L.pcl_timer_start(solver._h))
        for _ in range(args.calls):
            call()
        _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
        return ms.value / args.calls

    rng = np.random.default_rng(7)
    q0 = state.q.copy('F')
    q0[1] = 0.03 * q0[0]
    q0[2] = 0.05 * q0[0]
    for m in range(5):
        q0[m] = (q0[m] + (0.0 if m < 4 else 0.5)) * (1.0 + 0.01 * rng.random(q0[m].shape))
    state.q[...] = q0
    solver._push(state)
    res = {"tool": "cellfn_reach_bench", "label": args.label, "n": args.n, "calls": args.calls, "reps": args.reps,
           "plane_bytes": plane}

    a = [segment(lambda: point.apply(solver, state, dt)) for _ in range(args.reps)]
    res["pointwise_ms"] = stat(a)
    if not args.pointwise_only:
        stencil = pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC, params=[args.nu, 0], reach=1)
        # what one call changes, and that it computes what its numpy twin does
        rinf, vinf, einf = problems.shock_state()
        modes = [([rinf, rinf * vinf, 0., einf, 0.], 'edge'), ('wall', 'edge')]
        state.q[...] = q0
        solver._push(state)
        stencil.apply(solver, state, dt)
        solver._host_stale = True
        solver._pull(state)
        got = state.q.copy('F')
        state.q[...] = q0
        t0 = time.perf_counter()
        problems.diffusion_src(args.nu, modes)(solver, state, dt)
        numpy_alone_ms = 1e3 * (time.perf_counter() - t0)
        res["stencil_equals_numpy_bitwise"] = bool(np.array_equal(got, state.q))
        changed = float(np.mean(got.view(np.uint64) != q0.view(np.uint64)))
        res["fraction_of_values_changed_by_one_call"] = changed
        state.q[...] = q0
        solver._push(state)

        total, fill, snap, launch, b2 = [], [], [], [], []
        for _ in range(args.reps):
            total.append(segment(lambda: stencil.apply(solver, state, dt)))
            fill.append(segment(lambda: solver.apply_q_bcs(state)))
            snap.append(segment(lambda: _lib.check(L.pcl_backup(solver._h))))
            launch.append(segment(lambda: stencil.launch(solver, state.t, dt)))
            b2.append(segment(lambda: point.apply(solver, state, dt)))
        res["pointwise_ms_interleaved"] = stat(b2)
        res["stencil_ms"] = {"total": stat(total), "ghost_fill": stat(fill), "snapshot": stat(snap),
                             "snapshot_plus_kernel": stat(launch)}
        kernel = res["stencil_ms"]["snapshot_plus_kernel"]["median"] - res["stencil_ms"]["snapshot"]["median"]
        res["stencil_ms"]["kernel_by_difference"] = kernel
        snap_bytes, kernel_bytes = 2 * 5 * plane, (5 + 5 * changed) * plane
        res["stencil_bytes"] = {"snapshot": snap_bytes, "kernel": kernel_bytes}
        res["stencil_GBps"] = {"snapshot": snap_bytes / res["stencil_ms"]["snapshot"]["median"] / 1e6,
                               "kernel": kernel_bytes / kernel / 1e6,
                               "total": (snap_bytes + kernel_bytes) / res["stencil_ms"]["total"]["median"] / 1e6}
        res["copy_rate_GBps"] = COPY_GBPS
        res["fraction_of_copy_rate"] = {k: v / COPY_GBPS for k, v in res["stencil_GBps"].items()}

        c = []
        solver.step_src = problems.diffusion_src(args.nu, modes)
        for _ in range(args.python_calls + 1):
            t0 = time.perf_counter()
            solver._host_stale = True
            solver._apply_src(state, dt)
            _lib.check(L.pcl_sync(solver._h))
            c.append(1e3 * (time.perf_counter() - t0))
        c = c[1:]                                         # the first call allocates the host temporaries
        res["python_ms"] = stat(c)
        res["python_numpy_alone_ms"] = numpy_alone_ms
        res["python_over_stencil"] = res["python_ms"]["median"] / res["stencil_ms"]["total"]["median"]
    solver.teardown()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
