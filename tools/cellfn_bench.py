#!/usr/bin/env python
"""
What a source term costs per call on the resident 4096^2 shock-bubble state, three ways:

  (a) builtin   the built-in src_euler_radial kernel through pcl_src (the yardstick)
  (b) cell      the same arithmetic as a cell function (pyclaw.CellSource, problems.EULER_RAD_CELL_SRC)
  (c) python    the reference's numpy euler_rad_src around a device -> host -> device round trip of q

(a) and (b) are timed with device events around `--calls` launches, alternating, `--reps` times each, on two states: the
initial condition (gas at rest: the source changes no value, and a cell function stores only values that changed) and
the same with both momenta non-zero everywhere (every value of the four components changes); (c) with a host clock around whole calls (it ends in
a synchronous upload).  Before a state is timed (a) and (b) are applied to it and compared bit for bit.  Bytes per call
of (a) and (b) where every cell changes: four of the five q planes read and written plus one aux plane read.  Prints one
JSON line; needs a GPU.

  python tools/cellfn_bench.py [--n 4096] [--calls 50] [--reps 7] [--python-calls 2] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--python-calls", type=int, default=2)
    ap.add_argument("--math", default="exact")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    if L.pcl_device_count() < 1:
        raise SystemExit("cellfn_bench: no HIP device (nothing here can be measured without one)")

    claw = problems.shockbubble(pyclaw, mx=args.n, my=args.n, run=False, math=args.math)
    solver, state = claw.solver, claw.solution.state
    builtin = pyclaw.EulerRadialSource(problems.gamma1, 2)
    cell = pyclaw.CellSource(problems.EULER_RAD_CELL_SRC, params=[problems.gamma1, 2])
    solver.step_src = cell
    t0 = time.perf_counter()
    solver.setup(claw.solution)
    setup_s = time.perf_counter() - t0
    dt = 1e-8
    ms = ctypes.c_float()
    med = lambda v: float(np.median(v))
    plane = 8.0 * args.n * args.n
    nbytes = (4 * 2 + 1) * plane          # the built-in kernel: 4 q planes + aux read, 4 q planes written, whatever the state
    res = {"tool": "cellfn_bench", "n": args.n, "math": args.math, "calls": args.calls, "reps": args.reps,
           "setup_s": setup_s, "builtin_bytes_per_call": nbytes, "states": {}}

    def after(src, q0):
        state.q[...] = q0
        solver._push(state)
        src.apply(solver, state, dt)
        solver._host_stale = True
        solver._pull(state)
        return state.q.copy('F')

    def timed(src):
        src.apply(solver, state, dt)                      # warm: the first launch loads the code object
        _lib.check(L.pcl_sync(solver._h))
        _lib.check(L.pcl_timer_start(solver._h))
        for _ in range(args.calls):
            src.apply(solver, state, dt)
        _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
        return ms.value / args.calls

    # "bubble": the shock-bubble initial condition -- the gas is at rest (q[2] = 0), so the source returns every cell bit
    # for bit and the cell function's store-if-changed writes nothing; "moving": the same state with both momenta
    # non-zero everywhere, so that all four components change in (nearly) every cell
    q_bubble = state.q.copy('F')
    q_moving = q_bubble.copy('F')
    rng = np.random.default_rng(7)
    q_moving[1] = 0.03 * q_moving[0] * (1.0 + rng.random(q_moving[0].shape))
    q_moving[2] = 0.05 * q_moving[0] * (1.0 + rng.random(q_moving[0].shape))
    for name, q0 in (("bubble", q_bubble), ("moving", q_moving)):
        qa, qb = after(builtin, q0), after(cell, q0)
        same = bool(np.array_equal(qa.view(np.uint64), qb.view(np.uint64)))
        changed = float(np.mean(qa.view(np.uint64)[:4] != q0.view(np.uint64)[:4]))
        state.q[...] = q0
        solver._push(state)
        a, b = [], []
        for _ in range(args.reps):
            a.append(timed(builtin))
            b.append(timed(cell))
        res["states"][name] = {
            "cell_equals_builtin_bitwise": same, "fraction_of_values_changed_by_one_call": changed,
            "builtin_ms": {"median": med(a), "min": min(a), "max": max(a), "all": a},
            "cell_ms": {"median": med(b), "min": min(b), "max": max(b), "all": b},
            # the cell function stores a value only where its bits changed: 4 q planes + aux read, 4 * changed written
            "cell_bytes_per_call": (5 + 4 * changed) * plane,
            "builtin_GBps": nbytes / med(a) / 1e6, "cell_GBps": (5 + 4 * changed) * plane / med(b) / 1e6,
            "cell_over_builtin": med(b) / med(a)}

    c = []
    state.q[...] = q_bubble
    solver._push(state)
    solver.step_src = problems.euler_rad_src
    for _ in range(args.python_calls + 1):
        t0 = time.perf_counter()
        solver._host_stale = True
        solver._apply_src(state, dt)
        _lib.check(L.pcl_sync(solver._h))
        c.append(1e3 * (time.perf_counter() - t0))
    c = c[1:]                                             # the first call allocates the host temporaries
    solver.teardown()
    res["python_ms"] = {"median": med(c), "min": min(c), "max": max(c), "all": c}
    res["python_over_cell"] = med(c) / res["states"]["moving"]["cell_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
