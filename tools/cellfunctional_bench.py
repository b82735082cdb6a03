#!/usr/bin/env python
"""
What a functional costs per call on the resident 4096^2 shock-bubble state: mass and total energy (sums) and the largest
density (max), three ways:

  (a) device    pyclaw.CellFunctional.evaluate in resident mode, the host read of the three doubles included
  (b) python    the route of Controller.write_F with a Python compute_F: download q, compute_F(state), np.sum per
                component (np.max for the density)
  (c) yardstick the no-store pointwise cell function over the same planes: the Euler radial source as a pyclaw.CellSource
                on the initial state (gas at rest: it reads four q planes and aux and stores nothing) -- the "bubble"
                case of tools/cellfn_bench.py

(a) and (c) are timed with a host clock around `--calls` calls that each end in a synchronisation of the stream (what a
caller of evaluate() waits for), alternating, `--reps` times each; (c) also with device events around the launches
alone, which leaves out the host's share.  (b) with a host clock around whole calls.  Before anything is timed the device
values are compared with numpy on the same state.  Bytes per call of (a): the body reads q[0] and q[3], two planes.
Prints one JSON line; needs a GPU.

  python tools/cellfunctional_bench.py [--n 4096] [--calls 50] [--reps 7] [--python-calls 3] [--out FILE]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyclaw_amd as pyclaw                  # noqa: E402
from pyclaw_amd import _lib                  # noqa: E402
from apps import problems                   # noqa: E402

BODY = "f[0] = q[0] * c.d[0] * c.d[1]; f[1] = q[3] * c.d[0] * c.d[1]; f[2] = q[0];"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--python-calls", type=int, default=3)
    ap.add_argument("--math", default="exact")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    if L.pcl_device_count() < 1:
        raise SystemExit("cellfunctional_bench: no HIP device (nothing here can be measured without one)")

    claw = problems.shockbubble(pyclaw, mx=args.n, my=args.n, run=False, math=args.math)
    solver, solution = claw.solver, claw.solution
    state = solution.state
    cell = pyclaw.CellSource(problems.EULER_RAD_CELL_SRC, params=[problems.gamma1, 2])
    solver.step_src = cell
    solver.setup(solution)
    solver.begin_resident(solution)
    F = pyclaw.CellFunctional(BODY, 3, reduce=('sum', 'sum', 'max'))
    dx, dy = state.grid.d
    med = lambda v: float(np.median(v))
    stat = lambda v: {"median": med(v), "min": min(v), "max": max(v), "all": v}
    plane = 8.0 * args.n * args.n
    ms = ctypes.c_float()

    def compute_F(st):
        st.F[0] = st.q[0] * dx * dy
        st.F[1] = st.q[3] * dx * dy
        st.F[2] = st.q[0]

    state.mF = 3

    def python_route():
        solver._host_stale = True
        solver._pull(state)
        compute_F(state)
        return [float(np.sum(state.F[0])), float(np.sum(state.F[1])), float(np.max(state.F[2]))]

    # the values first: the sums within the order-free bound N u sum|f| of the exact sum, the maximum bitwise
    got = F.evaluate(solver, state)
    want = python_route()
    ncell = args.n * args.n
    exact = [math.fsum(state.F[0].ravel()), math.fsum(state.F[1].ravel())]
    bound = [ncell * 2.0 ** -53 * e for e in exact]           # (both integrands are positive: sum|f| is the sum)
    ok = all(abs(got[k] - exact[k]) <= bound[k] for k in range(2)) and got[2] == want[2]
    res = {"tool": "cellfunctional_bench", "n": args.n, "math": args.math, "calls": args.calls, "reps": args.reps,
           "device_values": [float(v) for v in got], "numpy_values": want, "fsum_values": exact,
           "device_minus_fsum": [float(got[k] - exact[k]) for k in range(2)], "bound": bound, "values_agree": bool(ok),
           "functional_bytes_per_call": 2 * plane, "yardstick_bytes_per_call": 5 * plane}

    def timed_functional():
        F.evaluate(solver, state)
        t0 = time.perf_counter()
        for _ in range(args.calls):
            F.evaluate(solver, state)
        return 1e3 * (time.perf_counter() - t0) / args.calls

    def timed_yardstick_host():
        cell.apply(solver, state, 1e-8)
        _lib.check(L.pcl_sync(solver._h))
        t0 = time.perf_counter()
        for _ in range(args.calls):
            cell.apply(solver, state, 1e-8)
            _lib.check(L.pcl_sync(solver._h))
        return 1e3 * (time.perf_counter() - t0) / args.calls

    def timed_yardstick_events():
        _lib.check(L.pcl_sync(solver._h))
        _lib.check(L.pcl_timer_start(solver._h))
        for _ in range(args.calls):
            cell.apply(solver, state, 1e-8)
        _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
        return ms.value / args.calls

    a, c, ce = [], [], []
    for _ in range(args.reps):
        a.append(timed_functional())
        c.append(timed_yardstick_host())
        ce.append(timed_yardstick_events())
    again = F.evaluate(solver, state)
    res["repeatable_bitwise"] = bool(np.array_equal(again.view(np.uint64), got.view(np.uint64)))
    b = []
    for _ in range(args.python_calls + 1):
        t0 = time.perf_counter()
        python_route()
        b.append(1e3 * (time.perf_counter() - t0))
    b = b[1:]                                             # the first call allocates the host temporaries
    solver.end_resident(solution)
    solver.teardown()
    res["device_ms"] = stat(a)
    res["python_ms"] = stat(b)
    res["yardstick_ms"] = stat(c)
    res["yardstick_events_ms"] = stat(ce)
    res["device_GBps"] = 2 * plane / med(a) / 1e6
    res["yardstick_GBps"] = 5 * plane / med(c) / 1e6
    res["device_over_yardstick"] = med(a) / med(c)
    res["python_over_device"] = med(b) / med(a)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
