#!/usr/bin/env python
"""
What the shock-bubble inflow state costs per application on the lower x side of the resident 4096^2 Euler state
(mbc 2), three ways, each through the call apply_q_bcs makes for a custom side (Solver._custom_bc):

  (a) builtin   pyclaw.ConstantStateBC: the built-in constant-state fill, pcl_bc_const (the yardstick)
  (b) cell      the same state restated as a cell function (pyclaw.CellBC, `q[m] = p[m]`), pcl_cellbc_apply
  (c) python    the reference's numpy shockbc around a download of the whole ghosted q and an upload of the strip

(a) and (b) are timed with device events around `--calls` applications, alternating, `--reps` times each; (c) with a
host clock around whole calls (it ends in a synchronous upload).  Before anything is timed the three are applied to the
same ghosted array and compared bit for bit.  Both device fills write mbc * (n + 2 mbc) * 5 doubles, a few hundred KB:
what is measured is a launch, not bandwidth.  Prints one JSON line; needs a GPU.

  python tools/cellbc_bench.py [--n 4096] [--calls 200] [--reps 7] [--python-calls 2] [--out FILE]
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

BODY = "for (int m = 0; m < MEQN; m++) q[m] = p[m];"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--python-calls", type=int, default=2)
    ap.add_argument("--math", default="exact")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    if L.pcl_device_count() < 1:
        raise SystemExit("cellbc_bench: no HIP device (nothing here can be measured without one)")

    claw = problems.shockbubble(pyclaw, mx=args.n, my=args.n, run=False, math=args.math, with_src=False)
    solver, state = claw.solver, claw.solution.state
    rinf, vinf, einf = problems.shock_state()
    inflow = [rinf, rinf * vinf, 0., einf, 0.]
    fills = {"builtin": pyclaw.ConstantStateBC(inflow), "cell": pyclaw.CellBC(BODY, params=inflow),
             "python": problems.shockbc}
    solver.user_bc_lower = fills["cell"]
    t0 = time.perf_counter()
    solver.setup(claw.solution)
    setup_s = time.perf_counter() - t0
    solver._push(state)
    dim = state.grid.dimensions[0]
    mbc = solver.mbc
    ms = ctypes.c_float()
    med = lambda v: float(np.median(v))

    def apply(fn):
        solver._custom_bc(state, dim, 0, 0, fn)

    def frame(fn):
        """the lower x ghost columns, corners included, after one application on a frame of NaNs"""
        strip = np.full((state.meqn, mbc, args.n + 2 * mbc), np.nan, order='F')
        _lib.check(L.pcl_put_strip(solver._h, 0, 0, mbc, _lib.d(strip)))
        apply(fn)
        _lib.check(L.pcl_get_strip(solver._h, 0, 0, mbc, _lib.d(strip)))
        return strip

    strips = {name: frame(fn) for name, fn in fills.items()}
    same = all(np.array_equal(strips["builtin"].view(np.uint64), s.view(np.uint64)) for s in strips.values())

    def timed(fn):
        apply(fn)                                         # warm: the first launch loads the code object
        _lib.check(L.pcl_sync(solver._h))
        _lib.check(L.pcl_timer_start(solver._h))
        for _ in range(args.calls):
            apply(fn)
        _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
        return ms.value / args.calls

    a, b = [], []
    for _ in range(args.reps):
        a.append(timed(fills["builtin"]))
        b.append(timed(fills["cell"]))
    c = []
    for _ in range(args.python_calls + 1):
        t0 = time.perf_counter()
        apply(fills["python"])
        _lib.check(L.pcl_sync(solver._h))
        c.append(1e3 * (time.perf_counter() - t0))
    c = c[1:]                                             # the first call touches the host staging array for the first time
    solver.teardown()
    res = {"tool": "cellbc_bench", "n": args.n, "mbc": mbc, "math": args.math, "calls": args.calls, "reps": args.reps,
           "setup_s": setup_s, "ghost_cells_per_application": mbc * (args.n + 2 * mbc),
           "three_fills_equal_bitwise": bool(same),
           "builtin_ms": {"median": med(a), "min": min(a), "max": max(a), "all": a},
           "cell_ms": {"median": med(b), "min": min(b), "max": max(b), "all": b},
           "python_ms": {"median": med(c), "min": min(c), "max": max(c), "all": c},
           "cell_over_builtin": med(b) / med(a), "python_over_cell": med(c) / med(b)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
