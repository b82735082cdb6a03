#!/usr/bin/env python
"""
What gauges cost per step of the resident 4096^2 shock-bubble run (bench.py's state: device callbacks, no source term,
begin_resident, the one-kernel step with the next step enqueued ahead), three ways, each through
solver.evolve_to_time(solution, tend):

  (a) none     no gauges
  (b) gather   16 gauges, solver.gauge_log = False: pcl_get_cells after every accepted step (an upload of the indices, a
               gather launch, a download and a synchronisation of the solver's stream -- behind the step enqueued ahead)
  (c) log      16 gauges, solver.gauge_log = True: every step records its gauge cells into the device log (pcl_gauge_log),
               the lines are written when evolve_to_time returns

One solver per arm, all three alive at once; a segment is one evolve_to_time call of about `--steps` steps, timed with a
host clock between two device synchronisations (the log's read-back and the writing of the lines are inside the window);
the arms take turns, `--reps` segments each, after `--warmup` segments -- by default 3200 steps per arm in all, which
keeps the run in the early, quiet-tile state bench.py measures (its 2000 steps).  The gauge files of (b) and (c) are compared byte for
byte at the end.  Prints one JSON line with ms per accepted step (median, min, max and every segment) and the step-ahead
counts of each arm; needs a GPU.

  python tools/gauge_bench.py [--n 4096] [--steps 400] [--reps 7] [--warmup 1] [--gauges 16] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyclaw_amd as pyclaw                  # noqa: E402
from pyclaw_amd import _lib                  # noqa: E402
from apps import problems                   # noqa: E402


class Arm:
    def __init__(self, name, n, ngauges, log, outdir):
        self.name = name
        dt0 = 0.005 * (2.0 / n) / (2.0 / 160.0)                   # as bench.py scales it
        claw = problems.shockbubble(pyclaw, mx=n, my=n, device_callbacks=True, with_src=False, dt_initial=dt0, run=False)
        self.solver, self.solution = claw.solver, claw.solution
        grid = self.solution.state.grid
        grid.gauge_path = os.path.join(outdir, name) + os.sep
        if ngauges:
            # spread over the grid, the quiet gas ahead of the shock and the region behind it alike
            rng = np.random.default_rng(1)
            cells = np.stack([rng.integers(0, n, ngauges), rng.integers(0, n, ngauges)], axis=1)
            grid.add_gauges([((i + 0.5) * grid.d[0], (j + 0.5) * grid.d[1]) for i, j in cells.tolist()])
        self.solver.gauge_log = log
        self.solver.setup(self.solution)
        self.solver.dt = self.solver.dt_initial
        self.solver.begin_resident(self.solution)
        self.ms, self.steps = [], 0

    def segment(self, nsteps, keep):
        L, s = _lib.lib(), self.solver
        s.max_steps = 4 * nsteps                                   # (the default, 1000, is what one call may take)
        _lib.check(L.pcl_sync(s._h))
        t0 = time.perf_counter()
        st = s.evolve_to_time(self.solution, self.solution.t + nsteps * s.dt)
        _lib.check(L.pcl_sync(s._h))
        t1 = time.perf_counter()
        if keep:
            self.ms.append(1e3 * (t1 - t0) / st['numsteps'])
            self.steps += st['numsteps']

    def ahead(self):
        a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        _lib.check(_lib.lib().pcl_step_ahead_stats(self.solver._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"enqueued": a.value, "adopted": b.value, "dropped": c.value}

    def finish(self):
        res = {"ms_per_step": {"median": float(np.median(self.ms)), "min": min(self.ms), "max": max(self.ms), "all": self.ms},
               "timed_steps": self.steps, "step_ahead": self.ahead(),
               "step_ahead_armed": bool((getattr(self.solver, '_step_ahead_sent', None) or (0,))[0])}
        self.solver.end_resident(self.solution)
        self.solver.teardown()
        res["step_forms"] = self.solver.status.get("step_forms")
        files = []
        for f in self.solution.state.grid.gauge_files:
            f.close()
            files.append(open(f.name, "rb").read())
        return res, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gauges", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if _lib.lib().pcl_device_count() < 1:
        raise SystemExit("gauge_bench: no HIP device (nothing here can be measured without one)")
    with tempfile.TemporaryDirectory() as tmp:
        arms = [Arm("none", args.n, 0, True, tmp), Arm("gather", args.n, args.gauges, False, tmp),
                Arm("log", args.n, args.gauges, True, tmp)]
        for k in range(args.warmup + args.reps):
            for arm in arms:
                arm.segment(args.steps, k >= args.warmup)
        out = {arm.name: arm.finish() for arm in arms}
    res = {"tool": "gauge_bench", "n": args.n, "gauges": args.gauges, "steps_per_segment": args.steps, "reps": args.reps,
           "warmup_segments": args.warmup, "gauge_files_equal_bytewise": out["gather"][1] == out["log"][1],
           "gauge_lines": out["log"][1][0].count(b"\n") if out["log"][1] else 0}
    for name, (r, _) in out.items():
        res[name] = r
    med = lambda name: res[name]["ms_per_step"]["median"]
    spread = lambda name: res[name]["ms_per_step"]["max"] - res[name]["ms_per_step"]["min"]
    res["gather_minus_log_ms"] = med("gather") - med("log")
    res["log_minus_none_ms"] = med("log") - med("none")
    res["spreads_added_ms"] = spread("gather") + spread("log")
    res["gain_counts"] = bool(res["gather_minus_log_ms"] > res["spreads_added_ms"])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
