#!/usr/bin/env python
"""
What SharpClaw costs in 3-D (SharpClawSolver3D over a SharpCellRiemann3D: sharp3_kernel, csrc/sharpclaw.hpp), measured in one
job with the arms taking turns:

  vc3d_pulse   256^3 variable-coefficient acoustics (VC_ACOUSTICS_3D_RP, WENO5), the plane pulse of the acoustics app:
               ms per SSP104 step and, from the library's per-launch events (pcl_kernel_timing), ms per x, y and z pass;
  vc3d_dense   the same solver on a state with a jump at every interface (every cell different);
  vc2d         4096^2 variable-coefficient acoustics through CellRiemann(VC_ACOUSTICS_2D_RP, sharpclaw=True) -- the same number
               of cells -- ms per SSP104 step and per x and y pass: the yardstick;
  euler3d      256^3 Euler equations (EULER_3D_RP), ms per SSP104 step and per pass.

Segments of `--steps` steps alternate between the arms; each figure is the median (min - max) of `--reps` segments.  Times
are device events around the enqueued work (pcl_timer_start / _stop), after `--warmup` steps.  The cost per cell and pass is
reported against the 2-D y pass.  Also records the cold compile time of each 3-D handle in this process.  Writes one JSON line
(`--out`, default profiles/sharp3_bench.json).  Needs a GPU.

`--resource-usage` needs none: it compiles the handles with PCL_CELLFN_DUMP set and writes VGPRs, SGPRs, LDS, scratch and
spills of every sharp3_kernel from the code objects' metadata (default profiles/sharp3_resource_usage.txt).

  python tools/sharp3_bench.py [--n 256] [--n2 4096] [--steps 2] [--warmup 1] [--reps 7] [--out FILE]
  python tools/sharp3_bench.py --resource-usage [--out FILE]
"""
import argparse
import ctypes
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")

# (name, body, meqn, mwaves, aux, capa, lim_type, weno_order, params)
HANDLES = [("vc_acoustics_3d weno5", "VC_ACOUSTICS_3D_RP", 4, 2, (0, 1), False, 2, 5, ()),
           ("vc_acoustics_3d weno5 capa", "VC_ACOUSTICS_3D_RP", 4, 2, (0, 1), True, 2, 5, ()),
           ("vc_acoustics_3d tvd2", "VC_ACOUSTICS_3D_RP", 4, 2, (0, 1), False, 1, 5, ()),
           ("vc_acoustics_3d legacy weno5", "VC_ACOUSTICS_3D_RP", 4, 2, (0, 1), False, 3, 5, ()),
           ("vc_acoustics_3d weno7 capa", "VC_ACOUSTICS_3D_RP", 4, 2, (0, 1), True, 2, 7, ()),
           ("vc_acoustics_3d weno17", "VC_ACOUSTICS_3D_RP", 4, 2, (0, 1), False, 2, 17, ()),
           ("euler_3d weno5", "EULER_3D_RP", 5, 3, (), False, 2, 5, (1.4,)),
           ("euler_3d weno9", "EULER_3D_RP", 5, 3, (), False, 2, 9, (1.4,))]
KEYS = (".name", ".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")


def spread(vals):
    return {"median": float(np.median(vals)), "min": min(vals), "max": max(vals), "all": vals}


def resource_usage(out):
    """each handle in a process of its own, so that every compile is this process's first and its code object is number 0"""
    lines = ["# sharp3_kernel<UserRp, DIR, CAPA, LIM, K> compiled at run time for gfx950, exact mode: per kernel (DIR 1, 2, 3) the",
             "# figures of the code object's metadata (llvm-readelf --notes); compile = wall time of the compile call in a fresh",
             "# process on the build machine (the compiler's own start included)", ""]
    for name, body, meqn, mw, aux, capa, lim, order, par in HANDLES:
        with tempfile.TemporaryDirectory() as d:
            code = ("import sys, time; sys.path.insert(0, %r)\nimport pyclaw_amd as pyclaw\nfrom apps import problems\nt = time.time()\n"
                    "pyclaw.SharpCellRiemann3D(problems.%s + '// %f\\n', %d, %d, params=%r, aux=%r, capa=%r).compile('exact', sharp=(%d, %d))\n"
                    "print(time.time() - t)\n" % (ROOT, body, time.time(), meqn, mw, list(par), aux, capa, lim, order))
            env = dict(os.environ, PCL_CELLFN_DUMP=d)
            p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if p.returncode != 0:
                raise SystemExit("sharp3_bench: compile of %s failed:\n%s" % (name, p.stdout[-2000:]))
            lines.append("== %s: meqn %d, aux %r, capa %r, lim_type %d, weno_order %d; compile %.2f s"
                         % (name, meqn, aux, capa, lim, order, float(p.stdout.strip().splitlines()[-1])))
            for co in sorted(glob.glob(os.path.join(d, "*.co"))):
                notes = subprocess.run([READELF, "--notes", co], stdout=subprocess.PIPE, text=True, check=True).stdout
                cur = {}        # a kernel's keys come in alphabetical order: .vgpr_spill_count ends its block
                for ln in notes.splitlines():
                    ln = ln.strip()
                    for k in KEYS:
                        if ln.startswith(k + ":"):
                            cur[k] = ln.split(":", 1)[1].strip()
                    if ln.startswith(".vgpr_spill_count:"):
                        if len(cur) == len(KEYS) and "sharp3_kernel" in cur[".name"]:
                            lines.append("   " + "  ".join("%s %s" % (k[1:], cur[k]) for k in KEYS[1:]) + "  " + cur[".name"])
                        cur = {}
            lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines))
    print("sharp3_bench: %d handles -> %s" % (len(HANDLES), out))


class Arm(object):
    """one solver, resident, stepping with a fixed dt; ms per step by device events, ms per pass by the library's launch events"""

    def __init__(self, name, claw, cells, ndim, dt):
        from pyclaw_amd import _lib
        self.name, self.claw, self.cells, self.ndim = name, claw, cells, ndim
        t = time.time()
        claw.solver.setup(claw.solution)
        self.setup_s = time.time() - t
        claw.solver.dt_variable = False
        claw.solver.dt = dt
        claw.solver.begin_resident(claw.solution)
        self.L, self._lib = _lib.lib(), _lib
        self.step_ms, self.pass_ms, self.rejected = [], [[] for _ in range(ndim)], 0

    def steps(self, n):
        for _ in range(n):
            self.rejected += self.claw.solver.step(self.claw.solution) is False

    def segment(self, n):
        L, _lib, h = self.L, self._lib, self.claw.solver._h
        ms = ctypes.c_float()
        _lib.check(L.pcl_sync(h))
        _lib.check(L.pcl_timer_start(h))
        self.steps(n)
        _lib.check(L.pcl_timer_stop(h, ctypes.byref(ms)))
        self.step_ms.append(ms.value / n)
        # the same steps again with an event pair around every launch: ms per pass (x, y in the first two slots, z in the third)
        _lib.check(L.pcl_kernel_timing(h, 1))
        self.steps(n)
        t2, n2 = np.zeros(2), np.zeros(2, dtype=np.int64)
        _lib.check(L.pcl_kernel_timing_read(h, _lib.d(t2), n2.ctypes.data_as(ctypes.POINTER(ctypes.c_long))))
        t3, n3, a, b = ctypes.c_double(), ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        _lib.check(L.pcl_step_form_stats(h, ctypes.cast(ctypes.byref(t3), _lib.dp), ctypes.byref(n3), ctypes.byref(a), ctypes.byref(b)))
        _lib.check(L.pcl_kernel_timing(h, 0))
        tot, cnt = [t2[0], t2[1], t3.value], [int(n2[0]), int(n2[1]), int(n3.value)]
        for k in range(self.ndim):
            self.pass_ms[k].append(tot[k] / max(cnt[k], 1))

    def result(self):
        passes = {"xyz"[k]: spread(self.pass_ms[k]) for k in range(self.ndim)}
        for v in passes.values():
            v["ns_per_cell"] = v["median"] * 1e6 / self.cells
        return {"cells": self.cells, "ms_per_step": spread(self.step_ms), "ms_per_pass": passes, "setup_s": self.setup_s,
                "rejected_steps": int(self.rejected), "cfl": self.claw.solver.cfl.get_cached_max()}

    def close(self):
        self.claw.solver.end_resident(self.claw.solution)
        self.claw.solver.teardown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--n2", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--math", default="exact")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resource-usage", dest="resource_usage", action="store_true")
    args = ap.parse_args()
    if args.resource_usage:
        return resource_usage(args.out or os.path.join(ROOT, "profiles", "sharp3_resource_usage.txt"))

    import pyclaw_amd as pyclaw
    from pyclaw_amd import _lib
    from apps import problems
    if _lib.lib().pcl_device_count() < 1:
        raise SystemExit("sharp3_bench: no HIP device (nothing here can be measured without one)")
    n, n2 = args.n, args.n2
    rng = np.random.default_rng(1)
    arms = []

    def vc3(name, dense):
        claw = problems.acoustics3D(pyclaw, mx=n, my=n, mz=n, run=False, math=args.math, solver_type='sharpclaw')
        if dense:
            st = claw.solution.state
            st.q[...] = rng.uniform(-1.0, 1.0, st.q.shape)
        return Arm(name, claw, n ** 3, 3, 0.4 * 2.0 / n)        # a Courant number of 0.4 per direction (c = 1)
    arms.append(vc3("vc3d_pulse", False))
    arms.append(vc3("vc3d_dense", True))
    claw = problems.vc_acoustics2D(pyclaw, mx=n2, my=n2, run=False, math=args.math)
    solver = pyclaw.SharpClawSolver2D()
    old = claw.solver
    solver.rp = pyclaw.CellRiemann(problems.VC_ACOUSTICS_2D_RP, 3, 2, 2, aux=(0, 1), sharpclaw=True)
    solver.mwaves, solver.math = 2, args.math
    for k in range(2):
        solver.bc_lower[k], solver.bc_upper[k] = old.bc_lower[k], old.bc_upper[k]
        solver.aux_bc_lower[k], solver.aux_bc_upper[k] = old.aux_bc_lower[k], old.aux_bc_upper[k]
    claw.solver = solver
    d2 = float(claw.solution.state.grid.d[0])
    cmax = float(claw.solution.state.aux[1].max())
    arms.append(Arm("vc2d", claw, n2 * n2, 2, 0.4 * d2 / cmax))
    claw = problems.euler3D(pyclaw, n=n, across=(n, n), run=False, math=args.math, solver_type='sharpclaw')
    arms.append(Arm("euler3d", claw, n ** 3, 3, 0.2 / n))

    for a in arms:
        a.steps(args.warmup)
    for r in range(args.reps):
        for a in arms:
            a.segment(args.steps)
        print("round %d: " % (r + 1) + ", ".join("%s %.2f ms" % (a.name, a.step_ms[-1]) for a in arms), file=sys.stderr, flush=True)
    res = {"tool": "sharp3_bench", "n": n, "n2": n2, "math": args.math, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "what": "ms per SSP104 step (ten stages) and per directional pass, segments alternating between the arms in one process; "
                   "median (min - max) of the segments",
           "arms": {a.name: a.result() for a in arms}}
    y2 = res["arms"]["vc2d"]["ms_per_pass"]["y"]["ns_per_cell"]
    res["pass_cost_over_2d_y"] = {a.name: {k: v["ns_per_cell"] / y2 for k, v in res["arms"][a.name]["ms_per_pass"].items()}
                                  for a in arms}
    for a in arms:
        a.close()
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "sharp3_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
