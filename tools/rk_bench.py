#!/usr/bin/env python
"""
What a Runge-Kutta scheme given by its Butcher tableau costs on the resident 4096^2 acoustics state of
`tools/cellrp_bench.py --sharpclaw` (2-D acoustics, WENO5, three components), in one job with the arms taking turns:

  steps     ms per step of SSP104 (ten fused stages, the hand-written path), RK44 (four stages) and DP5 (six stages): three
            solvers set up side by side in this process, timed in alternating segments of `--steps` steps by device events;
  lincomb   ms per launch of the combination kernel (sharpclaw.hpp: rk_lincomb_kernel, pcl_rk_lincomb) with n = 1, 4 and 6
            terms, D = S1, A = Q: n + 1 arrays in, one out, `--launches` launches per segment by device events;
  copy      the rate of tools/ubench/copy_rates' grid-stride double x2 copy kernel (2048 workgroups, the same launch shape)
            moving the same number of bytes as each of those launches: a child process per segment, between the segments of
            the kernel.

The yardstick of the kernel is that copy rate; the yardstick of a step is SSP104's cost per stage.  Writes one JSON line
(`--out`, default profiles/rk_bench.json).  Needs a GPU.

`--resource-usage` needs none: it compiles kernels.hip for the device with the exact mode's flags and writes the compiler's
register / LDS / occupancy report of every rk_lincomb_kernel instantiation (default profiles/rk_resource_usage.txt).

  python tools/rk_bench.py [--n 4096] [--steps 5] [--warmup 2] [--reps 5] [--launches 20] [--out FILE]
  python tools/rk_bench.py --resource-usage [--out FILE]
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COPY_SRC = os.path.join(ROOT, "tools", "ubench", "copy_rates.hip")
COPY_BIN = os.path.join(ROOT, "tools", "ubench", "copy_rates")
SCHEMES = ("SSP104", "RK44", "DP5")
STAGES = {"SSP104": 10, "RK44": 4, "DP5": 6}
TERMS = (1, 4, 6)


def spread(vals):
    return {"median": float(np.median(vals)), "min": min(vals), "max": max(vals), "all": vals}


def resource_usage(out):
    csrc = os.path.join(ROOT, "pyclaw_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I/opt/rocm/include", "-ffp-contract=off",
           "-DPCL_NS=exact", "-DPCL_FAST=0", "-DPCL_DENORM_GUARD=0", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", "kernels.hip", "-o", os.devnull]
    p = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise SystemExit("rk_bench: the compile failed:\n" + p.stdout[-2000:])
    # the report of one kernel: a "Function Name:" remark followed by its figures, up to the next one
    blocks, keep = [], False
    for line in p.stdout.splitlines():
        m = re.search(r"remark: (.*)$", line)
        if not m:
            continue
        text = m.group(1).replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
        if text.startswith("Function Name:"):
            keep = "rk_lincomb_kernel" in text
            if keep:
                blocks.append([])
        if keep:
            blocks[-1].append(text)
    if not blocks:
        raise SystemExit("rk_bench: no rk_lincomb_kernel in the compiler's report")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("# hipcc -Rpass-analysis=kernel-resource-usage, gfx950, exact mode: rk_lincomb_kernel<N>, N = number of terms\n")
        for b in blocks:
            f.write("\n".join(b) + "\n\n")
    print("rk_bench: %d instantiations -> %s" % (len(blocks), out))


def ensure_copy_binary():
    if not os.path.exists(COPY_BIN) or os.path.getmtime(COPY_BIN) < os.path.getmtime(COPY_SRC):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-o", COPY_BIN, COPY_SRC])


def copy_ms(doubles, launches):
    """the x2 copy kernel over `doubles` doubles (read and written once each), ms per launch"""
    out = subprocess.run([COPY_BIN, str(int(doubles)), str(launches)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=120)
    m = re.search(r"^COPY \d+ doubles\s+([0-9.]+) ms", out.stdout, flags=re.M)
    if out.returncode != 0 or not m:
        raise SystemExit("rk_bench: copy_rates failed (exit %d):\n%s" % (out.returncode, out.stdout[-1000:]))
    return float(m.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--math", default="exact")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resource-usage", dest="resource_usage", action="store_true")
    args = ap.parse_args()
    if args.resource_usage:
        return resource_usage(args.out or os.path.join(ROOT, "profiles", "rk_resource_usage.txt"))

    import pyclaw_amd as pyclaw
    from pyclaw_amd import _lib
    from apps import problems
    L = _lib.lib()
    if L.pcl_device_count() < 1:
        raise SystemExit("rk_bench: no HIP device (nothing here can be measured without one)")
    ensure_copy_binary()
    ms = ctypes.c_float()

    claws = {}
    for ti in SCHEMES:
        claw = problems.acoustics2D(pyclaw, mx=args.n, my=args.n, run=False, math=args.math, solver_type='sharpclaw',
                                    time_integrator=ti)
        claw.solver.setup(claw.solution)
        claw.solver.dt_variable = False
        claw.solver.dt = claw.solver.dt_initial       # the app's own first step: a Courant number of 0.45
        claw.solver.begin_resident(claw.solution)
        claws[ti] = claw
    rejected = 0
    for ti in SCHEMES:
        for _ in range(args.warmup):
            rejected += claws[ti].solver.step(claws[ti].solution) is False
    seg = {ti: [] for ti in SCHEMES}
    for r in range(args.reps):
        for ti in SCHEMES:
            solver, solution = claws[ti].solver, claws[ti].solution
            _lib.check(L.pcl_sync(solver._h))
            _lib.check(L.pcl_timer_start(solver._h))
            for _ in range(args.steps):
                rejected += solver.step(solution) is False
            _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
            seg[ti].append(ms.value / args.steps)
        print("round %d: " % (r + 1) + ", ".join("%s %.3f ms" % (ti, seg[ti][-1]) for ti in SCHEMES), file=sys.stderr, flush=True)
    steps = {}
    for ti in SCHEMES:
        s = spread(seg[ti])
        steps[ti] = {"ms_per_step": s, "stages": STAGES[ti], "ms_per_stage": s["median"] / STAGES[ti],
                     "cfl": claws[ti].solver.cfl.get_cached_max()}
    for ti in ("SSP104", "RK44"):
        claws[ti].solver.end_resident(claws[ti].solution)
        claws[ti].solver.teardown()

    # the combination kernel on DP5's handle (six stage registers): S1 = Q + sum of n terms
    solver = claws["DP5"].solver
    st = claws["DP5"].solution.state
    pitch = (args.n + 2 * solver.mbc + 15) // 16 * 16
    total = pitch * (args.n + 2 * solver.mbc) * st.meqn        # doubles per register, as pcl_create lays them out
    coef = np.array([0.5, 0.25, -0.125, 1.0, 0.75, -0.5])
    stages = np.arange(6, dtype=np.int32)
    lin = {n: [] for n in TERMS}
    cop = {n: [] for n in TERMS}

    def fire(n, count):
        for _ in range(count):
            _lib.check(L.pcl_rk_lincomb(solver._h, 1, 0, n, _lib.i(stages), _lib.d(coef)))
    for n in TERMS:
        fire(n, 3)
    for r in range(args.reps):
        for n in TERMS:
            _lib.check(L.pcl_sync(solver._h))
            _lib.check(L.pcl_timer_start(solver._h))
            fire(n, args.launches)
            _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
            lin[n].append(ms.value / args.launches)
            _lib.check(L.pcl_sync(solver._h))
            # the same bytes: n + 2 arrays of `total` doubles move, the copy moves two per double copied
            cop[n].append(copy_ms((n + 2) * total // 2, args.launches))
        print("round %d: " % (r + 1) + ", ".join("n=%d %.3f ms (copy %.3f ms)" % (n, lin[n][-1], cop[n][-1]) for n in TERMS),
              file=sys.stderr, flush=True)
    solver.end_resident(claws["DP5"].solution)
    solver.teardown()
    kernel = {}
    for n in TERMS:
        nbytes = (n + 2) * total * 8
        a, b = spread(lin[n]), spread(cop[n])
        kernel["n=%d" % n] = {"bytes": nbytes, "lincomb_ms": a, "copy_ms": b, "lincomb_GBps": nbytes / a["median"] / 1e6,
                              "copy_GBps": nbytes / b["median"] / 1e6, "lincomb_over_copy": a["median"] / b["median"],
                              "spreads_overlap": not (a["min"] > b["max"] or b["min"] > a["max"])}
    res = {"tool": "rk_bench", "n": args.n, "grid": [args.n, args.n], "math": args.math, "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "launches": args.launches, "register_doubles": total, "rejected_steps": int(rejected),
           "what": "ms per step (segments of the three schemes alternating in one process); ms per pcl_rk_lincomb launch "
                   "against copy_rates' x2 copy kernel over the same bytes, alternating",
           "steps_ms": steps, "kernel": kernel}
    line = json.dumps(res)
    print(line)
    out = args.out or os.path.join(ROOT, "profiles", "rk_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
