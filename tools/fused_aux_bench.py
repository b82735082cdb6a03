#!/usr/bin/env python
"""
ms per step of the dimension-split 2-D step in its two forms, for problems that stage aux planes in the one-kernel form
(classic_fused.hpp): 4096^2 vc_acoustics_2d (a smooth pulse in a layered medium) and 4096^2 euler_5wave_2d with a
capacity function.  PCL_TUNE_FUSED_STEP is read once per process, so every (problem, form) pair runs in a fresh child
process: warm-up steps, then the median over repeated timed windows (device-synchronised wall time).

    python tools/fused_aux_bench.py [--n 4096] [--warmup 30] [--windows 7] [--steps 40] [--lib PATH]

--lib runs the same measurement against another build of the library (PCL_LIB_OVERRIDE), e.g. the parent commit's, whose
aux / capa solvers run two passes in either mode: the yardstick.  One JSON line per run, a table at the end.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(name, n):
    g = 2
    shape = (n + 2 * g, n + 2 * g)
    x = (np.arange(shape[0]) - g + 0.5) / n
    X, Y = np.meshgrid(x, x, indexing="ij")
    if name == "vc_acoustics":
        layer = (np.floor(X * 8).astype(int) % 2).astype(float)
        aux = np.asfortranarray(np.stack([1.0 + 3.0 * layer, 1.0 + layer]))          # Z, c
        q = np.zeros((3,) + shape, order="F")
        q[0] = np.exp(-200.0 * ((X - 0.5) ** 2 + (Y - 0.5) ** 2))                     # pressure pulse, spread over the grid
        q[0] += 0.05 * np.sin(2 * np.pi * 6 * X) * np.cos(2 * np.pi * 5 * Y)
        return dict(rp=14, meqn=3, mwaves=2, par=[0.0], q=q, aux=aux, mcapa=0, mthlim=[4, 4], smax=2.0)
    rng = np.random.default_rng(0)
    q = np.empty((5,) + shape, order="F")
    q[0] = 1.0 + 0.2 * np.sin(2 * np.pi * 3 * X) * np.sin(2 * np.pi * 2 * Y)
    q[1] = 0.1 * np.cos(2 * np.pi * 2 * X)
    q[2] = 0.05 * np.sin(2 * np.pi * 4 * Y)
    q[3] = 2.5 + 0.3 * np.cos(2 * np.pi * X * Y)
    q[4] = 0.5 + 0.5 * np.sin(2 * np.pi * 5 * X)
    aux = np.asfortranarray(0.75 + 0.5 * rng.random((1,) + shape))
    return dict(rp=11, meqn=5, mwaves=5, par=[1.4, 0.4], q=q, aux=aux, mcapa=1, mthlim=[4, 4, 4, 4, 2], smax=2.5)


def child(a):
    from pyclaw_amd import _lib as L
    lib = L.lib()
    p = problem(a.problem, a.n)
    cfg = L.Config()
    cfg.ndim = 2
    cfg.n[0], cfg.n[1] = a.n, a.n
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.rp, cfg.maux = 2, p["meqn"], p["mwaves"], p["rp"], p["aux"].shape[0]
    for k, m in enumerate([1, 2, -1, 0, 0, p["mcapa"], p["aux"].shape[0]]):
        cfg.method[k] = m
    for k, m in enumerate(p["mthlim"]):
        cfg.mthlim[k] = m
    for k, v in enumerate(p["par"]):
        cfg.rp_params[k] = v
    cfg.d[0] = cfg.d[1] = 1.0 / a.n
    h = C.c_void_p()
    L.check(lib.pcl_create(C.byref(cfg), C.byref(h)))
    L.check(lib.pcl_put_aux(h, L.d(p["aux"])))
    L.check(lib.pcl_put_q(h, L.d(p["q"]), 1))
    bc = np.full(4, 2, dtype=np.int32)                   # periodic
    cst = np.zeros(32)
    dt = 0.4 / a.n / p["smax"] / (1.0 / 0.75 if p["mcapa"] else 1.0)
    cfl = C.c_double()

    def steps(k):
        for _ in range(k):
            L.check(lib.pcl_bc_step(h, L.i(bc), L.d(cst), dt, C.cast(C.byref(cfl), L.dp)))
    steps(a.warmup)
    L.check(lib.pcl_sync(h))
    ms = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        steps(a.steps)
        L.check(lib.pcl_sync(h))
        ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    t, nl = np.zeros(3), np.zeros(3, dtype=np.int64)
    s1, s0 = C.c_long(0), C.c_long(0)
    L.check(lib.pcl_step_form_stats(h, L.d(t), nl.ctypes.data_as(C.POINTER(C.c_long)), C.byref(s1), C.byref(s0)))
    lib.pcl_destroy(h)
    print(json.dumps({"problem": a.problem, "n": a.n, "mode": int(os.environ.get("PCL_TUNE_FUSED_STEP", "2")),
                      "lib": os.environ.get("PCL_LIB_OVERRIDE", "this build"), "ms_per_step_median": float(np.median(ms)),
                      "ms_per_step_windows": [round(v, 4) for v in ms], "steps_one_kernel": int(s1.value),
                      "steps_two_pass": int(s0.value), "cfl": cfl.value}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lib", default=None, help="another build of libpyclaw_amd.so to measure instead (the yardstick)")
    ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--problem", default=None, help="(internal) run one measurement in this process")
    a = ap.parse_args()
    if a.problem:
        return child(a)
    rows = []
    for prob in ("vc_acoustics", "euler_capa"):
        for mode in a.modes:
            env = dict(os.environ)
            env["PCL_TUNE_FUSED_STEP"] = str(mode)
            if a.lib:
                env["PCL_LIB_OVERRIDE"] = os.path.abspath(a.lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--problem", prob, "--n", str(a.n), "--warmup",
                                  str(a.warmup), "--windows", str(a.windows), "--steps", str(a.steps)], env=env,
                                 stdout=subprocess.PIPE, text=True, timeout=900)
            if out.returncode != 0:
                raise SystemExit("child failed: %s mode %d" % (prob, mode))
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    for r in rows:
        print("%-13s mode %d  %.4f ms/step  (one-kernel steps %d, two-pass steps %d)" %
              (r["problem"], r["mode"], r["ms_per_step_median"], r["steps_one_kernel"], r["steps_two_pass"]))


if __name__ == "__main__":
    main()
