#!/usr/bin/env python
"""
What a user-written Riemann solver costs per step on the resident 4096^2 acoustics problem, three ways:

  (a) two_pass  the built-in acoustics_2d solver held to the two-pass form of the step (PCL_TUNE_FUSED_STEP=0)
  (b) user      the same solver as a pyclaw.CellRiemann (problems.ACOUSTICS_2D_RP): always two passes
  (c) default   the built-in solver on its default path (the one-kernel step with its quiet tiles)

(a) and (b) run the same kernel template over the same tiles; (b) against (c) is the price of not having the one-kernel
step.  PCL_TUNE_FUSED_STEP is read once per process, so every measurement is a child process of its own: `--reps` rounds
of a, b, c in turn.  A child sets the problem up, takes `--warmup` steps and times `--steps` calls of step_hyperbolic at
a fixed dt with device events, on two states: "pulse", the app's initial condition (most of the box is at rest), and
"dense", the same with noise on every component of every cell.  Prints one JSON line with median (min - max) ms per
step, and the hiprtc compile time of the user solver as the children saw it (one progress line per child goes to
stderr); needs a GPU.

--aux measures the same three ways on the problem with cell-wise coefficients instead: vc_acoustics_2d in a layered
medium (problems.vc_acoustics2D) against its restatement as a CellRiemann that reads aux=(0, 1)
(problems.VC_ACOUSTICS_2D_RP).  The sweeps then stage two aux planes next to q.

--unsplit measures the unsplit step (dim_split = False, order_trans = 2) two ways instead: "builtin", the built-in
solver, and "user", the same solver as a CellRiemann with a transverse body (problems.ACOUSTICS_2D_RPT, or with --aux
problems.VC_ACOUSTICS_2D_RPT).  Both run unsplit_x_kernel; in the y phase the user solver always takes the tile kernel,
the built-in solver without aux the marching kernel once the grid is large enough for it (kernels.hip: 4096^2, not
2048^2), so at 2048^2 the two runs execute the same templates and at 4096^2 their difference is the price of that limit.
The children also time the run-time compile of the solver with and without its transverse text.

--fwave measures the three ways of the first paragraph on the p-system (apps/psystem.py: psystem2D, dimension-split):
the built-in f-wave solver psystem_fwave_2d held to two passes, the same solver as a CellRiemann compiled with
fwave=True (PSYSTEM_FWAVE_2D_RP, aux=(0, 1, 2, 3)), and the built-in solver on its default path.

--capa measures acoustics on a grid with a capacity function (problems.capa_acoustics2D) two ways: "two_pass", the
built-in solver held to two passes, and "user", ACOUSTICS_2D_RP in a CellRiemann compiled with capa=True.

--sharpclaw measures the SharpClaw stages two ways: ms per SSP104 step (ten fused stages, WENO5) of 2-D acoustics with
"builtin", rp_acoustics_2d, and "user", ACOUSTICS_2D_RP in a CellRiemann compiled with sharpclaw=True.  Both run
sharp_kernel over the same tiles.  The children also time every distinct run-time compile they make: the user solver's
SharpClaw kernels ("compile_s") and, for comparison, the same body's classic sweeps ("compile_classic_s").

--one-kernel measures what CellRiemann(..., one_kernel=True) buys, three ways: "default", the built-in solver on its
default path (the one-kernel step with its quiet tiles: the yardstick), "user_onek", the same solver as a CellRiemann
compiled with one_kernel=True (the same one-kernel step around the body, chosen as for the built-in solver), and "user",
the CellRiemann without it (always two passes).  With --aux the same on vc_acoustics_2d against CellRiemann(aux=(0, 1)).
"compile_s" is the cold run-time compile with the one-kernel step, "compile_plain_s" the one without, each as its
children saw it.

--ndim 3 measures the dimension-split 3-D step two ways on the workload of `bench.py --ndim 3` (its build3d: 3-D acoustics
in two materials, n^3 cells, n = 512 unless --n says otherwise): "builtin", rp_vc_acoustics_3d, and "user", the same solver
as a CellRiemann3D (problems.VC_ACOUSTICS_3D_RP, aux=(0, 1)).  Both run sweep3_kernel over the same tiles, and nothing
here is read once per process, so the two solvers live side by side in this process and are timed in alternating
segments of `--steps` steps, `--reps` of each per state.

--ndim 3 --unsplit measures the unsplit 3-D step (step3, order_trans 22) on the grid of `bench.py --ndim 3 --unsplit` (its
build3d(unsplit=True), n = 256 unless --n says otherwise): "builtin", rp_vc_acoustics_3d in march3p_kernel, against "user",
the same solver as the three texts VC_ACOUSTICS_3D_RP / _RPT / _RPTT of a CellRiemann3D in the general form (pieces3_kernel
+ gather3_kernel through scratch planes), alternating as above; then, unless --euler-n 0, the Euler equations through
EULER_3D_RP / _RPT / _RPTT unsplit ("user") against the same bodies dimension-split ("builtin" in the output's terms:
the yardstick) on an --euler-n cube.  The output also holds the scratch bytes and the cold compile times of the
three-text handles.

  python tools/cellrp_bench.py [--aux] [--unsplit | --one-kernel] [--fwave | --capa | --sharpclaw | --ndim 3 [--unsplit]] [--n 4096] [--steps 20] [--warmup 3] [--reps 7] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ("two_pass", "user", "default")
VARIANTS_UNSPLIT = ("builtin", "user")
VARIANTS_CAPA = ("two_pass", "user")
VARIANTS_ONEK = ("default", "user_onek", "user")


def child(args):
    import pyclaw_amd as pyclaw
    from pyclaw_amd import _lib
    from apps import problems
    L = _lib.lib()
    if L.pcl_device_count() < 1:
        raise SystemExit("cellrp_bench: no HIP device (nothing here can be measured without one)")
    user = args.child in ("user", "user_onek")
    if args.sharpclaw:
        claw = problems.acoustics2D(pyclaw, mx=args.n, my=args.n, run=False, math=args.math, solver_type='sharpclaw',
                                    time_integrator='SSP104', user_rp=user)
    elif args.fwave:
        from apps import psystem
        claw = psystem.psystem2D(pyclaw, mx=args.n, my=args.n, solver_type='classic', run=False, math=args.math,
                                 user_rp=user)
    elif args.capa:
        claw = problems.capa_acoustics2D(pyclaw, mx=args.n, my=args.n, run=False, math=args.math, user_rp=user)
    elif args.unsplit:
        make = problems.vc_acoustics2D if args.aux else problems.acoustics2D
        claw = make(pyclaw, mx=args.n, my=args.n, run=False, math=args.math, dim_split=0, user_rp=user)
        claw.solver.order_trans = 2
    elif args.aux:
        claw = problems.vc_acoustics2D(pyclaw, mx=args.n, my=args.n, run=False, math=args.math, user_rp=user)
    else:
        claw = problems.acoustics2D(pyclaw, mx=args.n, my=args.n, run=False, math=args.math)
    solver, solution = claw.solver, claw.solution
    state = solution.state
    res = {"variant": args.child}
    if args.child == "user" and args.sharpclaw:
        rp = solver.rp
        sharp = (solver.lim_type, solver.weno_order, solver.char_decomp)
        t0 = time.perf_counter()
        rp.compile(args.math, sharp=sharp)
        res["compile_s"] = time.perf_counter() - t0
        classic = pyclaw.CellRiemann(rp.body, rp.meqn, rp.mwaves, 2)       # the same body's classic sweeps
        t0 = time.perf_counter()
        classic.compile(args.math)
        res["compile_classic_s"] = time.perf_counter() - t0
    elif user:
        if args.unsplit:        # the same normal body without the transverse text, for the compile time alone
            rp = solver.rp
            plain = pyclaw.CellRiemann(rp.body, rp.meqn, rp.mwaves, 2, aux=rp.aux)
            t0 = time.perf_counter()
            plain.compile(args.math)
            res["compile_plain_s"] = time.perf_counter() - t0
        elif not args.aux and not args.fwave and not args.capa:
            g = state.aux_global
            solver.rp = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2, params=[g['rho'], g['bulk'], g['cc'], g['zz']])
        solver.rp.one_kernel = args.child == "user_onek"
        t0 = time.perf_counter()
        solver.rp.compile(args.math)
        res["compile_s"] = time.perf_counter() - t0
    solver.setup(solution)
    solver.dt_variable = False
    # one step: the classic hyperbolic step, or the SSP104 step of its ten stages
    one_step = solver.step if args.sharpclaw else solver.step_hyperbolic
    if args.fwave or args.capa or args.sharpclaw:
        solver.dt = solver.dt_initial       # the app's own first step: within its cfl_desired on either state
    else:
        solver.dt = 0.45 * min(state.grid.d) / (float(state.aux[1].max()) if args.aux else state.aux_global['cc'])
    q_pulse = state.q.copy('F')
    rng = np.random.default_rng(7)
    q_dense = q_pulse + 0.01 * rng.standard_normal(q_pulse.shape)
    ms = ctypes.c_float()
    for name, q0 in (("pulse", q_pulse), ("dense", q_dense)):
        state.q[...] = q0
        solver.begin_resident(solution)
        for _ in range(args.warmup):
            one_step(solution)
        _lib.check(L.pcl_sync(solver._h))
        _lib.check(L.pcl_timer_start(solver._h))
        for _ in range(args.steps):
            one_step(solution)
        _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
        res[name + "_ms"] = ms.value / args.steps
        res[name + "_cfl"] = solver.cfl.get_cached_max()
        solver.end_resident(solution)
        res[name + "_sum"] = float(np.abs(state.q).sum())         # the variants compute the same thing
    solver.teardown()
    res["forms"] = solver.status.get("step_forms")
    print("CELLRP_CHILD " + json.dumps(res))


def run3(args):
    """--ndim 3: both solvers in this process, timed in alternating segments"""
    import pyclaw_amd as pyclaw
    from pyclaw_amd import _lib
    from apps import problems
    import bench
    L = _lib.lib()
    if L.pcl_device_count() < 1:
        raise SystemExit("cellrp_bench: no HIP device (nothing here can be measured without one)")
    n = (256 if args.unsplit else 512) if args.n == 4096 else args.n
    variants = VARIANTS_UNSPLIT

    def cold_compile(rp):
        """the run-time compile of rp's texts with nothing cached: a comment that no earlier run can have made"""
        twin = pyclaw.CellRiemann3D(rp.body + "// cold compile %r\n" % time.time(), rp.meqn, rp.mwaves, aux=rp.aux, rpt3=rp.rpt3,
                                    rptt3=rp.rptt3)
        t0 = time.perf_counter()
        twin.compile(args.math)
        return time.perf_counter() - t0

    def vc_pair():
        claws, compile_s = {}, None
        for v in variants:
            claw = bench.build3d(n, args.math, args.unsplit)
            if v == "user":
                trans = dict(rpt3=problems.VC_ACOUSTICS_3D_RPT, rptt3=problems.VC_ACOUSTICS_3D_RPTT) if args.unsplit else {}
                claw.solver.rp = pyclaw.CellRiemann3D(problems.VC_ACOUSTICS_3D_RP, 4, 2, aux=(0, 1), name="vc_acoustics_3d_user", **trans)
                t0 = time.perf_counter()
                claw.solver.rp.compile(args.math)
                compile_s = time.perf_counter() - t0
            claw.solver.setup(claw.solution)
            claw.solver.dt_variable = False
            claw.solver.dt = claw.solver.dt_initial         # bench.py's: a Courant number of 0.4 in the faster material
            claws[v] = claw
        return claws, compile_s

    def euler_pair(m):
        """the Euler bodies dimension-split ("builtin": the yardstick) and unsplit ("user") on an m^3 box of smooth data"""
        claws, compile_s = {}, None
        for v in variants:
            claw = problems.euler3D(pyclaw, n=m, across=(m, m), run=False, math=args.math, dim_split=v == "builtin")
            st = claw.solution.state
            X, Y, Z = st.grid.c_center
            rho = 1.0 + 0.2 * np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y) * np.cos(2 * np.pi * Z)
            vel = (0.3, -0.2, 0.25)
            st.q[0] = rho
            for k in range(3):
                st.q[1 + k] = rho * vel[k]
            st.q[4] = 1.0 / 0.4 + 0.5 * rho * sum(c * c for c in vel)
            if v == "user":
                t0 = time.perf_counter()
                claw.solver.rp.compile(args.math)
                compile_s = time.perf_counter() - t0
            claw.solver.setup(claw.solution)
            claw.solver.dt_variable = False
            claw.solver.dt = 0.4 * (1.0 / m) / 2.0          # sound speed about 1.2, |velocity| below 0.5
            claws[v] = claw
        return claws, compile_s
    if args.unsplit:
        res = {"tool": "cellrp_bench --ndim 3 --unsplit", "math": args.math, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
               "what": "ms per unsplit 3-D step (order_trans 22), segments of the two variants alternating in one process"}
        claws, compile_s = vc_pair()
        cold_vc = cold_compile(claws["user"].solver.rp)
        res["vc_acoustics"] = dict(alternate3(args, claws, variants), n=n, grid=[n, n, n], compile_s=compile_s,
                                   builtin="rp_vc_acoustics_3d, march3p_kernel", user="VC_ACOUSTICS_3D_RP / _RPT / _RPTT, pieces3_kernel + gather3_kernel",
                                   scratch_bytes=int(L.pcl_unsplit3_scratch_bytes(4, n, n, n, 2)), cold_compile_s=cold_vc)
        if args.euler_n > 0:
            m = args.euler_n
            claws, compile_s = euler_pair(m)
            cold_eu = cold_compile(claws["user"].solver.rp)
            res["euler"] = dict(alternate3(args, claws, variants, same=False), n=m, grid=[m, m, m], compile_s=compile_s,
                                builtin="EULER_3D_RP dimension-split (sweep3_kernel x 3)", user="EULER_3D_RP / _RPT / _RPTT unsplit",
                                scratch_bytes=int(L.pcl_unsplit3_scratch_bytes(5, m, m, m, 2)), cold_compile_s=cold_eu)
        return emit(args, res)
    claws, compile_s = vc_pair()
    res = {"tool": "cellrp_bench --ndim 3", "n": n, "grid": [n, n, n], "math": args.math, "steps": args.steps, "warmup": args.warmup,
           "reps": args.reps, "what": "ms per dimension-split 3-D step (x, y, z sweeps), segments of the two solvers alternating in one process",
           "compile_s": compile_s}
    res.update(alternate3(args, claws, variants))
    emit(args, res)


def emit(args, res):
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def alternate3(args, claws, variants, same=True):
    """warm both set-up solvers up on each state and time them in alternating segments; tears them down.  same: the two
    compute the same thing (then the output says whether they did)"""
    from pyclaw_amd import _lib
    L = _lib.lib()
    q_pulse = claws["builtin"].solution.state.q.copy('F')
    rng = np.random.default_rng(7)
    noise = 0.01 * rng.standard_normal(q_pulse.shape[1:])     # one plane's worth, on every component
    ms = ctypes.c_float()
    res = {"states": {}}

    def spread(vals):
        return {"median": float(np.median(vals)), "min": min(vals), "max": max(vals), "all": vals}
    for name in ("pulse", "dense"):
        for v in variants:
            st = claws[v].solution.state
            st.q[...] = q_pulse
            if name == "dense":
                st.q[...] += noise
            claws[v].solver.begin_resident(claws[v].solution)
            for _ in range(args.warmup):
                claws[v].solver.step_hyperbolic(claws[v].solution)
        seg = {v: [] for v in variants}
        for r in range(args.reps):
            for v in variants:
                solver, solution = claws[v].solver, claws[v].solution
                _lib.check(L.pcl_sync(solver._h))
                _lib.check(L.pcl_timer_start(solver._h))
                for _ in range(args.steps):
                    solver.step_hyperbolic(solution)
                _lib.check(L.pcl_timer_stop(solver._h, ctypes.byref(ms)))
                seg[v].append(ms.value / args.steps)
            print("round %d %s: builtin %.4f ms, user %.4f ms" % (r + 1, name, seg["builtin"][-1], seg["user"][-1]),
                  file=sys.stderr, flush=True)
        sums, cfls = set(), set()
        for v in variants:
            claws[v].solver.end_resident(claws[v].solution)
            sums.add(float(np.abs(claws[v].solution.state.q).sum()))       # the two compute the same thing
            cfls.add(claws[v].solver.cfl.get_cached_max())
        a, b = spread(seg["builtin"]), spread(seg["user"])
        res["states"][name] = {"builtin_ms": a, "user_ms": b,
                               "same_result_in_every_run": (len(sums) == 1 and len(cfls) == 1) if same else None,
                               "user_over_builtin": b["median"] / a["median"],
                               "user_and_builtin_spreads_overlap": not (b["min"] > a["max"] or a["min"] > b["max"])}
    for v in variants:
        claws[v].solver.teardown()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--math", default="exact")
    ap.add_argument("--out", default=None)
    ap.add_argument("--aux", action="store_true", help="the variable-coefficient problem: vc_acoustics_2d against CellRiemann(aux=(0, 1))")
    ap.add_argument("--unsplit", action="store_true", help="the unsplit step: the built-in solver against CellRiemann(transverse=...)")
    ap.add_argument("--fwave", action="store_true", help="the p-system: psystem_fwave_2d against CellRiemann(fwave=True)")
    ap.add_argument("--capa", action="store_true", help="acoustics with a capacity function: the built-in two passes against CellRiemann(capa=True)")
    ap.add_argument("--sharpclaw", action="store_true", help="the SSP104 step of SharpClaw: rp_acoustics_2d against CellRiemann(sharpclaw=True)")
    ap.add_argument("--ndim", type=int, default=2, choices=[2, 3],
                    help="3: the dimension-split 3-D step on bench.py's 3-D grid, rp_vc_acoustics_3d against CellRiemann3D")
    ap.add_argument("--one-kernel", dest="one_kernel", action="store_true",
                    help="CellRiemann(one_kernel=True) against the built-in one-kernel step and against the user solver's two passes")
    ap.add_argument("--euler-n", dest="euler_n", type=int, default=256,
                    help="--ndim 3 --unsplit: the cube of the Euler measurement (0: leave it out)")
    ap.add_argument("--child", default=None, choices=VARIANTS + VARIANTS_UNSPLIT + VARIANTS_ONEK[1:2])
    args = ap.parse_args()
    if args.ndim == 3:
        if args.aux or args.fwave or args.capa or args.sharpclaw or args.one_kernel:
            raise SystemExit("cellrp_bench: --ndim 3 is a measurement of its own")
        return run3(args)
    if (args.fwave or args.capa) and (args.aux or args.unsplit or (args.fwave and args.capa)):
        raise SystemExit("cellrp_bench: --fwave and --capa are measurements of their own (not with --aux, --unsplit or each other)")
    if args.sharpclaw and (args.aux or args.unsplit or args.fwave or args.capa):
        raise SystemExit("cellrp_bench: --sharpclaw is a measurement of its own")
    if args.one_kernel and (args.unsplit or args.fwave or args.capa or args.sharpclaw):
        raise SystemExit("cellrp_bench: --one-kernel goes with --aux or alone")
    if args.child:
        return child(args)

    # (--sharpclaw: two variants compared like the unsplit pair)
    variants = (VARIANTS_ONEK if args.one_kernel else VARIANTS_UNSPLIT if args.unsplit or args.sharpclaw
                else VARIANTS_CAPA if args.capa else VARIANTS)
    mode = (["--aux"] if args.aux else []) + (["--unsplit"] if args.unsplit else []) + (["--fwave"] if args.fwave else []) + \
           (["--capa"] if args.capa else []) + (["--sharpclaw"] if args.sharpclaw else [])
    # (the children of --one-kernel differ in their variant alone: nothing of the mode reaches them but --aux)
    label = mode + (["--one-kernel"] if args.one_kernel else [])
    runs = {v: [] for v in variants}
    for _ in range(args.reps):
        for v in variants:
            env = dict(os.environ)
            env.pop("PCL_TUNE_FUSED_STEP", None)
            if v == "two_pass":
                env["PCL_TUNE_FUSED_STEP"] = "0"
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--n", str(args.n), "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--math", args.math] + mode
            out = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            lines = [l for l in out.stdout.splitlines() if l.startswith("CELLRP_CHILD ")]
            if out.returncode != 0 or not lines:
                raise SystemExit("cellrp_bench: the %s run failed (exit %d):\n%s" % (v, out.returncode, out.stdout[-2000:]))
            runs[v].append(json.loads(lines[-1][len("CELLRP_CHILD "):]))
            print("round %d %s: pulse %.4f ms, dense %.4f ms" % (len(runs[v]), v, runs[v][-1]["pulse_ms"], runs[v][-1]["dense_ms"]),
                  file=sys.stderr, flush=True)

    def spread(vals):
        return {"median": float(np.median(vals)), "min": min(vals), "max": max(vals), "all": vals}
    res = {"tool": " ".join(["cellrp_bench"] + label), "n": args.n, "math": args.math, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "compile_s": spread([r["compile_s"] for r in runs["user_onek" if args.one_kernel else "user"]]), "forms": {v: runs[v][-1]["forms"] for v in variants},
           "states": {}}
    if args.one_kernel:
        res["compile_plain_s"] = spread([r["compile_s"] for r in runs["user"]])
        res["what"] = "ms per dimension-split step; default = the built-in solver's one-kernel path, user_onek = CellRiemann(one_kernel=True), user = its two passes"
    if args.unsplit:
        res["compile_plain_s"] = spread([r["compile_plain_s"] for r in runs["user"]])
    if args.sharpclaw:
        res["compile_classic_s"] = spread([r["compile_classic_s"] for r in runs["user"]])
        res["what"] = "ms per SSP104 step (ten fused stages, WENO5, lim_type 2)"
    for name in ("pulse", "dense"):
        st = {v + "_ms": spread([r[name + "_ms"] for r in runs[v]]) for v in variants}
        sums = set(r[name + "_sum"] for v in variants for r in runs[v])
        cfls = set(r[name + "_cfl"] for v in variants for r in runs[v])
        st["same_result_in_every_run"] = len(sums) == 1 and len(cfls) == 1
        if args.one_kernel:
            a, b, c = (st[v + "_ms"] for v in variants)
            st["user_onek_over_default"] = b["median"] / a["median"]
            st["user_onek_and_default_spreads_overlap"] = not (b["min"] > a["max"] or a["min"] > b["max"])
            st["user_over_user_onek"] = c["median"] / b["median"]
            st["user_onek_and_user_spreads_overlap"] = not (b["min"] > c["max"] or c["min"] > b["max"])
            res["states"][name] = st
            continue
        if args.unsplit or args.sharpclaw:
            a, b = (st[v + "_ms"] for v in variants)
            st["user_over_builtin"] = b["median"] / a["median"]
            st["user_and_builtin_spreads_overlap"] = not (b["min"] > a["max"] or a["min"] > b["max"])
            res["states"][name] = st
            continue
        a, b = st["two_pass_ms"], st["user_ms"]
        st["user_over_two_pass"] = b["median"] / a["median"]
        st["user_and_two_pass_spreads_overlap"] = not (b["min"] > a["max"] or a["min"] > b["max"])
        if "default" in variants:
            st["user_over_default"] = b["median"] / st["default_ms"]["median"]
        res["states"][name] = st
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
