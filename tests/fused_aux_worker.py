"""
Worker of tests/test_gpu_fused_aux.py: dimension-split 2-D problems whose Riemann solver reads aux arrays
(vc_acoustics_2d, vc_advection_2d, psystem_fwave_2d) or whose state has a capacity function, stepped through
pcl_bc_step on one GPU.  The switch PCL_TUNE_FUSED_STEP is read once per process, so the caller starts one worker per
mode (1: both sweeps in one kernel, classic_fused.hpp; 0: x pass + y pass, classic.hpp; 2: timed trials choose) and
compares the lines: one JSON line with, per case, a hash of the final state, the Courant number of every step and
[steps in the one-kernel form, steps in the two-pass form] (pcl_step_form_stats).  With a file name as argument the
final states go into that .npz as well (the caller holds them against the C oracle).

The case definitions (cases()) need no GPU: the test module imports them to run the oracle on the same inputs.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MBC = 2
RP_ACOUSTICS, RP_EULER5, RP_ADVECTION, RP_SHALLOW, RP_VC_ACOUSTICS, RP_VC_ADVECTION, RP_PSYSTEM = 10, 11, 12, 13, 14, 15, 17
CST, OUT, PER, REF = 0, 1, 2, 3           # PCL_BC_CUSTOM (constant state), OUTFLOW, PERIODIC, REFLECTING


class Case(object):
    """one problem: qbc / auxbc with ghost cells (Fortran order), bc[4] = x lower, x upper, y lower, y upper"""

    def __init__(self, name, rp, meqn, mwaves, par, q, aux, mcapa, bc, dt, dx, dy, steps, order=2, mthlim=None, fwave=0,
                 cstate=None, ghosts=False):
        self.name, self.rp, self.meqn, self.mwaves, self.par = name, rp, meqn, mwaves, list(par)
        self.q, self.aux, self.mcapa, self.bc, self.dt, self.dx, self.dy = q, aux, mcapa, list(bc), dt, dx, dy
        self.steps, self.order, self.fwave = steps, order, fwave
        self.mthlim = list(mthlim) if mthlim is not None else [4] * mwaves
        self.cstate = np.zeros((4, 8)) if cstate is None else cstate
        self.ghosts = ghosts               # the ghost cells of q are part of the input: no boundary conditions (bc < 0)
        self.mx, self.my = q.shape[1] - 2 * MBC, q.shape[2] - 2 * MBC
        self.maux = aux.shape[0]

    def method(self):
        return np.array([1, self.order, -1, 0, 0, self.mcapa, self.maux], dtype=np.int32)


def shape_of(mx, my):
    return (mx + 2 * MBC, my + 2 * MBC)


def quiet_patch(q, mx, my):
    """a constant patch: wavefronts without a jump (the shortcut of lane_core) next to wavefronts with jumps"""
    if mx >= 40 and my >= 10:
        i0, i1, j0, j1 = MBC + mx // 5, MBC + (4 * mx) // 5, MBC + my // 4, MBC + (3 * my) // 4
        q[:, i0:i1, j0:j1] = q[:, i0:i0 + 1, j0:j0 + 1]
    return q


def layered(mx, my):
    """impedance and sound speed in three layers across x, a fourth along y"""
    i, j = np.meshgrid(np.arange(mx + 2 * MBC), np.arange(my + 2 * MBC), indexing="ij")
    k = (3 * i // (mx + 2 * MBC) + (j > (my + 2 * MBC) // 2)) % 4
    z = np.array([1.0, 4.0, 2.0, 0.5])[k]
    c = np.array([1.0, 2.0, 0.5, 1.5])[k]
    return np.asfortranarray(np.stack([z, c]))


def vc_acoustics(name, mx, my, medium, bc, steps=24, order=2, mthlim=(4, 4), capa=False, seed=1):
    rng = np.random.default_rng(seed)
    shape = shape_of(mx, my)
    aux = layered(mx, my) if medium == "layered" else np.asfortranarray(0.5 + 1.5 * rng.random((2,) + shape))
    mcapa = 0
    if capa:                                # aux and capa together: the capacity function as a third component
        aux = np.asfortranarray(np.concatenate([aux, 0.5 + rng.random((1,) + shape)]))
        mcapa = 3
    q = quiet_patch(np.asfortranarray(rng.standard_normal((3,) + shape)), mx, my)
    dx, dy = 2.0 / mx, 1.3 / my
    dt = 0.4 * min(dx, dy) / 2.0 * (0.5 if capa else 1.0)
    return Case(name, RP_VC_ACOUSTICS, 3, 2, [0.0], q, aux, mcapa, bc, dt, dx, dy, steps, order, mthlim)


def vc_advection(name, n, bc, steps=24):
    """the rotating-flow edge velocities of apps/problems.py::rotating_flow (stream function, periodic), no capa"""
    d = 2.0 / n
    e = -1.0 + d * (np.arange(n + 2 * MBC + 1) - MBC)           # cell edges, ghost cells included
    XE, YE = np.meshgrid(e, e, indexing="ij")
    P = 0.5 * np.pi * (np.cos(np.pi * XE / 2) ** 2) * (np.cos(np.pi * YE / 2) ** 2)
    aux = np.asfortranarray(np.stack([(P[:-1, 1:] - P[:-1, :-1]) / d, -(P[1:, :-1] - P[:-1, :-1]) / d]))
    c = 0.5 * (e[1:] + e[:-1])
    X, Y = np.meshgrid(c, c, indexing="ij")
    q = np.asfortranarray(np.exp(-40.0 * ((X - 0.3) ** 2 + Y ** 2))[None])
    return Case(name, RP_VC_ADVECTION, 1, 1, [0.0], q, aux, 0, bc, 0.4 * d / 1.6, d, d, steps, 2, [3])


def psystem(name, mx, my, bc, steps=20, seed=5):
    """p-system, f-waves, linear stress law sigma = K eps (aux(3) = 1): density and modulus in a checkerboard"""
    rng = np.random.default_rng(seed)
    shape = shape_of(mx, my)
    i, j = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    cb = ((i // 7 + j // 5) % 2).astype(float)
    aux = np.empty((4,) + shape, order="F")
    aux[0] = 1.0 + 3.0 * cb
    aux[1] = 1.0 + 1.5 * cb + 0.1 * rng.random(shape)
    aux[2] = 1.0
    q = np.asfortranarray(0.3 * rng.standard_normal((3,) + shape))
    aux[3] = q[0]
    dx, dy = 1.0 / mx, 0.9 / my
    return Case(name, RP_PSYSTEM, 3, 2, [0.0], q, aux, 0, bc, 0.3 * min(dx, dy) / 2.0, dx, dy, steps, 2, [2, 4], fwave=1)


def with_capa(name, rp, mx, my, bc, steps=20, seed=9, capa=True, cstate=None):
    """the aux-free solvers with a capacity function 0.5 + U(0,1) in an extra aux component"""
    rng = np.random.default_rng(seed)
    shape = shape_of(mx, my)
    dx, dy = 1.0 / mx, 0.8 / my
    if rp == RP_EULER5:
        q = np.empty((5,) + shape, order="F")
        q[0] = 1.0 + 0.1 * rng.random(shape)
        q[1] = 0.1 * rng.random(shape) - 0.03
        q[2] = 0.05 * rng.random(shape) - 0.02
        q[3] = 2.5 + 0.1 * rng.random(shape)
        q[4] = rng.random(shape)
        meqn, mwaves, par, mth, smax = 5, 5, [1.4, 0.4], [4, 4, 4, 4, 2], 2.2
    elif rp == RP_ACOUSTICS:
        q = np.asfortranarray(rng.standard_normal((3,) + shape))
        meqn, mwaves, par, mth, smax = 3, 2, [1.0, 4.0, 2.0, 2.0], [4, 3], 2.0
    elif rp == RP_ADVECTION:
        q = np.asfortranarray(rng.random((1,) + shape))
        meqn, mwaves, par, mth, smax = 1, 1, [0.7, -0.4], [2], 0.7
    else:
        q = np.empty((3,) + shape, order="F")
        q[0] = 1.0 + 0.2 * rng.random(shape)
        q[1] = 0.1 * rng.standard_normal(shape)
        q[2] = 0.1 * rng.standard_normal(shape)
        meqn, mwaves, par, mth, smax = 3, 3, [1.0], [4, 4, 1], 1.6
    quiet_patch(q, mx, my)
    # two aux components (the construction of ref_step2ds_capa.npz): the capacity function is the second
    aux = np.asfortranarray(0.5 + rng.random((2,) + shape))
    dt = 0.2 * min(dx, dy) / smax           # capa >= 0.5 doubles dt/dx: Courant number <= 0.4
    return Case(name, rp, meqn, mwaves, par, q, aux, 2 if capa else 0, bc, dt, dx, dy, steps, 2, mth, cstate=cstate)


def golden_capa():
    """the input of tests/golden/ref_step2ds_capa.npz (ids = 1: the reference's own step2ds.f ran on it), ghost cells
    as given, one step"""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_ref_goldens", os.path.join(here, "golden", "make_ref_goldens.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    z = np.load(os.path.join(here, "golden", "ref_step2ds_capa.npz"), allow_pickle=False)
    mx, my = int(z["mx"]), int(z["my"])
    q, aux = G.euler_state(21, shape_of(mx, my)), G.capa_field(21, shape_of(mx, my))
    return Case("golden_capa", RP_EULER5, 5, 5, G.PAR, q, aux, 2, [-1] * 4, float(z["dt"]), float(z["dx"]), float(z["dy"]), 1,
                2, G.MTH, ghosts=True)


def cases():
    cs = []
    # vc_acoustics_2d: grids at and around the tile sizes (60 x 12 owned cells), thin, narrow, a non-multiple
    bcs = ([PER, PER, PER, PER], [REF, OUT, OUT, REF], [OUT, REF, PER, PER], [PER, PER, REF, OUT])
    for k, (mx, my) in enumerate(((60, 12), (61, 13), (59, 11), (120, 24), (121, 25), (64, 28), (300, 5), (3, 90), (300, 100))):
        cs.append(vc_acoustics("vc_acoustics_%s_%dx%d" % (("layered", "random")[k % 2], mx, my), mx, my, ("layered", "random")[k % 2],
                               bcs[k % 4], seed=10 + k))
    cs.append(vc_acoustics("vc_acoustics_walls_300x100", 300, 100, "random", [REF, REF, OUT, OUT], seed=30))
    # 80 steps: PCL_TUNE_FUSED_STEP=2 runs its trial steps (64 .. 71 of a window) in both forms
    cs.append(vc_acoustics("vc_acoustics_window_200x90", 200, 90, "layered", [PER, PER, OUT, REF], steps=80, seed=31))
    # orders 1 and 2, every limiter id
    for order in (1, 2):
        for lim in ((0, 1), (2, 3), (4, 5), (5, 0)):
            cs.append(vc_acoustics("vc_acoustics_order%d_lim%d%d_130x75" % (order, lim[0], lim[1]), 130, 75, "random",
                                   [REF, OUT, PER, PER] if order == 1 else [PER, PER, OUT, OUT], steps=12, order=order,
                                   mthlim=lim, seed=40 + order))
    cs.append(vc_acoustics("vc_acoustics_capa_130x75", 130, 75, "layered", [REF, OUT, PER, PER], capa=True, seed=50))
    cs.append(vc_acoustics("vc_acoustics_capa_61x13", 61, 13, "random", [PER, PER, OUT, REF], capa=True, seed=51))
    cs.append(vc_advection("vc_advection_rotating_64", 64, [PER, PER, PER, PER]))
    cs.append(vc_advection("vc_advection_rotating_150", 150, [PER, PER, PER, PER]))
    cs.append(psystem("psystem_linear_130x66", 130, 66, [PER, PER, REF, OUT]))
    cs.append(psystem("psystem_linear_61x25", 61, 25, [REF, REF, PER, PER]))
    cst = np.zeros((4, 8))
    cst[0, :5] = [1.05, 0.02, 0.0, 2.55, 0.5]
    cs.append(with_capa("euler_capa_130x75", RP_EULER5, 130, 75, [CST, OUT, REF, REF], cstate=cst))
    cs.append(with_capa("euler_capa_off_130x75", RP_EULER5, 130, 75, [CST, OUT, REF, REF], capa=False, cstate=cst))
    cs.append(with_capa("euler_capa_61x13", RP_EULER5, 61, 13, [PER, PER, OUT, OUT], seed=8))
    cs.append(with_capa("acoustics_capa_121x57", RP_ACOUSTICS, 121, 57, [REF, OUT, PER, PER]))
    cs.append(with_capa("advection_capa_200x40", RP_ADVECTION, 200, 40, [PER, PER, OUT, OUT]))
    cs.append(with_capa("shallow_capa_90x61", RP_SHALLOW, 90, 61, [REF, REF, OUT, REF]))
    cs.append(golden_capa())
    return cs


def fill_ghosts(q, bc, cstate):
    """qbc = Y(X(q)) in place: x sides first, then y sides over the x-filled array (solver.py:354-452)"""
    g = MBC
    for idim in (0, 1):
        v = q if idim == 0 else q.transpose(0, 2, 1)
        n = v.shape[1]
        for side in (0, 1):
            t = bc[2 * idim + side]
            if t < 0:
                continue
            for k in range(g):
                dst = k if side == 0 else n - g + k
                if t == CST:
                    v[:, dst, :] = cstate[2 * idim + side][:v.shape[0], None]
                    continue
                if t == OUT:
                    src = g if side == 0 else n - g - 1
                elif t == PER:
                    src = n - 2 * g + k if side == 0 else g + k
                else:
                    src = 2 * g - 1 - k if side == 0 else n - g - 1 - k
                v[:, dst, :] = v[:, src, :]
                if t == REF and v.shape[0] > idim + 1:
                    v[idim + 1, dst, :] = -v[idim + 1, dst, :]
    return q


def oracle_run(coracle, c):
    """the same steps on the CPU: boundary conditions, x pass, y pass of the x-swept array (orc_step2ds)"""
    q = c.q.copy("F")
    cfls = []
    for _ in range(c.steps):
        if not c.ghosts:
            fill_ghosts(q, c.bc, c.cstate)
        # clawpack.py:538-546: qnew starts as a copy of qbc, the y pass takes the x-swept array as qold and qnew
        qnew, cfl = q.copy("F"), 0.0
        for ids, qold in ((1, q), (2, qnew)):
            _, cf = coracle.step2ds(c.rp, c.par, max(c.mx, c.my), MBC, c.mx, c.my, qold, qnew, c.aux, c.dx, c.dy, c.dt,
                                    c.method(), np.array(c.mthlim, dtype=np.int32), ids, fwave=bool(c.fwave))
            cfl = max(cfl, cf)
        q = qnew
        cfls.append(cfl)
    return q[:, MBC:-MBC, MBC:-MBC], cfls


def state_hash(q):
    # -0.0 hashed as +0.0 (np.array_equal semantics): a wavefront without a jump hands its cells through as they are,
    # the full solve computes q + 0; the two forms cut the grid into different wavefronts (tests/fused_step_worker.py)
    return hashlib.sha256(np.ascontiguousarray(q + 0.0).tobytes()).hexdigest()


def gpu_run(c):
    from pyclaw_amd import _lib as L
    lib = L.lib()
    cfg = L.Config()
    cfg.ndim = 2
    cfg.n[0], cfg.n[1] = c.mx, c.my
    cfg.mbc, cfg.meqn, cfg.mwaves, cfg.rp, cfg.maux, cfg.fwave = MBC, c.meqn, c.mwaves, c.rp, c.maux, c.fwave
    for k, m in enumerate(c.method()):
        cfg.method[k] = int(m)
    for k, m in enumerate(c.mthlim):
        cfg.mthlim[k] = m
    for k, p in enumerate(c.par):
        cfg.rp_params[k] = p
    cfg.d[0], cfg.d[1] = c.dx, c.dy
    h = C.c_void_p()
    L.check(lib.pcl_create(C.byref(cfg), C.byref(h)))
    try:
        L.check(lib.pcl_put_aux(h, L.d(c.aux)))
        if c.ghosts:
            L.check(lib.pcl_put_q(h, L.d(c.q), 1))
        else:                               # the ghost frame starts as NaN: the step has to evaluate the boundary conditions
            L.check(lib.pcl_put_q(h, L.d(np.full(c.q.shape, np.nan, order="F")), 1))
            L.check(lib.pcl_put_q(h, L.d(np.asfortranarray(c.q[:, MBC:-MBC, MBC:-MBC])), 0))
        bc = np.array(c.bc, dtype=np.int32)
        cst = np.ascontiguousarray(c.cstate, dtype=np.float64)
        cfls = []
        for _ in range(c.steps):
            cfl = C.c_double()
            if c.ghosts:
                L.check(lib.pcl_step_hyperbolic(h, c.dt, C.cast(C.byref(cfl), L.dp)))
            else:
                L.check(lib.pcl_bc_step(h, L.i(bc), L.d(cst), c.dt, C.cast(C.byref(cfl), L.dp)))
            cfls.append(cfl.value)
        out = np.zeros((c.meqn, c.mx, c.my), order="F")
        L.check(lib.pcl_get_q(h, L.d(out), 0))
        ms, nl = np.zeros(3), np.zeros(3, dtype=np.int64)
        s1, s0 = C.c_long(0), C.c_long(0)
        L.check(lib.pcl_step_form_stats(h, L.d(ms), nl.ctypes.data_as(C.POINTER(C.c_long)), C.byref(s1), C.byref(s0)))
    finally:
        lib.pcl_destroy(h)
    return out, cfls, [int(s1.value), int(s0.value)]


def main():
    res, dump = {}, {}
    for c in cases():
        out, cfls, forms = gpu_run(c)
        res[c.name] = {"hash": state_hash(out), "cfl": [repr(v) for v in cfls], "forms": forms,
                       "finite": bool(np.isfinite(out).all())}
        dump[c.name] = out
    if len(sys.argv) > 1:
        np.savez(sys.argv[1], **dump)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
