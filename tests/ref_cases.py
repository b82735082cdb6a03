"""
The cases that pin the classic 1-D, 2-D and 3-D steps to the reference's own step and flux Fortran, stated once.

tests/test_oracle_vs_ref.py (oracle, and the flang build where it is present) and tests/test_gpu_ref_pins.py (device) both
take key and input from here, so a pin's key and its input cannot drift apart.

The reference build behind these pins is the reference's step1.f / step1fw.f / step2.f / step2ds.f / flux2.f / flux2fw.f /
step3.f / step3ds.f / flux3.f / limiter.f / philim.f, unchanged, linked against this repository's restated Riemann solvers
(oracle/ref_rp_shim.c).  So the pins cover the step around the solver -- slicing, aux rows, Godunov update, CFL, limiter,
second-order and transverse corrections, flux differencing with and without capa -- and do NOT cover the third-party
solver formulas, which are the oracle's on both sides.

A BLOCK is one (solver, extents): what a test function is parametrised over.  groups(block) yields (key, g) for every
step kind, order and capa choice on the block's one seeded state; a group g runs once per limiter vector in g["mthlims"]
and its pin holds the results of all of them (run_host: outputs stacked on a leading axis, the Courant numbers as a vector).

Shapes are the smallest at which the kernels' tile, strip and wavefront edges occur: 1 cell, a few cells, just under and
over 64 (one wavefront / one strip), and one extent past 128 (more than one block).  States are admissible: h > 0, p > 0,
positive impedances, sound speeds, densities and capacities, so no result holds a NaN.
"""
import numpy as np

from oracle import oracle as O

MBC = 2

# ---------------------------------------------------------------------------------------------------- 1-D
# name -> (rp, meqn, mwaves, solver aux components, fwave)
SOLVERS_1D = {
    "advection": (O.RP_ADVECTION_1D, 1, 1, 0, False),
    "acoustics": (O.RP_ACOUSTICS_1D, 2, 2, 0, False),
    "burgers": (O.RP_BURGERS_1D, 1, 1, 0, False),
    "euler": (O.RP_EULER_1D, 3, 3, 0, False),
    "shallow": (O.RP_SHALLOW_1D, 2, 2, 0, False),
    "advection_color": (O.RP_ADVECTION_COLOR_1D, 1, 1, 1, False),
    "elasticity_fwave": (O.RP_ELASTICITY_FWAVE_1D, 2, 2, 3, True),              # linear stress in every cell
    "elasticity_fwave_exp": (O.RP_ELASTICITY_FWAVE_1D, 2, 2, 3, True),          # cells of linear and of exponential stress
}
MX_1D = [1, 2, 61, 300]
LIMITERS_1D = [0, 1, 2, 3, 4, 5]

# ---------------------------------------------------------------------------------------------------- 2-D
# name -> (rp, meqn, mwaves, solver aux components, fwave)
SOLVERS_2D = {
    "acoustics": (O.RP_ACOUSTICS_2D, 3, 2, 0, False),
    "advection": (O.RP_ADVECTION_2D, 1, 1, 0, False),
    "shallow": (O.RP_SHALLOW_2D, 3, 3, 0, False),
    "vc_acoustics": (O.RP_VC_ACOUSTICS_2D, 3, 2, 2, False),
    "vc_advection": (O.RP_VC_ADVECTION_2D, 1, 1, 2, False),
    "psystem_fwave_linear": (O.RP_PSYSTEM_FWAVE_2D, 3, 2, 4, True),
    "psystem_fwave_exp": (O.RP_PSYSTEM_FWAVE_2D, 3, 2, 4, True),
}
SHAPES_2D = [(1, 1), (7, 5), (61, 59), (130, 17)]


# Blocks the host back ends run and the GPU leg does not: the exponential stress law calls exp() inside the Riemann solver,
# and the device's exp() differs from glibc's by an ulp (tests/test_fwave.py holds those solvers to the oracle to 1e-13).
# That is solver arithmetic, outside what these pins cover; the GPU leg is bitwise or absent, so they are absent there.
# The f-wave STEP (step1fw.f, flux2fw.f) reaches the device through the linear-stress blocks.
HOST_ONLY = ("elasticity_fwave_exp", "psystem_fwave_exp")


def limiter_vectors_2d(mwaves):
    """all-MC, mixed, all-zero"""
    return [[4] * mwaves, [3, 1, 5][:mwaves], [0] * mwaves]


# ---------------------------------------------------------------------------------------------------- 3-D
SHAPES_3D = [(1, 1, 1), (9, 7, 5), (61, 6, 9), (3, 17, 2), (65, 20, 3)]
TRANS_ORDER_3D = [(t, o) for t in (0, 10, 11) for o in (1, 2)] + [(t, 2) for t in (20, 21, 22)]
LIMITERS_3D = [[4, 3], [1, 2], [5, 0], [0, 0]]


def blocks(dim, device=False):
    """[(solver name, extents)] of a dimension, in a fixed order; device=True: those of the GPU leg (not HOST_ONLY)"""
    if dim == 1:
        every = [(s, (mx,)) for s in SOLVERS_1D for mx in MX_1D]
    elif dim == 2:
        every = [(s, n) for s in SOLVERS_2D for n in SHAPES_2D]
    else:
        every = [("vc_acoustics", n) for n in SHAPES_3D]
    return [b for b in every if not (device and b[0] in HOST_ONLY)]


def block_id(block):
    return "%s-%s" % (block[0], "x".join(str(k) for k in block[1]))


def _seed(name, n):
    return [sum(ord(c) for c in name)] + list(n)


def _with_capa(rng, aux, full):
    """the capacity function as one more aux component behind the solver's own: values in [0.5, 1.5)"""
    capa = 0.5 + rng.random((1,) + full)
    return np.asfortranarray(capa if aux is None else np.concatenate([aux, capa]))


def _method(order, trans, mcapa, maux):
    return np.array([1, order, trans, 0, 0, mcapa, maux], dtype=np.int32)


def _state_1d(name, rng, full):
    meqn = SOLVERS_1D[name][1]
    q = np.empty((meqn,) + full, order="F")
    par, aux = [0.0], None
    if name == "advection":
        q[0] = rng.standard_normal(full)
        par = [0.8 if full[0] % 2 else -0.7]
    elif name == "acoustics":
        q[...] = rng.standard_normal((2,) + full)
        par = [1.0, 4.0, 2.0, 2.0]                              # rho, bulk, c, Z
    elif name == "burgers":
        q[0] = rng.standard_normal(full)                        # both signs: transonic rarefactions occur
    elif name == "euler":
        rho = 0.2 + 2.0 * rng.random(full)
        u = 3.0 * (rng.random(full) - 0.5)
        p = 0.1 + 2.0 * rng.random(full)
        q[0], q[1], q[2] = rho, rho * u, p / 0.4 + 0.5 * rho * u * u
        par = [1.4, 0.4]
    elif name == "shallow":
        h = 0.2 + 2.0 * rng.random(full)
        q[0], q[1] = h, h * 2.0 * (rng.random(full) - 0.5)
        par = [9.81]
    elif name == "advection_color":
        q[0] = rng.random(full)
        aux = np.asfortranarray(1.5 * (rng.random((1,) + full) - 0.3))          # edge velocities of both signs
    elif name.startswith("elasticity_fwave"):
        q[0] = 0.2 * (rng.random(full) - 0.5)                                   # strain
        aux = np.empty((3,) + full, order="F")
        aux[0] = 0.5 + 2.0 * rng.random(full)                                   # density
        aux[1] = 0.5 + 2.0 * rng.random(full)                                   # K
        # 1: linear stress, 0: exponential
        aux[2] = (rng.random(full) < 0.5).astype(np.float64) if name.endswith("exp") else 1.0
        q[1] = aux[0] * (rng.random(full) - 0.5)                                # momentum
    return q, aux, par


def _state_2d(name, rng, full):
    meqn = SOLVERS_2D[name][1]
    q = np.empty((meqn,) + full, order="F")
    par, aux = [0.0], None
    if name == "acoustics":
        q[...] = rng.standard_normal((3,) + full)
        par = [1.0, 4.0, 2.0, 2.0]
    elif name == "advection":
        q[0] = rng.standard_normal(full)
        par = [0.7, -0.4]
    elif name == "shallow":
        h = 0.2 + 2.0 * rng.random(full)
        q[0] = h
        q[1] = h * 2.0 * (rng.random(full) - 0.5)
        q[2] = h * 2.0 * (rng.random(full) - 0.5)
        par = [9.81]
    elif name == "vc_acoustics":
        q[...] = rng.standard_normal((3,) + full)
        aux = np.asfortranarray(0.5 + 2.0 * rng.random((2,) + full))            # impedance, sound speed
    elif name == "vc_advection":
        q[0] = rng.random(full)
        aux = np.asfortranarray(1.5 * (rng.random((2,) + full) - 0.4))          # edge velocities of both signs
    else:                                                                       # psystem_fwave_*
        q[0] = 0.2 * (rng.random(full) - 0.5)
        aux = np.empty((4,) + full, order="F")
        aux[0] = 0.5 + 2.0 * rng.random(full)
        aux[1] = 0.5 + 2.0 * rng.random(full)
        aux[2] = 1.0 if name.endswith("linear") else 0.0
        aux[3] = q[0]                                                           # the app copies the strain there
        q[1] = aux[0] * (rng.random(full) - 0.5)
        q[2] = aux[0] * (rng.random(full) - 0.5)
    return q, aux, par


def groups(dim, block):
    """(key, g) for every group of the block; g is a dict: what run_host and the device runner read"""
    name, n = block
    rng = np.random.default_rng(_seed(name, n))
    full = tuple(k + 2 * MBC for k in n)
    base = "%dd/%s/%s" % (dim, name, "x".join(str(k) for k in n))
    if dim == 1:
        rp, meqn, mwaves, saux, fwave = SOLVERS_1D[name]
        q, aux, par = _state_1d(name, rng, full)
        auxc = _with_capa(rng, aux, full)
        (mx,) = n
        for capa in ((0,) if fwave else (0, 1)):
            maux = saux + capa
            for order in (1, 2):
                yield "%s/order%d/capa%d" % (base, order, capa), dict(
                    dim=1, kind="step1", rp=rp, par=par, meqn=meqn, mwaves=mwaves, maux=maux, n=n, q=q,
                    aux=auxc if capa else aux, d=(1.0 / mx,), dt=0.3 / mx, fwave=fwave, arg=None,
                    method=_method(order, 0, maux if capa else 0, maux), mthlims=[[lim] * mwaves for lim in LIMITERS_1D],
                    whole=False)
    elif dim == 2:
        rp, meqn, mwaves, saux, fwave = SOLVERS_2D[name]
        q, aux, par = _state_2d(name, rng, full)
        auxc = _with_capa(rng, aux, full)
        mx, my = n
        d = (1.0 / mx, 0.8 / my)
        dt = 0.1 / max(mx, my)
        for capa in (0, 1):
            maux = saux + capa
            for order in (1, 2):
                common = dict(dim=2, rp=rp, par=par, meqn=meqn, mwaves=mwaves, maux=maux, n=n, q=q,
                              aux=auxc if capa else aux, d=d, dt=dt, fwave=fwave, mthlims=limiter_vectors_2d(mwaves))
                for ids in (1, 2):
                    yield "%s/ids%d/order%d/capa%d" % (base, ids, order, capa), dict(
                        common, kind="step2ds", arg=ids, whole=True, method=_method(order, -1, maux if capa else 0, maux))
                for trans in (0, 1, 2):
                    yield "%s/trans%d/order%d/capa%d" % (base, trans, order, capa), dict(
                        common, kind="step2", arg=None, whole=False,
                        method=_method(order, trans, maux if capa else 0, maux))
    else:
        q = np.asfortranarray(rng.standard_normal((4,) + full))
        aux = np.asfortranarray(0.5 + 2.0 * rng.random((2,) + full))            # impedance, sound speed
        auxc = _with_capa(rng, aux, full)
        common = dict(dim=3, rp=O.RP_VC_ACOUSTICS_3D, par=None, meqn=4, mwaves=2, n=n, q=q, d=(0.1, 0.07, 0.13), dt=0.02,
                      fwave=False, mthlims=LIMITERS_3D)
        for trans, order in TRANS_ORDER_3D:
            yield "%s/trans%d/order%d" % (base, trans, order), dict(
                common, kind="step3", arg=None, whole=False, maux=2, aux=aux, method=_method(order, trans, 0, 2))
        for capa in (0, 1):
            for idir in (1, 2, 3):
                for order in (1, 2):
                    yield "%s/idir%d/order%d/capa%d" % (base, idir, order, capa), dict(
                        common, kind="step3ds", arg=idir, whole=True, maux=2 + capa, aux=auxc if capa else aux,
                        method=_method(order, -1, 3 if capa else 0, 2 + capa))


def compared(g, out):
    """the part of a step's result that is compared: the whole array for the dimension-split 2-D and 3-D steps, the
    interior for the unsplit steps (their outermost ghost cells receive transverse increments nobody reads) and for 1-D
    (step1.f also dirties ghost cells 0 and mx+1)"""
    if g["whole"]:
        return out
    return out[(slice(None),) + (slice(MBC, -MBC),) * g["dim"]]


def run_host(backend, g):
    """the group on a host back end with the call surface of oracle.COracle (the oracle itself, or the RefClassic*
    builds of the reference Fortran) -> (compared results stacked over the limiter vectors, their Courant numbers)"""
    outs, cfls = [], []
    n, d, q0 = g["n"], g["d"], g["q"]
    maxm = max(n)
    for mth in g["mthlims"]:
        a = q0.copy("F")
        if g["kind"] == "step1":
            _, cfl = backend.step1(g["rp"], g["par"], MBC, n[0], a, g["aux"], d[0], g["dt"], g["method"], mth,
                                   fwave=g["fwave"])
        elif g["kind"] == "step2ds":
            _, cfl = backend.step2ds(g["rp"], g["par"], maxm, MBC, n[0], n[1], q0.copy("F"), a, g["aux"], d[0], d[1], g["dt"],
                                     g["method"], mth, g["arg"], fwave=g["fwave"])
        elif g["kind"] == "step2":
            _, cfl = backend.step2(g["rp"], g["par"], maxm, MBC, n[0], n[1], q0.copy("F"), a, g["aux"], d[0], d[1], g["dt"],
                                   g["method"], mth, fwave=g["fwave"])
        elif g["kind"] == "step3ds":
            _, cfl = backend.step3ds(g["rp"], maxm, MBC, n[0], n[1], n[2], q0.copy("F"), a, g["aux"], d[0], d[1], d[2],
                                     g["dt"], g["method"], mth, g["arg"])
        else:
            _, cfl = backend.step3(g["rp"], maxm, MBC, n[0], n[1], n[2], q0.copy("F"), a, g["aux"], d[0], d[1], d[2], g["dt"],
                                   g["method"], mth)
        outs.append(compared(g, a).copy())
        cfls.append(cfl)
    return np.stack(outs), np.array(cfls)
