"""
GPU: user-written Riemann solvers that read aux arrays (pyclaw.CellRiemann(..., aux=...), pcl_cellrp_compile_aux;
DESIGN.md 4.4d).  The library compiles its own sweep kernel with NAUX > 0 around the body, so the built-in solvers with
cell-wise coefficients restated as bodies (apps/problems.py) must give the bits of the built-in path: against the frozen
oracle through the solver handle with the aux array put beside q, with the coefficients in other components than 0 and 1,
on states with flat stretches of q inside noisy aux (the jump-free shortcut takes the body's speeds, each interface with
its own aux), and through the public interface against the same run with the built-in solver.  A solver the library does
not have (1-D acoustics in a layered medium) is checked against a numpy Godunov update on dyadic data, where every
operation is exact.  'exact' arithmetic; comparisons are equalities.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyclaw_amd as pyclaw
from apps import problems
from oracle import oracle as O
from pyclaw_amd import _lib as L

PCL_RP_CELL = 100


class Handle(object):
    """a PCL_RP_CELL solver handle with maux aux components and `body`, which reads the components `aux`, compiled"""

    def __init__(self, body, meqn, mwaves, shape, d, mbc, order, mthlim, maux, aux, math=0):
        ndim = len(shape)
        self.rp = pyclaw.CellRiemann(body, meqn, mwaves, ndim, aux=aux).compile(['exact', 'fast', 'strict'][math])
        cfg = L.Config()
        cfg.ndim = ndim
        for k in range(ndim):
            cfg.n[k] = shape[k]
            cfg.d[k] = d[k]
        cfg.mbc, cfg.meqn, cfg.mwaves, cfg.maux = mbc, meqn, mwaves, maux
        for k, v in enumerate([1, order, -1 if ndim == 2 else 0, 0, 0, 0, maux]):
            cfg.method[k] = v
        for k, m in enumerate(mthlim):
            cfg.mthlim[k] = m
        cfg.rp = PCL_RP_CELL
        cfg.math = math
        self.h = C.c_void_p()
        L.check(L.lib().pcl_create(C.byref(cfg), C.byref(self.h)))

    def attach(self):
        L.check(L.lib().pcl_cellrp_attach(self.h, self.rp._rp))
        return self

    def put_aux(self, aux):
        """the aux array with its ghost cells"""
        assert aux.flags.f_contiguous
        L.check(L.lib().pcl_put_aux(self.h, L.d(aux)))
        return self

    def sweep(self, q0, ids, dt):
        """one pass over q0 (ghost cells included); returns the new array with ghosts and the Courant number"""
        lib = L.lib()
        cfl = C.c_double()
        L.check(lib.pcl_put_q(self.h, L.d(q0), 1))
        L.check(lib.pcl_sweep(self.h, ids, dt, C.cast(C.byref(cfl), L.dp)))
        out = np.empty_like(q0, order="F")
        L.check(lib.pcl_get_q(self.h, L.d(out), 1))
        return out, cfl.value

    def step(self, q0, dt):
        lib = L.lib()
        cfl = C.c_double()
        L.check(lib.pcl_put_q(self.h, L.d(q0), 1))
        L.check(lib.pcl_step_hyperbolic(self.h, dt, C.cast(C.byref(cfl), L.dp)))
        out = np.empty_like(q0, order="F")
        L.check(lib.pcl_get_q(self.h, L.d(out), 1))
        return out, cfl.value

    def close(self):
        L.lib().pcl_destroy(self.h)
        self.h = None


# ---- the restated solvers against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("mx", [1, 7, 61, 241, 257])
def test_colour_equation_1d_against_the_oracle(coracle, mx):
    """velocities standard normal: both signs, so both fluctuations run"""
    rng = np.random.default_rng(13 * mx)
    mbc = 2
    q0 = np.asfortranarray(rng.standard_normal((1, mx + 2 * mbc)))
    aux = np.asfortranarray(rng.standard_normal((1, mx + 2 * mbc)))
    dx, dt = 1.0 / mx, 0.2 / mx
    for lim in [[4], [1], [0]]:
        for order in (1, 2):
            method = np.array([1, order, 0, 0, 0, 0, 1], dtype=np.int32)
            ref = q0.copy("F")
            _, cfl_ref = coracle.step1(O.RP_ADVECTION_COLOR_1D, np.zeros(8), mbc, mx, ref, aux, dx, dt, method,
                                       np.array(lim, dtype=np.int32))
            hd = Handle(problems.ADVECTION_COLOR_1D_RP, 1, 1, (mx,), (dx,), mbc, order, lim, 1, (0,)).attach().put_aux(aux)
            try:
                out, cfl = hd.sweep(q0, 1, dt)
                out2, cfl2 = hd.step(q0, dt)
            finally:
                hd.close()
            # interior cells: the Fortran also dirties ghost cells 0 and mx+1, which nobody reads (test_gpu_classic.py)
            assert np.array_equal(out[:, mbc:-mbc], ref[:, mbc:-mbc]), (lim, order, np.abs(out - ref)[:, mbc:-mbc].max())
            assert cfl == cfl_ref and cfl > 0, (lim, order)
            assert np.array_equal(out2, out) and cfl2 == cfl


def check_2d(coracle, name, rp, meqn, mwaves, q0, coef, mx, my, mbc, lims, orders, maux=2, listed=(0, 1), dev_aux=None):
    """coef: the solver's two coefficient planes (what the oracle gets as aux(1), aux(2)); dev_aux: the aux array of the
    device handle where it is not coef itself, with the body listing `listed`"""
    dev_aux = coef if dev_aux is None else dev_aux
    dx, dy, dt = 2.0 / mx, 2.0 / my, 0.2 / max(mx, my)
    results = []
    for lim in lims:
        for order in orders:
            method = np.array([1, order, -1, 0, 0, 0, 2], dtype=np.int32)
            mth = np.array(lim, dtype=np.int32)
            hd = Handle(getattr(problems, name), meqn, mwaves, (mx, my), (dx, dy), mbc, order, lim, maux, listed).attach()
            hd.put_aux(dev_aux)
            try:
                passes = []
                for ids in (1, 2):
                    ref = q0.copy("F")
                    _, cfl_ref = coracle.step2ds(rp, np.zeros(8), max(mx, my), mbc, mx, my, q0.copy("F"), ref, coef, dx, dy, dt,
                                                 method, mth, ids)
                    out, cfl = hd.sweep(q0, ids, dt)
                    assert np.array_equal(out, ref), (lim, order, ids, np.abs(out - ref).max())
                    assert cfl == cfl_ref, (lim, order, ids)
                    passes.append((ref, cfl_ref))
                # the whole step: the y pass over the x pass' result, the larger of the two Courant numbers
                ref2 = passes[0][0].copy("F")
                _, cfl_y = coracle.step2ds(rp, np.zeros(8), max(mx, my), mbc, mx, my, passes[0][0].copy("F"), ref2, coef, dx, dy,
                                           dt, method, mth, 2)
                out, cfl = hd.step(q0, dt)
                assert np.array_equal(out, ref2), (lim, order, "step", np.abs(out - ref2).max())
                assert cfl == max(passes[0][1], cfl_y), (lim, order, "step")
                results.append((passes[0][1], passes[1][1], out))
            finally:
                hd.close()
    return results


def coefficients(name, rng, shape):
    """edge velocities: standard normal, both signs; impedance and sound speed: uniform in [0.5, 2], positive as the
    solver requires"""
    if name == "VC_ADVECTION_2D_RP":
        return np.asfortranarray(rng.standard_normal((2,) + shape))
    return np.asfortranarray(rng.uniform(0.5, 2.0, (2,) + shape))


SYSTEMS_2D = [("VC_ADVECTION_2D_RP", O.RP_VC_ADVECTION_2D, 1, 1), ("VC_ACOUSTICS_2D_RP", O.RP_VC_ACOUSTICS_2D, 3, 2)]
LIMITERS_2D = {1: [[4], [1], [0]], 2: [[4, 4], [1, 2], [0, 0]]}


@pytest.mark.parametrize("mx,my", [(1, 1), (7, 5), (61, 59), (241, 65)])
@pytest.mark.parametrize("name,rp,meqn,mwaves", SYSTEMS_2D)
def test_restated_2d_solvers_against_the_oracle(coracle, name, rp, meqn, mwaves, mx, my):
    """(61, 59): one cell over the 60-cell strip; (241, 65): one over the 240-cell x tile and the 64-row y tile"""
    rng = np.random.default_rng(7 * mx + my + meqn)
    q0 = np.asfortranarray(rng.standard_normal((meqn, mx + 4, my + 4)))
    coef = coefficients(name, rng, (mx + 4, my + 4))
    check_2d(coracle, name, rp, meqn, mwaves, q0, coef, mx, my, 2, LIMITERS_2D[mwaves], (1, 2))


@pytest.mark.parametrize("name,rp,meqn,mwaves", SYSTEMS_2D)
def test_restated_2d_solvers_with_three_ghost_layers(coracle, name, rp, meqn, mwaves):
    rng = np.random.default_rng(5 + meqn)
    mx, my, mbc = 61, 59, 3
    q0 = np.asfortranarray(rng.standard_normal((meqn, mx + 2 * mbc, my + 2 * mbc)))
    coef = coefficients(name, rng, (mx + 2 * mbc, my + 2 * mbc))
    check_2d(coracle, name, rp, meqn, mwaves, q0, coef, mx, my, mbc, LIMITERS_2D[mwaves][:1], (2,))


def test_the_listed_components_are_the_ones_the_body_gets(coracle):
    """maux = 4 with the impedance in component 3, the sound speed in component 1 and NaN in 0 and 2: the body lists
    (3, 1) and computes the bits of the run with the same coefficients in (0, 1) -- which are the oracle's"""
    rng = np.random.default_rng(31)
    mx, my = 61, 59
    q0 = np.asfortranarray(rng.standard_normal((3, mx + 4, my + 4)))
    coef = coefficients("VC_ACOUSTICS_2D_RP", rng, (mx + 4, my + 4))
    aux4 = np.asfortranarray(np.full((4, mx + 4, my + 4), np.nan))
    aux4[3], aux4[1] = coef[0], coef[1]
    args = (coracle, "VC_ACOUSTICS_2D_RP", O.RP_VC_ACOUSTICS_2D, 3, 2, q0, coef, mx, my, 2, LIMITERS_2D[2][:1], (2,))
    (cx, cy, out), = check_2d(*args)
    (cx4, cy4, out4), = check_2d(*args, maux=4, listed=(3, 1), dev_aux=aux4)
    assert np.array_equal(out4, out) and (cx4, cy4) == (cx, cy) and np.isfinite(out4).all()


@pytest.mark.parametrize("name,rp,meqn,mwaves", SYSTEMS_2D)
def test_flat_q_inside_noisy_aux_takes_the_speeds_of_the_body(coracle, name, rp, meqn, mwaves):
    """a block of 170 x 150 equal q cells inside noise, and whole constant rows and columns, with aux noisy everywhere:
    wavefronts of either pass lie inside the block, are jump-free in q and take speeds(), the body again, every interface
    with its own auxl / auxr.  The largest speed of the whole array sits inside the block, so the Courant number of
    either pass comes out right only through that path."""
    rng = np.random.default_rng(3 + meqn)
    mx, my = 257, 200
    q0 = np.asfortranarray(rng.standard_normal((meqn, mx + 4, my + 4)))
    for m in range(meqn):
        q0[m, 40:210, 30:180] = 0.25 * (m + 1)
        q0[m, :, 190:194] = -0.5 * (m + 1)
        q0[m, 230:236, :] = 1.5 + m
    coef = coefficients(name, rng, (mx + 4, my + 4))
    # cell (100, 100): inside the strip of cells 60..123 of row 100 (x pass) and of column 100 (y pass), all of the block
    if name == "VC_ADVECTION_2D_RP":
        coef[0, 100, 100] = coef[1, 100, 100] = -7.0         # both edge velocities; the rest is standard normal
        speed = np.abs(coef)
        top = [np.unravel_index(np.argmax(speed[k]), speed[k].shape) for k in (0, 1)]
        assert top == [(100, 100), (100, 100)] and speed[:, 100, 100].min() == 7.0
    else:
        coef[1, 100, 100] = 3.0                              # the sound speed; the rest is below 2
        top = np.unravel_index(np.argmax(coef[1]), coef[1].shape)
        assert top == (100, 100)
    assert 60 <= 100 < 124 and 40 <= 60 and 124 <= 210 and 30 <= 60 and 124 <= 180
    dtdx, dtdy = (0.2 / 257) / (2.0 / mx), (0.2 / 257) / (2.0 / my)
    big = 7.0 if name == "VC_ADVECTION_2D_RP" else 3.0
    for cx, cy, _ in check_2d(coracle, name, rp, meqn, mwaves, q0, coef, mx, my, 2, LIMITERS_2D[mwaves][:2], (2,)):
        # (the oracle's Courant numbers, which the device's were equal to: those of the planted cell)
        assert cx == pytest.approx(dtdx * big, rel=1e-14) and cy == pytest.approx(dtdy * big, rel=1e-14)


# ---- a solver the library does not have --------------------------------------------------------------------------------------
def layered_godunov_step(q, zz, cc, dtd, mbc):
    """first-order update of the interior cells by VC_ACOUSTICS_1D_RP in numpy, any float type: q (2, n), zz and cc (n,);
    returns the new array and the Courant number over the interfaces mbc .. mbc + mx (step1.f)"""
    mx = q.shape[1] - 2 * mbc
    sl, sr = slice(mbc - 1, mbc + mx), slice(mbc, mbc + mx + 1)        # interface k lies between cells k-1 and k
    d1, d2 = q[0, sr] - q[0, sl], q[1, sr] - q[1, sl]
    zim, zi = zz[sl], zz[sr]
    a1 = (-d1 + zi * d2) / (zim + zi)
    a2 = (d1 + zim * d2) / (zim + zi)
    s0, s1 = -cc[sl], cc[sr]
    amdq = np.stack([s0 * (-a1 * zim), s0 * a1])
    apdq = np.stack([s1 * (a2 * zi), s1 * a2])
    new = q.copy()
    new[:, mbc:mbc + mx] = q[:, mbc:mbc + mx] - dtd * apdq[:, :-1] - dtd * amdq[:, 1:]
    return new, max((dtd * np.abs(s0)).max(), (dtd * np.abs(s1)).max())


@pytest.mark.parametrize("mx", [61, 257])
def test_layered_acoustics_1d_against_a_numpy_godunov_update(mx):
    """Z = 1 in every cell (the divisor is 2), c from {0.5, 1, 2} cell by cell, q integer multiples of 1/64 in [-2, 2],
    dt/dx = 1/4: every product, quotient and sum of the first-order step is exact in double precision whatever the order
    of operations, which the long-double recomputation below verifies; the comparison with the device is an equality."""
    rng = np.random.default_rng(mx)
    mbc = 2
    n = mx + 2 * mbc
    q0 = rng.integers(-128, 129, size=(2, n)).astype(np.float64) / 64.0
    zz = np.ones(n)
    cc = rng.choice([0.5, 1.0, 2.0], size=n)
    assert len(set(cc[mbc:-mbc])) == 3
    ref, cfl_ref = layered_godunov_step(q0, zz, cc, 0.25, mbc)
    ld = np.longdouble
    refl, cfll = layered_godunov_step(q0.astype(ld), zz.astype(ld), cc.astype(ld), ld(0.25), mbc)
    assert np.array_equal(ref.astype(ld), refl) and ld(cfl_ref) == cfll and cfl_ref == 0.5
    d = 1.0 / 64
    aux = np.asfortranarray(np.stack([zz, cc]))
    hd = Handle(problems.VC_ACOUSTICS_1D_RP, 2, 2, (mx,), (d,), mbc, 1, [0, 0], 2, (0, 1)).attach().put_aux(aux)
    try:
        out, cfl = hd.step(np.asfortranarray(q0), 0.25 * d)
    finally:
        hd.close()
    assert np.array_equal(out[:, mbc:-mbc], ref[:, mbc:-mbc]), np.abs(out - ref)[:, mbc:-mbc].max()
    assert cfl == cfl_ref


# ---- refusals that need a solver handle ---------------------------------------------------------------------------------------
def test_a_list_past_maux_is_refused_at_attach_and_nothing_is_attached():
    hd = Handle("s[0] = auxr[0];", 1, 1, (7, 5), (0.1, 0.1), 2, 2, [4], 2, (2,))
    try:
        assert L.lib().pcl_cellrp_attach(hd.h, hd.rp._rp) == L.EINVAL
        msg = L.lib().pcl_last_error().decode()
        assert "aux component 2" in msg and "maux = 2" in msg
        q0 = np.asfortranarray(np.ones((1, 11, 9)))
        cfl = C.c_double()
        L.check(L.lib().pcl_put_q(hd.h, L.d(q0), 1))
        L.check(L.lib().pcl_put_aux(hd.h, L.d(np.asfortranarray(np.ones((2, 11, 9))))))
        rc = L.lib().pcl_step_hyperbolic(hd.h, 0.01, C.cast(C.byref(cfl), L.dp))
        assert rc == L.ESTATE and b"pcl_cellrp_attach" in L.lib().pcl_last_error()
    finally:
        hd.close()


def test_a_step_before_the_aux_array_was_put_is_refused():
    hd = Handle(problems.VC_ADVECTION_2D_RP, 1, 1, (7, 5), (0.1, 0.1), 2, 2, [4], 2, (0, 1)).attach()
    try:
        q0 = np.asfortranarray(np.ones((1, 11, 9)))
        cfl = C.c_double()
        L.check(L.lib().pcl_put_q(hd.h, L.d(q0), 1))
        for call in (lambda: L.lib().pcl_step_hyperbolic(hd.h, 0.01, C.cast(C.byref(cfl), L.dp)),
                     lambda: L.lib().pcl_sweep(hd.h, 2, 0.01, C.cast(C.byref(cfl), L.dp))):
            assert call() == L.EINVAL
            assert b"reads aux arrays and there are none" in L.lib().pcl_last_error()
        out, _ = hd.put_aux(np.asfortranarray(np.ones((2, 11, 9)))).step(q0, 0.01)       # and with it the step runs
        assert np.array_equal(out, q0)
    finally:
        hd.close()


# ---- the public interface ----------------------------------------------------------------------------------------------------
def traced(solver):
    """(dt, Courant number) of every hyperbolic step, rejected ones included"""
    log, inner = [], solver.step_hyperbolic

    def step_hyperbolic(solution):
        inner(solution)
        log.append((solver.dt, solver.cfl.get_cached_max()))
    solver.step_hyperbolic = step_hyperbolic
    return log


def layered_claw(user, math='exact', hook=False):
    claw = problems.vc_acoustics2D(pyclaw, mx=61, my=59, run=False, math=math, user_rp=user)
    s = claw.solver
    s.bc_lower[0], s.bc_upper[0] = pyclaw.BC.reflecting, pyclaw.BC.outflow
    s.bc_lower[1], s.bc_upper[1] = pyclaw.BC.outflow, pyclaw.BC.reflecting
    if hook:        # the sound speed grows about 3 % a step, on the device
        s.start_step = pyclaw.CellStartStep("aux[1] = aux[1] * (1.0 + 4.0 * c.dt);", writes_aux=True)
    return claw


def colour_claw(user):
    solver = pyclaw.ClawSolver1D()
    solver.rp = (pyclaw.CellRiemann(problems.ADVECTION_COLOR_1D_RP, 1, 1, 1, aux=(0,)) if user
                 else pyclaw.riemann.rp_advection_color_1d)
    solver.mwaves = 1
    solver.limiters = 4
    solver.bc_lower[0] = solver.bc_upper[0] = pyclaw.BC.periodic
    solver.aux_bc_lower[0] = solver.aux_bc_upper[0] = pyclaw.BC.periodic
    state = pyclaw.State(pyclaw.Grid([pyclaw.Dimension('x', 0.0, 1.0, 257)]), 1, 1)
    xc, xe = state.grid.x.center, state.grid.x.edge
    state.q[0, :] = np.exp(-80.0 * (xc - 0.4) ** 2)
    state.aux[0, :] = 0.25 + np.sin(2 * np.pi * xe[:-1])            # velocity at the left edge: both signs
    claw = pyclaw.Controller()
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    solver.dt_initial = 0.5 / 257
    return claw


def run_steps(claw, nsteps, resident=False):
    """nsteps accepted steps, one evolve_to_time call each"""
    solver, solution = claw.solver, claw.solution
    log = traced(solver)
    solver.setup(solution)
    solver.dt = solver.dt_initial
    if resident:
        solver.begin_resident(solution)
    for k in range(nsteps):
        solver.evolve_to_time(solution)
    if resident:
        solver.end_resident(solution)
    q = solution.state.q.copy()
    solver.teardown()
    forms = solver.status.get("step_forms")
    return q, log, forms


def test_claw_solver_2d_equals_the_built_in_run():
    """10 steps of a 61 x 59 box in a layered medium, reflecting / outflow sides, variable dt: q, every dt and every
    Courant number of the run with rp_vc_acoustics_2d; the user run takes the two passes"""
    q_ref, log_ref, forms_ref = run_steps(layered_claw(False), 10)
    q, log, forms = run_steps(layered_claw(True), 10)
    print("forms: built-in %s, user %s" % (forms_ref, forms))
    assert forms["one_kernel"] == 0 and forms["two_pass"] >= 10
    assert len(log) >= 10 and log == log_ref
    assert np.array_equal(q, q_ref)


def test_aux_written_on_the_device_every_step_is_what_the_body_sees():
    """a CellStartStep with writes_aux=True raises the sound speed in front of every step, on both runs: the user run is
    the built-in run again, and not the run without the hook"""
    q_ref, log_ref, _ = run_steps(layered_claw(False, hook=True), 10)
    q, log, forms = run_steps(layered_claw(True, hook=True), 10)
    q_plain, log_plain, _ = run_steps(layered_claw(True), 10)
    assert forms["one_kernel"] == 0
    assert len(log) >= 10 and log == log_ref and np.array_equal(q, q_ref)
    assert log != log_plain and not np.array_equal(q, q_plain)


def test_resident_run_with_a_gauge_writes_the_same_file(tmp_path):
    out = []
    for user in (False, True):
        claw = layered_claw(user)
        grid = claw.solution.state.grid
        grid.gauge_path = str(tmp_path / ("user" if user else "builtin")) + os.sep
        grid.add_gauges([((30 + 0.5) * grid.d[0], (12 + 0.5) * grid.d[1])])       # Grid.add_gauges: index = floor(x / d)
        assert grid.gauges == [[30, 12]]
        q, log, _ = run_steps(claw, 16, resident=True)
        for f in grid.gauge_files:
            f.close()
        files = [open(f.name, "rb").read() for f in grid.gauge_files]
        out.append((q, log, files))
    (q_ref, log_ref, files_ref), (q, log, files) = out
    assert len(files) == 1 and files[0].count(b"\n") == 16
    assert files == files_ref and log == log_ref and np.array_equal(q, q_ref)


def test_claw_solver_1d_colour_equation_equals_the_built_in_run():
    q_ref, log_ref, _ = run_steps(colour_claw(False), 10)
    q, log, _ = run_steps(colour_claw(True), 10)
    assert len(log) >= 10 and log == log_ref
    assert np.array_equal(q, q_ref) and not np.array_equal(q, colour_claw(True).solution.state.q)


def test_fast_mode_is_within_the_projects_gate_of_exact():
    """rtol 1e-12 of the exact run's largest value, the gate of the 'fast' arithmetic"""
    q_ref, _, _ = run_steps(layered_claw(True), 10)
    q, _, _ = run_steps(layered_claw(True, math='fast'), 10)
    print("fast against exact: max |diff| = %g, largest value %g" % (np.abs(q - q_ref).max(), np.abs(q_ref).max()))
    assert np.abs(q - q_ref).max() <= 1e-12 * np.abs(q_ref).max()
