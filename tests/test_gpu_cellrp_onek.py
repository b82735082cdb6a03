"""
GPU: user-written Riemann solvers in the ONE-KERNEL form of the dimension-split 2-D step (pyclaw.CellRiemann(...,
one_kernel=True), pcl_cellrp_compile_onek; classic_fused.hpp).  The library compiles step2ds_kernel
around the user's body, so a built-in solver restated as a body must give the built-in one-kernel run's bytes, every
mechanism built on that step (quiet tiles, tile lists, form trials, step ahead) must behave for it as for the built-in
solver, and any system must give what its own two passes give.

Equality is bit for bit -- q as 64-bit words, every dt and every Courant number -- wherever both runs are one-kernel
runs.  Against a two-pass run the sign of a zero is left out, as in tests/test_gpu_fused_step.py: a wavefront without a
jump hands its cells through as they are where the full solve computes q + 0, and the two forms cut the grid into
different wavefronts.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyclaw_amd as pyclaw
from apps import problems, psystem
from pyclaw_amd import _lib as L

import test_gpu_cellrp as G
import test_gpu_cellrp_aux as A
import test_gpu_cellrp_form as F
import test_gpu_quiet_tiles as Q
import test_gpu_step_ahead as SA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = pyclaw.BC
ACOUSTICS_PAR = [1.0, 4.0, 2.0, 2.0]         # rho, bulk, cc, zz


def bits(q):
    return np.ascontiguousarray(q).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_but_zero_signs(a, b):
    return a.shape == b.shape and np.array_equal(bits(a + 0.0), bits(b + 0.0))


def hexlog(log):
    return [(float(dt).hex(), float(c).hex()) for dt, c in log]


def one_kernel(claw):
    """the user solver of the claw, with the one-kernel step compiled around its body"""
    assert isinstance(claw.solver.rp, pyclaw.CellRiemann) and not claw.solver.rp.one_kernel
    claw.solver.rp.one_kernel = True
    return claw


def acoustics_claw(kind, math='exact'):
    """kind: 'builtin', 'user' (the plain body: two passes) or 'onek'"""
    claw = G.acoustics_claw(kind != 'builtin', math=math)
    return one_kernel(claw) if kind == 'onek' else claw


# ---- 1. basic equality ----------------------------------------------------------------------------------------------
def test_acoustics_equals_the_same_body_without_it_and_the_built_in_run():
    """61 x 59: two tiles by five, every tile on the frame, a ragged last tile in both directions; reflecting and outflow
    sides, variable dt, 10 steps"""
    q_ref, log_ref, forms_ref = G.run_steps(acoustics_claw('builtin'), 10)
    q_two, log_two, forms_two = G.run_steps(acoustics_claw('user'), 10)
    q, log, forms = G.run_steps(acoustics_claw('onek'), 10)
    print("forms: built-in %s, user %s, user one_kernel %s" % (forms_ref, forms_two, forms))
    assert forms["one_kernel"] >= 10 and forms["two_pass"] == 0
    assert forms_two["one_kernel"] == 0 and forms_ref["one_kernel"] >= 10
    assert len(log) >= 10 and hexlog(log) == hexlog(log_ref) == hexlog(log_two)
    assert same_bits(q, q_ref)                      # two one-kernel runs: no sign-of-zero normalisation
    assert same_but_zero_signs(q, q_two)
    assert not np.array_equal(q, acoustics_claw('builtin').solution.state.q)


# ---- 2. quiet tiles -------------------------------------------------------------------------------------------------
BUMP_SHAPE = (300, 84)          # five tiles by seven


def bump_claw(kind, steps=12, dt_variable=False, params=ACOUSTICS_PAR):
    """acoustics on 300 x 84 cells, exactly uniform (zero) outside a bump of radius 8 cells around cell (30, 18).  A step
    moves the disturbed region by at most two cells per sweep, so over 12 steps it stays within 8 + 48 cells of (30, 18):
    columns < 87, rows < 75 -- the tiles tx = 3 (columns 180..239), ty = 2..4 (rows 24..59) keep a quiet 3 x 3
    neighbourhood (columns 118.., tiles tx 2..4) throughout."""
    mx, my = BUMP_SHAPE
    solver = pyclaw.ClawSolver2D()
    solver.mwaves = 2
    solver.limiters = [4, 4]
    solver.dim_split = True
    solver.cfl_max, solver.cfl_desired = 0.5, 0.45
    solver.dt_variable = dt_variable
    for k in range(2):
        solver.bc_lower[k] = solver.bc_upper[k] = B.outflow
    grid = pyclaw.Grid([pyclaw.Dimension('x', 0.0, 3.0, mx), pyclaw.Dimension('y', 0.0, 0.84, my)])
    state = pyclaw.State(grid, 3)
    for key, v in zip(('rho', 'bulk', 'cc', 'zz'), params):
        state.aux_global[key] = v
    i, j = np.meshgrid(np.arange(mx), np.arange(my), indexing='ij')
    r = np.sqrt((i - 30.0) ** 2 + (j - 18.0) ** 2)
    state.q[...] = 0.0
    state.q[0] = np.where(r < 8.0, 1.0 + np.cos(np.pi * r / 8.0), 0.0)
    assert np.count_nonzero(state.q[0]) > 100 and not state.q[0, 41:, :].any() and not state.q[0, :, 29:].any()
    if kind == 'builtin':
        solver.rp = pyclaw.riemann.rp_acoustics_2d
    else:
        solver.rp = pyclaw.CellRiemann(problems.ACOUSTICS_2D_RP, 3, 2, 2, params=params, one_kernel=(kind == 'onek'))
    solver.dt_initial = 0.4 * 0.01 / params[2]
    return Q.controller(state, solver, steps * solver.dt_initial)


def test_quiet_tiles_skip_for_a_user_solver_as_for_the_built_in_one():
    on, off = Q.run_both(lambda: bump_claw('onek'))          # skipping on and off: identical bytes, the same step log
    ref_on, _ = Q.run_both(lambda: bump_claw('builtin'))
    assert len(on[3]) == 12
    assert on[3] == ref_on[3], (on[3], ref_on[3])           # (computed, skipped) after every step
    assert Q.skipped(on) > 0
    # the first launch computes all 35 tiles; every later one skips at least the three tiles of bump_claw's argument
    assert on[3][0] == (35, 0) and all(c + k == 35 and k >= 3 for c, k in on[3][1:]), on[3]
    assert on[2] == ref_on[2] and on[0] == ref_on[0]        # and the built-in run's log and bytes


# ---- 3. other systems -----------------------------------------------------------------------------------------------
def system_claw(name, kind):
    """a system on its small grid; kind: 'user' (two passes), 'onek', or 'builtin' where the library has the solver"""
    mx, my = {"shallow": (61, 59), "burgers": (73, 37), "scalars5": (73, 37), "euler5": (61, 59)}[name]
    grid = pyclaw.Grid([pyclaw.Dimension('x', -1.0, 1.0, mx), pyclaw.Dimension('y', -1.0, 1.0, my)])
    X, Y = grid.c_center
    bump = np.exp(-12.0 * ((X - 0.2) ** 2 + (Y + 0.1) ** 2))
    solver = pyclaw.ClawSolver2D()
    solver.dim_split = True
    solver.cfl_max, solver.cfl_desired = 0.5, 0.45
    bcs = [B.reflecting, B.outflow, B.outflow, B.reflecting]
    builtin = None
    if name == "shallow":
        meqn = mwaves = 3
        body, params, speed = problems.SHALLOW_2D_RP, [1.0], 1.5
        q = np.stack([1.0 + 0.5 * bump, 0.1 * bump, -0.05 * bump])
        builtin = pyclaw.riemann.rp_shallow_2d
    elif name == "burgers":
        meqn = mwaves = 1
        body, params, speed = problems.BURGERS_2D_RP, [], 1.25
        q = (np.sin(np.pi * X) * np.cos(np.pi * Y) + 0.25)[None]            # crosses zero: the transonic branch runs
        bcs = [B.periodic] * 4
    elif name == "scalars5":
        meqn = mwaves = 5
        body, params, speed = problems.SCALARS_2D_RP, [1.0, -0.5, 0.75, -1.25, 0.25], 1.25
        q = np.stack([bump * (k + 1) + 0.1 * k * np.sin(np.pi * (X + k * Y)) for k in range(5)])
        bcs = [B.periodic, B.periodic, B.outflow, B.outflow]
    else:       # EULER_3D_RP over ixy = 1, 2: the third momentum is carried along
        meqn, mwaves = 5, 3
        body, params, speed = problems.EULER_3D_RP, [1.4], 2.0
        rho, u, v, w, pr = 1.0 + 0.3 * bump, 0.1 * bump, -0.1 * bump, 0.05 + 0.0 * bump, 1.0 + 0.5 * bump
        q = np.stack([rho, rho * u, rho * v, rho * w, pr / 0.4 + 0.5 * rho * (u * u + v * v + w * w)])
    state = pyclaw.State(grid, meqn)
    state.q[...] = q
    if kind == 'builtin':
        state.aux_global['g'] = params[0]
        solver.rp = builtin
    else:
        solver.rp = pyclaw.CellRiemann(body, meqn, mwaves, 2, params=params, one_kernel=(kind == 'onek'))
    solver.mwaves = mwaves
    solver.limiters = [4] * mwaves
    for k in range(2):
        solver.bc_lower[k], solver.bc_upper[k] = bcs[2 * k], bcs[2 * k + 1]
    solver.dt_initial = 0.4 * min(grid.d) / speed
    claw = pyclaw.Controller()
    claw.solution = pyclaw.Solution(state)
    claw.solver = solver
    return claw


def check_against_its_two_passes(make, builtin=True, nsteps=10):
    """make(kind) -> claw.  The one-kernel run against the same body's two passes and, where there is one, against the
    built-in solver's run (which takes the one-kernel step: bit for bit)"""
    q_two, log_two, forms_two = G.run_steps(make('user'), nsteps)
    q, log, forms = G.run_steps(make('onek'), nsteps)
    print("forms: user %s, user one_kernel %s" % (forms_two, forms))
    assert forms["one_kernel"] >= nsteps and forms["two_pass"] == 0 and forms_two["one_kernel"] == 0
    assert len(log) >= nsteps and hexlog(log) == hexlog(log_two)
    assert np.isfinite(q).all() and same_but_zero_signs(q, q_two)
    assert not np.array_equal(q, make('user').solution.state.q)
    if builtin:
        q_ref, log_ref, forms_ref = G.run_steps(make('builtin'), nsteps)
        assert forms_ref["one_kernel"] >= nsteps
        assert hexlog(log) == hexlog(log_ref) and same_bits(q, q_ref)


@pytest.mark.parametrize("name", ["shallow", "burgers", "scalars5", "euler5"])
def test_other_systems_equal_their_two_passes(name):
    check_against_its_two_passes(lambda kind: system_claw(name, kind), builtin=(name == "shallow"))


def user_kind(make_user, make_builtin):
    def make(kind):
        if kind == 'builtin':
            return make_builtin()
        claw = make_user()
        return one_kernel(claw) if kind == 'onek' else claw
    return make


def test_vc_acoustics_in_a_layered_medium():
    """aux=(0, 1): the one-kernel step over the whole block with the two planes staged next to q"""
    check_against_its_two_passes(user_kind(lambda: A.layered_claw(True), lambda: A.layered_claw(False)))


def test_acoustics_with_a_capacity_function():
    check_against_its_two_passes(user_kind(lambda: F.capa_acoustics_claw(True, 1), lambda: F.capa_acoustics_claw(False, 1)))


@pytest.mark.parametrize("linearity", [1, 2])
def test_psystem_fwave_with_its_aux_list(linearity):
    """fwave=True: the FWAVE instantiation, in which no wavefront takes the shortcut"""
    check_against_its_two_passes(user_kind(lambda: F.psystem_claw(True, "classic", linearity),
                                           lambda: F.psystem_claw(False, "classic", linearity)))


# ---- 4. form trials -------------------------------------------------------------------------------------------------
TWO_PASS_RUN = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_cellrp as G
import test_gpu_cellrp_onek as T
q, log, forms = G.run_steps(T.acoustics_claw('onek'), 80)
print("RESULT " + json.dumps({"q": T.bits(q + 0.0).ravel().tolist(), "log": T.hexlog(log), "forms": forms}))
"""


def test_form_trials_run_both_forms_and_change_nothing():
    """80 steps at 61 x 59 pass the trial steps 64..71 and the verdict: both forms ran; the result is that of the same
    solver held to two passes (PCL_TUNE_FUSED_STEP=0 is read once per process: a child)"""
    q, log, forms = G.run_steps(acoustics_claw('onek'), 80)
    print("forms: %s" % (forms,))
    assert forms["one_kernel"] >= 64 and forms["two_pass"] >= 3 and forms["one_kernel"] + forms["two_pass"] == len(log)
    env = dict(os.environ, PCL_TUNE_FUSED_STEP="0")
    p = subprocess.run([sys.executable, "-c", TWO_PASS_RUN % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    ref = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert ref["forms"]["one_kernel"] == 0 and ref["forms"]["two_pass"] == len(log)
    assert hexlog(log) == [tuple(e) for e in ref["log"]]
    assert np.array_equal(bits(q + 0.0).ravel(), np.array(ref["q"], dtype=np.uint64))


# ---- 5. resident mode with device boundary conditions: step ahead -------------------------------------------------
def bump_run(kind, armed, script, params=ACOUSTICS_PAR):
    r = SA.Run(lambda: bump_claw(kind, dt_variable=True, params=params), armed, rule=1)
    script(r)
    q = r.q_bytes().copy()
    return r.close() + (q,)     # (hash, finite, step count, log, (enqueued, adopted, dropped), the final interior q)


def test_steps_enqueued_ahead_are_adopted_as_for_the_built_in_solver():
    on = bump_run('onek', True, SA.steady(40))
    off = bump_run('onek', False, SA.steady(40))
    ref = bump_run('builtin', True, SA.steady(40))
    print("step ahead (enqueued, adopted, dropped): user %s, built-in %s" % (on[4], ref[4]))
    assert on[1] and on[:4] == off[:4]                  # armed or not: the same bytes, steps and log
    assert on[4] == ref[4] and on[4][1] >= 30, (on[4], ref[4])
    assert on[:4] == ref[:4]                            # the built-in run's bytes (two one-kernel runs: every bit)


def test_params_reassigned_behind_a_step_drop_the_step_enqueued_ahead():
    """the sound speed changes behind step 5: the pending step was computed with the old one and is dropped, and no
    Courant maximum cached for a skipped tile -- the old body's speeds -- survives"""
    new = [1.0, 2.25, 1.5, 1.5]
    seen = {}

    def script(r):
        for k in range(16):
            if k == 5:
                before = r.stats() if r.armed else None         # (drops the pending step itself: counted below)
                r.solver.rp.params = new
                r.solver.rp.send_params(r.solver)
                seen["before"] = before
            r.step()
            if k == 5 and r.armed:
                seen["skip"] = r.skip_stats()
        if r.armed:
            seen["after"] = r.stats()
    on = bump_run('onek', True, script)
    assert seen["skip"][1] == 0 and seen["skip"][0] == 35, seen         # the step behind the change computed every tile
    assert seen["after"][2] >= seen["before"][2] + 1, seen
    off = bump_run('onek', False, script)
    two = bump_run('user', False, script)
    assert on[1] and on[:4] == off[:4]
    # the two-pass run with the same change: the log bit for bit, q up to the sign of a zero
    assert on[2:4] == two[2:4]
    assert same_but_zero_signs(on[5], two[5]) and same_bits(on[5], off[5])
    cfls = [float.fromhex(e[3]) / float.fromhex(e[2]) for e in on[3] if e[0] == "bc_step"]
    assert abs(cfls[5] / cfls[4] - 0.75) < 1e-12, cfls[3:7]            # cc 2 -> 1.5 shows in the very next Courant number


def test_params_reassigned_give_the_two_pass_bytes():
    """(the same through the public interface, where the final state can be compared up to the sign of a zero)"""
    new = [1.0, 2.25, 1.5, 1.5]

    def change(c):
        c.solver.rp.params = new
    q_two, log_two, _ = G.run_steps(bump_claw('user', dt_variable=True), 12, change=(5, change), resident=True)
    q, log, forms = G.run_steps(bump_claw('onek', dt_variable=True), 12, change=(5, change), resident=True)
    assert forms["one_kernel"] >= 12 and forms["two_pass"] == 0
    assert hexlog(log) == hexlog(log_two) and log[5] != log[4]
    assert same_but_zero_signs(q, q_two)


# ---- 6. re-attach ---------------------------------------------------------------------------------------------------
def test_another_body_attached_between_two_steps_computes_every_tile():
    """the second body is the first one with another sound speed written into it: the same module would keep the quiet
    tiles' cached speeds, another one must not"""
    slow = "const double cc_ = 1.5, zz_ = 1.5;\n" + problems.ACOUSTICS_2D_RP.replace("p[2]", "cc_").replace("p[3]", "zz_")
    assert "cc_" in slow and slow.count("p[") == 0
    seen = {}

    def script_for(onek):
        def script(r):
            other = pyclaw.CellRiemann(slow, 3, 2, 2, one_kernel=onek).compile()
            for k in range(12):
                if k == 6:
                    if onek:
                        seen["before"] = r.skip_stats()
                    L.check(r.L.pcl_cellrp_attach(r.h, other._rp))
                r.step()
                if k == 6 and onek:
                    seen["behind"] = r.skip_stats()
            if onek:
                seen["end"] = r.skip_stats()
        return script
    on = bump_run('onek', False, script_for(True))
    two = bump_run('user', False, script_for(False))
    assert seen["before"][1] > 0 and seen["behind"] == (35, 0) and seen["end"][1] > 0, seen
    # the two-pass run with the same attach: the step count and the log bit for bit, q up to the sign of a zero
    assert on[1] and on[2:4] == two[2:4]
    assert same_but_zero_signs(on[5], two[5])
    # and the second body is in it: not the run that keeps the first one
    kept = bump_run('onek', False, SA.steady(12))
    assert not same_but_zero_signs(on[5], kept[5])
    cfls = [float.fromhex(e[3]) / float.fromhex(e[2]) for e in on[3] if e[0] == "bc_step"]
    assert abs(cfls[6] / cfls[5] - 0.75) < 1e-12, cfls[4:8]


# ---- 7. math modes --------------------------------------------------------------------------------------------------
def test_strict_equals_its_own_two_passes():
    q_two, log_two, _ = G.run_steps(acoustics_claw('user', math='strict'), 10)
    q, log, forms = G.run_steps(acoustics_claw('onek', math='strict'), 10)
    assert forms["one_kernel"] >= 10 and forms["two_pass"] == 0
    assert hexlog(log) == hexlog(log_two) and same_but_zero_signs(q, q_two)


def test_fast_mode_is_within_the_projects_gate_of_exact():
    """rtol 1e-12 of the exact run's largest value, the gate of the 'fast' arithmetic"""
    q_ref, _, _ = G.run_steps(acoustics_claw('onek'), 10)
    q, _, forms = G.run_steps(acoustics_claw('onek', math='fast'), 10)
    print("fast against exact: max |diff| = %g" % np.abs(q - q_ref).max())
    assert forms["one_kernel"] >= 10
    assert np.abs(q - q_ref).max() <= 1e-12 * np.abs(q_ref).max()


# ---- 8. refused or left alone ---------------------------------------------------------------------------------------
def test_three_ghost_layers_run_the_two_passes():
    def make(kind):
        claw = acoustics_claw(kind)
        claw.solver.mbc = 3
        return claw
    q_two, log_two, _ = G.run_steps(make('user'), 6)
    q, log, forms = G.run_steps(make('onek'), 6)
    assert forms["one_kernel"] == 0 and forms["two_pass"] >= 6
    assert hexlog(log) == hexlog(log_two) and same_bits(q, q_two)


def test_an_unsplit_solver_never_uses_the_extra_kernel():
    def make(onek):
        claw = problems.acoustics2D(pyclaw, mx=61, my=59, run=False, dim_split=0, user_rp=True)
        claw.solver.rp.one_kernel = onek
        return claw
    q_ref, log_ref, _ = G.run_steps(make(False), 6)
    q, log, forms = G.run_steps(make(True), 6)
    assert not forms or forms["one_kernel"] == 0
    assert hexlog(log) == hexlog(log_ref) and same_bits(q, q_ref)


def test_more_than_one_block_and_a_missing_aux_array_are_refused_as_before():
    hd = G.Handle(problems.ACOUSTICS_2D_RP, 3, 2, (61, 59), (0.1, 0.1), 2, 2, [4, 4], ACOUSTICS_PAR)
    try:
        hd.rp.one_kernel = True
        hd.rp.compile()
        hd.attach()
        nbr = np.full(8, -1, dtype=np.int32)
        assert L.lib().pcl_comm_init(hd.h, 1, 0, C.create_string_buffer(128), L.i(nbr)) == L.EINVAL
        assert b"one block" in L.lib().pcl_last_error()
        assert L.lib().pcl_fuse_source(hd.h, 1, L.d(np.array([0.4, 2.0])), 2) == L.EINVAL
    finally:
        hd.close()
    hd = A.Handle(problems.VC_ACOUSTICS_2D_RP, 3, 2, (61, 59), (0.1, 0.1), 2, 2, [4, 4], 2, (0, 1))
    try:
        hd.rp.one_kernel = True
        hd.rp.compile()
        hd.attach()
        q0 = np.asfortranarray(np.ones((3, 65, 63)))
        cfl = C.c_double()
        L.check(L.lib().pcl_put_q(hd.h, L.d(q0), 1))
        assert L.lib().pcl_step_hyperbolic(hd.h, 0.01, C.cast(C.byref(cfl), L.dp)) == L.EINVAL
        assert b"reads aux arrays and there are none" in L.lib().pcl_last_error()
        # and with it the step runs (the one-kernel step writes interior cells alone)
        out, _ = hd.put_aux(np.asfortranarray(np.ones((2, 65, 63)))).step(q0, 0.01)
        assert np.array_equal(out[:, 2:-2, 2:-2], q0[:, 2:-2, 2:-2])
    finally:
        hd.close()
