"""
GPU: the device gauge log (pcl_gauge_log, include/pyclaw_amd.h) changes nothing but the time.  Every case
runs the same problem twice, with solver.gauge_log = False (the gather after every step, pcl_get_cells) and with True (every
step records its gauge cells, the lines are written when the log is read), and the gauge files must agree byte for byte.
Every case also checks that the device recorded exactly the lines the logged path wrote: recorded - popped of
pcl_gauge_log_stats against the calls of write_gauge_values that were on the logged path.
"""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import pyclaw_amd as pyclaw
from pyclaw_amd import _lib
from apps import problems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = pyclaw.BC


def cell_coords(grid, cells):
    """coordinates that Grid.add_gauges maps to these cells (its rule: index = floor(x / d))"""
    return [tuple((i + 0.5) * d for i, d in zip(c, grid.d)) for c in cells]


def log_stats(solver):
    a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.lib().pcl_gauge_log_stats(solver._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return {"recorded": a.value, "popped": b.value, "reads": c.value}


def instrument(claw, cells, path, log, capacity=None):
    """gauges at `cells`, files under `path`; counts the lines of the logged path and keeps the log's totals from just
    before the handle goes"""
    solver, grid = claw.solver, claw.solution.state.grid
    grid.gauge_path = str(path) + os.sep
    grid.add_gauges(cell_coords(grid, cells))
    assert grid.gauges == [list(c) for c in cells]
    solver.gauge_log = log
    if capacity is not None:
        solver.gauge_log_capacity = capacity
    seen = {"logged": 0, "direct": 0, "stats": None, "armed": False, "since_arming": 0, "key": None}
    write, teardown = solver.write_gauge_values, solver.teardown

    def counted(solution):
        on = solver._glog_on
        seen["armed"] = seen["armed"] or solver._glog_key is not None
        if on and solver._glog_key != seen["key"]:       # armed (again) since the last line: the totals started afresh
            seen["key"], seen["since_arming"] = solver._glog_key, 0
        if not on:
            seen["key"] = None
        write(solution)
        seen["logged" if on else "direct"] += 1
        seen["since_arming"] += int(on)

    def kept():
        seen["stats"] = log_stats(solver)
        teardown()
        del solver.write_gauge_values, solver.teardown       # (the solver no longer refers to itself through the two)
    solver.write_gauge_values, solver.teardown = counted, kept
    return seen


def files_of(claw):
    return [open(f.name, "rb").read() for f in claw.solution.state.grid.gauge_files]


def both(make, cells, tmp_path, capacity=None, logged=True):
    """the run with the gather and the run with the log: identical files; returns (claw, files, seen) of the logged run"""
    out = []
    for log in (False, True):
        claw = make()
        seen = instrument(claw, cells, tmp_path / ("log" if log else "gather"), log, capacity)
        claw.run()
        out.append((claw, files_of(claw), seen))
    (_, ref, ref_seen), (claw, got, seen) = out
    assert all(len(f) > 0 for f in ref) and len(ref) == len(cells)
    assert got == ref
    assert ref_seen["logged"] == 0 and ref_seen["stats"]["recorded"] == 0 and not ref_seen["armed"]
    st = seen["stats"]
    print("gauge log: logged lines %d, direct %d, stats %s" % (seen["logged"], seen["direct"], st))
    if logged == "mixed":       # the run went from one path to the other and back: the totals are those of the last arming
        assert seen["logged"] > 0 and seen["direct"] > 1 and st["recorded"] - st["popped"] == seen["since_arming"] > 0
        return claw, got, seen
    assert st["recorded"] - st["popped"] == seen["logged"]
    if logged:
        assert seen["logged"] > 0 and seen["direct"] == 1          # Controller.run's initial line alone
        assert all(f.count(b"\n") == seen["logged"] + 1 for f in got)
    else:
        assert seen["logged"] == 0 and st["recorded"] == 0 and not seen["armed"]
    return claw, got, seen


def test_entry_points_exist():
    L = _lib.lib()
    for name in ("pcl_gauge_log", "pcl_gauge_log_read", "pcl_gauge_log_stats", "pcl_gauge_log_trace"):
        assert hasattr(L, name)
    assert pyclaw.ClawSolver2D().gauge_log is True and pyclaw.ClawSolver2D().gauge_log_capacity == 1024


# ---- 1: Controller.run, corner cells and an interior cell ------------------------------------------------------------------
def test_controller_run_corner_and_interior_cells(tmp_path):
    cells = [(0, 0), (59, 49), (7, 12)]
    claw, files, seen = both(lambda: problems.acoustics2D(pyclaw, mx=60, my=50, nout=3, run=False), cells, tmp_path)
    for g, text in zip(cells, files):
        rows = [[float(v) for v in line.split()] for line in text.decode().splitlines()]
        times = [r[0] for r in rows]
        assert times[0] == 0.0 and all(b > a for a, b in zip(times, times[1:]))
        assert len(rows) == claw.nout * claw.solver.status['numsteps'] + 1     # status counts the last evolve call
        series = {r[0]: r[1:] for r in rows}
        for kept in claw.frames:
            assert series[kept.t] == list(kept.state.q[:, g[0], g[1]])
    assert seen["stats"]["reads"] == claw.nout


# ---- 2: flushes in the middle of a run -------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [3, 1])
def test_small_capacity_flushes_mid_run(tmp_path, capacity):
    claw, files, seen = both(lambda: problems.acoustics2D(pyclaw, mx=60, my=50, nout=1, run=False), [(3, 4), (59, 0)],
                             tmp_path, capacity=capacity)
    steps = claw.solver.status['numsteps']
    assert steps > 10 and seen["logged"] == steps
    assert seen["stats"]["reads"] >= steps // capacity


# ---- 3: rejected steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook", [False, True])
def test_rejected_steps_leave_no_record(tmp_path, hook):
    """a dt_initial far above the stable one: the first step is rejected.  Without a hook the undo is the pointer swap
    (pcl_undo_step); a CellStartStep makes it the copied backup (pcl_backup / pcl_restore)"""
    def make():
        claw = problems.acoustics2D(pyclaw, mx=60, my=50, nout=2, tfinal=0.06, run=False)
        claw.solver.dt_initial = 0.05            # Courant number about 3 against cfl_max 0.5
        if hook:
            claw.solver.start_step = pyclaw.CellStartStep("q[0] = q[0] - c.dt * p[0] * q[0];", params=[0.5])
        return claw
    claw, files, seen = both(make, [(0, 49), (30, 25)], tmp_path)
    assert claw.solver._pre_step_modifies_q() == hook
    assert seen["stats"]["popped"] >= 1


# ---- 4: aux ----------------------------------------------------------------------------------------------------------------
def vc_acoustics(start_step=None):
    claw = problems.acoustics2D(pyclaw, mx=60, my=50, nout=2, tfinal=0.06, run=False)
    old = claw.solution.state
    state = pyclaw.State(old.grid, 3, 2)
    state.q[...] = old.q
    X = old.grid.x.center[:, None] + 0.0 * old.grid.y.center[None, :]
    state.aux[0] = old.aux_global['zz'] * (1.0 + 0.25 * X)
    state.aux[1] = old.aux_global['cc']
    claw.solution = pyclaw.Solution(state)
    claw.solver.rp = pyclaw.riemann.rp_vc_acoustics_2d
    for k in range(2):
        claw.solver.aux_bc_lower[k] = claw.solver.aux_bc_upper[k] = B.outflow
    claw.solver.compute_gauge_values = lambda q, aux: [q[0], aux[0] * q[1], aux[1], aux[0]]
    claw.solver.start_step = start_step
    return claw


def test_aux_in_compute_gauge_values(tmp_path):
    claw, files, seen = both(vc_acoustics, [(0, 0), (59, 49), (31, 17)], tmp_path)
    zz = [float(line.split()[4]) for line in files[2].decode().splitlines()]
    assert len(set(zz)) == 1 and zz[0] == claw.solution.state.aux[0, 31, 17]


def test_aux_written_by_a_start_step_is_recorded_per_step(tmp_path):
    # the impedance grows a little every step (the sound speed, and with it the Courant number, stays)
    hook = lambda: pyclaw.CellStartStep("aux[0] = aux[0] * (1.0 + 0.5 * c.dt);", writes_aux=True)
    claw, files, seen = both(lambda: vc_acoustics(hook()), [(0, 0), (31, 17)], tmp_path)
    zz = [float(line.split()[4]) for line in files[1].decode().splitlines()]
    assert all(b > a for a, b in zip(zz, zz[1:])) and len(zz) == seen["logged"] + 1


# ---- 5: the other steps: unsplit 2-D, 1-D, 3-D -----------------------------------------------------------------------------
def test_unsplit_2d(tmp_path):
    both(lambda: problems.acoustics2D(pyclaw, mx=60, my=50, nout=2, tfinal=0.06, dim_split=0, run=False),
         [(0, 0), (59, 49), (7, 12)], tmp_path)


def acoustics1d(mx=100):
    solver = pyclaw.ClawSolver1D()
    solver.rp = pyclaw.riemann.rp_acoustics_1d
    state = pyclaw.State(pyclaw.Grid(pyclaw.Dimension('x', 0.0, 1.0, mx)), 2)
    state.aux_global.update(rho=1.0, bulk=1.0, zz=1.0, cc=1.0)
    xc = state.grid.x.center
    state.q[0, :] = np.exp(-100 * (xc - 0.75) ** 2)
    state.q[1, :] = 0.
    solver.mwaves = 2
    solver.limiters = [4] * 2
    solver.dt_initial = state.grid.d[0] * 0.1
    solver.bc_lower[0] = solver.bc_upper[0] = B.periodic
    claw = pyclaw.Controller()
    claw.nout, claw.tfinal = 2, 0.4
    claw.solution, claw.solver = pyclaw.Solution(state), solver
    return claw


def test_1d_first_and_last_cell(tmp_path):
    both(acoustics1d, [(0,), (99,)], tmp_path)


@pytest.mark.parametrize("kind", ["hom", "het"])
def test_3d_split_and_unsplit(tmp_path, kind):
    claw, files, seen = both(lambda: problems.acoustics3D(pyclaw, test=kind, mx=12, my=10, mz=8, tfinal=0.3, nout=1, run=False),
                             [(0, 0, 0), (11, 9, 7), (5, 2, 6)], tmp_path)
    assert claw.solver.dim_split == (kind == "hom")
    last = [float(v) for v in files[2].decode().splitlines()[-1].split()]
    assert last[1:] == list(claw.frames[-1].state.q[:, 5, 2, 6])


# ---- 6: resident mode with step-ahead ----------------------------------------------------------------------------------------
def test_resident_mode_costs_no_adoption(tmp_path):
    """the one-kernel step of a resident run, the next step enqueued ahead: the record goes in front of it.  The log run
    adopts what the run without gauges adopts, call by call (pcl_step_ahead_stats between the calls is no read-only call:
    every run drops what is pending at the same places)"""
    cells = [(0, 0), (959, 479), (300, 100), (480, 7)]

    def run(gauges, log):
        claw = problems.shockbubble(pyclaw, mx=960, my=480, tfinal=1.0, device_callbacks=True, dt_initial=0.005 * 160 / 960,
                                    run=False)
        solver, solution = claw.solver, claw.solution
        seen = instrument(claw, cells if gauges else [], tmp_path / ("g%d%d" % (gauges, log)), log)
        solver.setup(solution)
        solver.dt = solver.dt_initial
        solver.begin_resident(solution)
        counts, steps = [], 0
        for k in range(3):
            steps += solver.evolve_to_time(solution, 0.004 * (k + 1))['numsteps']
            a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
            _lib.check(_lib.lib().pcl_step_ahead_stats(solver._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
            counts.append((a.value, b.value, c.value))
        assert solver._step_ahead_sent[0] == 1 and solver._src_fused
        solver.end_resident(solution)
        q = solution.state.q.copy()
        solver.teardown()
        forms = solver.status["step_forms"]
        for f in solution.state.grid.gauge_files:
            f.close()
        return counts, steps, q, files_of(claw), seen, forms

    plain = run(False, False)
    gather = run(True, False)
    logged = run(True, True)
    print("step ahead (enqueued, adopted, dropped) per call: no gauges %s, gather %s, log %s; forms %s"
          % (plain[0], gather[0], logged[0], logged[5]))
    assert logged[5]["one_kernel"] > 0 and plain[0][-1][1] > 0          # the one-kernel form, with adopted steps
    assert logged[0] == plain[0]
    assert logged[3] == gather[3] and len(logged[3]) == len(cells)
    assert np.array_equal(logged[2], plain[2]) and logged[1] == plain[1]
    st = logged[4]["stats"]
    assert logged[4]["logged"] == logged[1] and st["recorded"] - st["popped"] == logged[1] and st["reads"] == 3
    assert all(f.count(b"\n") == logged[1] for f in logged[3])


# ---- 7: what is not logged ---------------------------------------------------------------------------------------------------
def test_python_strang_source_keeps_the_gather(tmp_path):
    def make():
        claw = problems.shockbubble(pyclaw, mx=40, my=10, tfinal=0.02, run=False)
        claw.solver.src_split = 2
        return claw
    both(make, [(0, 0), (39, 9)], tmp_path, logged=False)


def test_sharpclaw_keeps_the_gather(tmp_path):
    both(lambda: problems.acoustics2D(pyclaw, mx=37, my=21, tfinal=0.03, nout=1, solver_type='sharpclaw',
                                      time_integrator='SSP33', run=False), [(0, 0), (36, 20)], tmp_path, logged=False)


def test_environment_switch_keeps_the_gather(tmp_path, monkeypatch):
    monkeypatch.setenv("PCL_GAUGE_LOG", "0")
    both(lambda: problems.acoustics2D(pyclaw, mx=60, my=50, nout=2, tfinal=0.06, run=False), [(0, 0), (59, 49)], tmp_path,
         logged=False)


def test_switch_of_paths_inside_a_call_keeps_the_order_of_lines(tmp_path):
    """a Python source term appears behind the hyperbolic step in the middle of an evolve_to_time call and goes again:
    step() decides afresh, the records held are written before the direct path writes its first line, and the log is armed
    again afterwards"""
    def make():
        claw = problems.acoustics2D(pyclaw, mx=60, my=50, nout=1, run=False)
        calls = [0]
        noop = lambda solver, state, dt: None

        def hook(solver, solution):
            calls[0] += 1
            if calls[0] == 5:
                solver.step_src = noop
            if calls[0] == 10:
                solver.step_src = None
        claw.solver.start_step = hook
        return claw
    claw, files, seen = both(make, [(0, 0), (59, 49), (7, 12)], tmp_path, logged="mixed")
    assert claw.solver.status['numsteps'] > 12
    for text in files:
        times = [float(line.split()[0]) for line in text.decode().splitlines()]
        assert len(times) == seen["logged"] + seen["direct"] and all(b > a for a, b in zip(times, times[1:]))


def test_changed_capacity_arms_again(tmp_path):
    cells = [(0, 0), (59, 49)]

    def run(log):
        claw = problems.acoustics2D(pyclaw, mx=60, my=50, run=False)
        solver, solution = claw.solver, claw.solution
        seen = instrument(claw, cells, tmp_path / ("log" if log else "gather"), log)
        solver.setup(solution)
        solver.dt = solver.dt_initial
        solver.evolve_to_time(solution, 0.03)
        keys = [solver._glog_key]
        solver.gauge_log_capacity = 2
        steps = solver.evolve_to_time(solution, 0.06)['numsteps']
        keys.append(solver._glog_key)
        solver.teardown()
        for f in solution.state.grid.gauge_files:
            f.close()
        return files_of(claw), seen, keys, steps
    ref, _, ref_keys, _ = run(False)
    got, seen, keys, steps = run(True)
    assert got == ref and ref_keys == [None, None]
    assert keys[0][1] == 1024 and keys[1][1] == 2 and keys[0][0] == keys[1][0] == ((0, 0), (59, 49))
    st = seen["stats"]
    assert st["recorded"] - st["popped"] == seen["since_arming"] == steps > 2 and st["reads"] >= steps // 2


def test_exception_in_the_loop_is_not_masked_by_the_flush(tmp_path):
    """fixed dt, and a hook that makes the fourth step ten times too long: evolve_to_time gives up behind a step that was
    recorded and never accepted.  The three accepted lines are written, and the exception is the loop's own"""
    cells = [(0, 0), (30, 25)]

    def run(log):
        claw = problems.acoustics2D(pyclaw, mx=60, my=50, run=False)
        solver, solution = claw.solver, claw.solution
        seen = instrument(claw, cells, tmp_path / ("log" if log else "gather"), log)
        solver.dt_variable = False
        calls = [0]

        def hook(solver, solution):
            calls[0] += 1
            if calls[0] == 4:
                solver.dt = 10 * solver.dt
        solver.start_step = hook
        solver.setup(solution)
        solver.dt = 0.005                           # Courant number 0.3 against cfl_max 0.5
        with pytest.raises(Exception, match="CFL too large"):
            solver.evolve_to_time(solution, 0.05)
        solver.teardown()
        for f in solution.state.grid.gauge_files:
            f.close()
        return files_of(claw), seen
    ref, _ = run(False)
    got, seen = run(True)
    assert got == ref and all(f.count(b"\n") == 3 for f in got)
    assert seen["logged"] == 3 and seen["stats"] == {"recorded": 4, "popped": 0, "reads": 1}


# ---- 8: two ranks on one GPU ---------------------------------------------------------------------------------------------------
def test_two_ranks_log_their_own_gauges(tmp_path):
    """each rank logs the gauges of its block (one of them in the column or row next to the cut); together the files are
    the serial run's"""
    import gauge_log_mp_worker as W
    serial = W.make()
    instrument(serial, W.CELLS, tmp_path / "serial", False)
    serial.run()
    ref = {os.path.basename(f.name): open(f.name, "rb").read() for f in serial.solution.state.grid.gauge_files}
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   PCL_HALO_TRANSPORT="host", PCL_FORCE_DEVICE="0", TORCHELASTIC_RUN_ID="gl%d" % port)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "gauge_log_mp_worker.py"),
                                       str(tmp_path / "ranks")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert [p.returncode for p in procs] == [0, 0], "\n----\n".join(o[-1500:] for o in outs)
    owned = [int(line.split()[-1]) for o in outs for line in o.splitlines() if line.startswith("GAUGES ")]
    assert len(owned) == 2 and min(owned) >= 1 and sum(owned) == len(W.CELLS), outs
    got = {name: open(os.path.join(str(tmp_path / "ranks"), name), "rb").read() for name in os.listdir(str(tmp_path / "ranks"))}
    assert got == ref


# ---- 9: refusals, and the records themselves through the raw ABI ---------------------------------------------------------------
def raw_solver(claw):
    solver, solution = claw.solver, claw.solution
    solver.setup(solution)
    solver._push(solution.state)
    return solver


def test_refusals_and_raw_records():
    L = _lib.lib()
    claw = problems.acoustics2D(pyclaw, mx=60, my=50, nout=1, run=False)
    solver = raw_solver(claw)
    h = solver._h
    ij = lambda *cells: np.array(cells, dtype=np.int32)
    for bad in ((60, 0), (0, 50), (-1, 3), (3, -1)):
        assert L.pcl_gauge_log(h, 2, _lib.i(ij((1, 1), bad)), 4) == _lib.EINVAL
        assert b"outside the interior" in L.pcl_last_error()
    assert L.pcl_gauge_log(h, 1, _lib.i(ij((1, 1))), 0) == _lib.EINVAL
    n = ctypes.c_int(-1)
    out = np.full((4, 3, 3), np.nan)
    assert L.pcl_gauge_log_read(h, 4, _lib.d(out), ctypes.byref(n)) == _lib.ESTATE          # not armed
    cells = ij((0, 0), (59, 49), (7, 12))
    _lib.check(L.pcl_gauge_log(h, 3, _lib.i(cells), 2))
    spec = solver._device_bc_spec(claw.solution.state)
    cfl, dt = ctypes.c_double(0.0), float(solver.dt_initial)
    step = lambda: L.pcl_bc_step(h, spec[2], spec[3], dt, ctypes.cast(ctypes.byref(cfl), _lib.dp))
    want = []
    for _ in range(2):
        assert step() == 0
        qv = np.empty((3, 3))
        _lib.check(L.pcl_get_cells(h, 3, _lib.i(cells), _lib.d(qv), None))
        want.append(qv)
    steps = ctypes.c_long()
    _lib.check(L.pcl_step_count(h, ctypes.byref(steps)))
    assert step() == _lib.ESTATE and b"gauge log is full" in L.pcl_last_error()             # an error return, nothing launched
    after = ctypes.c_long()
    _lib.check(L.pcl_step_count(h, ctypes.byref(after)))
    assert after.value == steps.value == 2 and log_stats(solver) == {"recorded": 2, "popped": 0, "reads": 0}
    assert L.pcl_gauge_log_read(h, 1, _lib.d(out), ctypes.byref(n)) == _lib.EINVAL and n.value == -1
    assert log_stats(solver)["reads"] == 0
    _lib.check(L.pcl_gauge_log_read(h, 4, _lib.d(out), ctypes.byref(n)))
    assert n.value == 2 and np.array_equal(out[:2], np.array(want)) and np.isnan(out[2:]).all()
    # room again; a rejected step's record goes with it (pointer-swap undo), the retake writes the same slot
    assert step() == 0
    _lib.check(L.pcl_undo_step(h))
    assert step() == 0 and log_stats(solver) == {"recorded": 4, "popped": 1, "reads": 1}
    _lib.check(L.pcl_gauge_log_read(h, 4, _lib.d(out), ctypes.byref(n)))
    assert n.value == 1
    qv = np.empty((3, 3))
    _lib.check(L.pcl_get_cells(h, 3, _lib.i(cells), _lib.d(qv), None))
    assert np.array_equal(out[0], qv)
    _lib.check(L.pcl_gauge_log(h, 0, None, 0))                                                # disarmed: steps record nothing
    assert step() == 0 and log_stats(solver) == {"recorded": 0, "popped": 0, "reads": 0}
    solver.teardown()
    # a SharpClaw handle
    sharp = problems.acoustics2D(pyclaw, mx=37, my=21, tfinal=0.03, nout=1, solver_type='sharpclaw', run=False)
    s2 = raw_solver(sharp)
    assert L.pcl_gauge_log(s2._h, 1, _lib.i(ij((1, 1))), 4) == _lib.ESTATE
    s2.teardown()
