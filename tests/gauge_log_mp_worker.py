"""
Worker for tests/test_gpu_gauge_log.py: one of N processes that share ONE GPU (PCL_FORCE_DEVICE=0, host-staged wire, like
tests/mp_gpu_worker.py) and run a decomposed dimension-split acoustics problem with gauges.  Every rank logs the gauges
Grid.add_gauges gave its block on the device (pcl_gauge_log) and writes their files into the directory named on the command
line; nothing is exchanged.  The test compares the files of all ranks with the serial run's.

  python tests/gauge_log_mp_worker.py <gauge directory>     with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyclaw_amd as pyclaw                  # noqa: E402
from pyclaw_amd import _lib, parallel       # noqa: E402
from apps import problems                   # noqa: E402

MX, MY = 90, 80
# two halves, whichever way the grid is cut: cells on both sides of the middle column and of the middle row
CELLS = [(44, 10), (45, 10), (10, 39), (10, 40)]


def make():
    return problems.acoustics2D(pyclaw, mx=MX, my=MY, tfinal=0.06, nout=2, run=False)


def main():
    parallel.init()
    claw = make()
    solver, grid = claw.solver, claw.solution.state.grid
    grid.gauge_path = sys.argv[1] + os.sep
    grid.add_gauges([tuple((i + 0.5) * d for i, d in zip(c, grid.d)) for c in CELLS])
    seen = {"logged": 0, "stats": None}
    write, teardown = solver.write_gauge_values, solver.teardown

    def counted(solution):
        on = solver._glog_on
        write(solution)
        seen["logged"] += int(on)

    def kept():
        a, b, c = ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
        _lib.check(_lib.lib().pcl_gauge_log_stats(solver._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        seen["stats"] = (a.value, b.value, c.value)
        teardown()
    solver.write_gauge_values, solver.teardown = counted, kept
    claw.run()
    ok = 0
    if grid.gauges:
        rec, pop, reads = seen["stats"]
        if not (seen["logged"] > 0 and rec - pop == seen["logged"] and reads >= claw.nout):
            print("rank %d: logged lines %d, stats %s" % (parallel.rank(), seen["logged"], seen["stats"]))
            ok = 3
    print("GAUGES rank %d owns %d" % (parallel.rank(), len(grid.gauges)))
    parallel.barrier()
    parallel.shutdown()
    sys.exit(ok)


if __name__ == "__main__":
    main()
