"""
Worker for tests/test_gpu_cellbc.py: one of N processes that share ONE GPU (PCL_FORCE_DEVICE=0, host-staged halo wire,
as tests/cellfn_mp_worker.py) and run a boundary-condition cell function (pyclaw.CellBC) on a grid cut in y
(PCL_PROC_GRID=1xN).  Rank 0 gathers the blocks and compares the assembled q, bit for bit, with the single-block result
the test computed with run_case() and saved.

  python tests/cellbc_mp_worker.py <ref.npz>     with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment

The run: 24 x 18 acoustics, 8 classic steps of fixed length.  The lower x side is custom on every rank (each owns a part
of it) and stamps the GLOBAL row index c.i[1] into the pressure; the upper y side is custom too and extrapolates, which
only the ranks that own that boundary launch.  A block whose c.i started at 0, or a y launch on a rank inside the grid,
would change q.
"""
import base64
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyclaw_amd as pyclaw                  # noqa: E402
from pyclaw_amd import parallel             # noqa: E402
from apps import problems                   # noqa: E402

BODY = ("if (c.idim == 0) { q[0] = p[0] * c.i[1]; q[1] = 0.0; q[2] = 0.0; }\n"
        "else { for (int m = 0; m < MEQN; m++) q[m] = qin(m, 0); }")
NSTEPS = 8


def pack(a):
    return {"shape": list(a.shape), "data": base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")}


def unpack(d):
    return np.frombuffer(base64.b64decode(d["data"]), dtype=np.float64).reshape(d["shape"])


def run_case():
    """this block's arrays by name, and its state"""
    claw = problems.acoustics2D(pyclaw, mx=24, my=18, run=False)
    solver, solution = claw.solver, claw.solution
    solver.bc_lower[0] = solver.bc_upper[1] = pyclaw.BC.custom
    solver.user_bc_lower = solver.user_bc_upper = pyclaw.CellBC(BODY, params=[0.125])
    solver.dt_variable = False
    solver.setup(solution)
    solver.dt = solver.dt_initial
    solver.evolve_to_time(solution, NSTEPS * solver.dt)
    assert solver.status['numsteps'] == NSTEPS
    solver.teardown()
    return {"q": solution.state.q.copy('F')}, solution.state


def main():
    ref = np.load(sys.argv[1])
    parallel.init()
    rank, size = parallel.rank(), parallel.world_size()
    arrays, st = run_case()
    rng = [(d.nstart, d.nend) for d in st.grid.dimensions]
    blocks = parallel._state["group"].allgather({"rng": rng, "arrays": {k: pack(v) for k, v in arrays.items()}})
    ok = 0
    if rank == 0:
        same = len(set(tuple(map(tuple, b["rng"])) for b in blocks)) == size
        # every block spans x and the blocks differ in y: only then does one rank alone own the upper y side
        cut_y = all(tuple(b["rng"][0]) == (0, ref["q"].shape[1]) for b in blocks) and \
            len(set(tuple(b["rng"][1]) for b in blocks)) == size
        print("cut in y: %s" % cut_y)
        full = np.full(ref["q"].shape, np.nan)
        for b in blocks:
            full[(slice(None),) + tuple(slice(lo, hi) for lo, hi in b["rng"])] = unpack(b["arrays"]["q"])
        eq = np.array_equal(full, ref["q"])
        print("q: %d ranks, max |diff| %g, equal %s" % (size, np.nanmax(np.abs(full - ref["q"])), eq))
        print("bit-identical: %s" % (same and eq and cut_y))
        ok = 0 if same and eq and cut_y else 3
    parallel.barrier()
    parallel.shutdown()
    sys.exit(ok)


if __name__ == "__main__":
    main()
