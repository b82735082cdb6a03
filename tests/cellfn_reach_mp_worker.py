"""
Worker for tests/test_gpu_cellfn_reach.py: one of N processes that share ONE GPU (PCL_FORCE_DEVICE=0, host-staged halo
wire, as tests/cellfn_mp_worker.py) and run cell functions that read neighbour cells on a decomposed grid.  Rank 0 gathers
the blocks and compares the assembled q, bit for bit, with the single-block result the test computed and saved.

  python tests/cellfn_reach_mp_worker.py <case> <ref.npz>     with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment

  advection   40 x 24 periodic advection with the diagonal-mean start_step and the 5-point diffusion step_src, both
              reach = 1: the corner ghost cells and the ghost columns next to the neighbour block come from the halo
              exchange of the apply_q_bcs in front of each launch
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


def pack(a):
    return {"shape": list(a.shape), "data": base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")}


def unpack(d):
    return np.frombuffer(base64.b64decode(d["data"]), dtype=np.float64).reshape(d["shape"])


def run_case(case, ref):
    """this block's q, and its state"""
    if case == "advection":
        solver, solution = problems.advection2D(pyclaw, 40, 24)
        solver.start_step = pyclaw.CellStartStep(problems.DIAGONAL_MEAN_CELL_HOOK, reach=1)
        solver.step_src = pyclaw.CellSource(problems.DIFFUSION_2D_CELL_SRC, params=[float(ref["nu"]), 0], reach=1)
        problems.fixed_steps(solver, solution, int(ref["nsteps"]), float(ref["dt"]))
        return solution.state.q, solution.state
    raise SystemExit("unknown case " + case)


def main():
    case, ref = sys.argv[1], np.load(sys.argv[2])
    parallel.init()
    rank, size = parallel.rank(), parallel.world_size()
    q, st = run_case(case, ref)
    rng = [(d.nstart, d.nend) for d in st.grid.dimensions]
    blocks = parallel._state["group"].allgather({"rng": rng, "q": pack(q)})
    ok = 0
    if rank == 0:
        same = len(set(tuple(map(tuple, b["rng"])) for b in blocks)) == size
        full = np.full(ref["q"].shape, np.nan)
        for b in blocks:
            full[(slice(None),) + tuple(slice(lo, hi) for lo, hi in b["rng"])] = unpack(b["q"])
        eq = np.array_equal(full, ref["q"])
        print("case %s: %d ranks, max |diff| %g, equal %s" % (case, size, np.nanmax(np.abs(full - ref["q"])), eq))
        same = same and eq
        print("bit-identical: %s" % same)
        ok = 0 if same else 3
    parallel.barrier()
    parallel.shutdown()
    sys.exit(ok)


if __name__ == "__main__":
    main()
