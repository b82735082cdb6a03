"""
Worker for tests/test_gpu_cellfunctional.py: one of N processes that share ONE GPU (PCL_FORCE_DEVICE=0, host-staged halo
wire, as tests/cellfn_mp_worker.py) and evaluate functionals on a decomposed grid.  Every rank compares what
CellFunctional.evaluate returns, bit for bit, with the single-block values the test computed and saved.

  python tests/cellfunctional_mp_worker.py <case> <ref.npz>     with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set

  integers  the periodic 40 x 24 advection grid with the integer data of ref["q"]: the four operations on it, and with
            reach = 1 the total variation, whose differences reach across the cut
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyclaw_amd as pyclaw                  # noqa: E402
from pyclaw_amd import parallel             # noqa: E402
from apps import problems                   # noqa: E402

import test_gpu_cellfunctional as T         # noqa: E402


def main():
    case, ref = sys.argv[1], np.load(sys.argv[2])
    if case != "integers":
        raise SystemExit("unknown case " + case)
    parallel.init()
    rank, size = parallel.rank(), parallel.world_size()
    solver, solution = problems.advection2D(pyclaw, 40, 24)
    st = solution.state
    lo = [d.nstart for d in st.grid.dimensions]
    hi = [d.nend for d in st.grid.dimensions]
    st.q[...] = ref["q"][:, lo[0]:hi[0], lo[1]:hi[1]]
    solver.setup(solution)
    four = pyclaw.CellFunctional(T.FOUR, 4, reduce=T.FOUR_OPS).evaluate(solver, st)
    tv = pyclaw.CellFunctional(T.TV_2D, 1, reach=1).evaluate(solver, st)
    solver.teardown()
    cut = (hi[0] - lo[0]) < 40 and size == 2
    same = cut and np.array_equal(four.view(np.uint64), ref["four"].view(np.uint64)) and \
        np.array_equal(tv.view(np.uint64), ref["tv"].view(np.uint64))
    print("rank %d of %d, block x %d..%d: four %s tv %s, single block %s %s" % (rank, size, lo[0], hi[0], four, tv,
                                                                                ref["four"], ref["tv"]))
    print("bit-identical: %s" % same)
    parallel.barrier()
    parallel.shutdown()
    sys.exit(0 if same else 3)


if __name__ == "__main__":
    main()
