"""
Worker for tests/test_gpu_rk.py: one of two processes that share ONE GPU (PCL_FORCE_DEVICE=0, PCL_HALO_TRANSPORT=host, as in
tests/mp_gpu_worker.py) and run 64 x 32 acoustics with time_integrator = 'RK44' on a decomposed grid.  Every stage exchanges
its halo and all-reduces its Courant number; the combinations are pointwise.  Rank 0 assembles the blocks and saves the field
for the test to compare with the same run on one block.

  python tests/rk_mp_worker.py <out.npy>       with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment
"""
import base64
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_claw(pyclaw):
    from apps import problems
    claw = problems.acoustics2D(pyclaw, mx=64, my=32, tfinal=0.04, nout=1, solver_type='sharpclaw', time_integrator='RK44',
                                run=False)
    return claw


def main():
    import pyclaw_amd as pyclaw
    from pyclaw_amd import parallel
    parallel.init()
    rank, size = parallel.rank(), parallel.world_size()
    claw = make_claw(pyclaw)
    claw.run()
    st = claw.frames[claw.nout].state
    rng = [(d.nstart, d.nend) for d in st.grid.dimensions]
    g = parallel._state["group"]
    blocks = g.allgather({"rng": rng, "shape": list(st.q.shape),
                          "q": base64.b64encode(np.ascontiguousarray(st.q).tobytes()).decode("ascii"),
                          "steps": int(claw.solver.status["numsteps"])})
    if rank == 0:
        full = np.full((3, 64, 32), np.nan)
        for b in blocks:
            q = np.frombuffer(base64.b64decode(b["q"]), dtype=np.float64).reshape(b["shape"])
            full[(slice(None),) + tuple(slice(lo, hi) for lo, hi in b["rng"])] = q
        nb = len(set(tuple(map(tuple, b["rng"])) for b in blocks))
        np.save(sys.argv[1], full)
        print("RK44 on %d ranks: %d distinct blocks, steps %s" % (size, nb, sorted(set(b["steps"] for b in blocks))))
    parallel.barrier()
    parallel.shutdown()


if __name__ == "__main__":
    main()
