"""
Worker for tests/test_gpu_cellfn.py: one of N processes that share ONE GPU (PCL_FORCE_DEVICE=0, host-staged halo wire,
as tests/mp_gpu_worker.py) and run a cell function on a decomposed grid.  Rank 0 gathers the blocks and compares the
assembled arrays, bit for bit, with the single-block result the test computed and saved.

  python tests/cellfn_mp_worker.py <case> <ref.npz>     with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment

  psystem   the p-system's unsplit classic step with the strain hook (start_step writes aux): q, aux and the resident aux
            with its ghost cells after 8 steps.  The aux halo exchange behind the hook is what a second block adds: the
            ghost columns next to the neighbour show it directly, and under the exponential law (ref["linearity"] = 2) q
            depends on them
  stamp     global index stamps on 65 x 3 cells: c.i of a block that does not start at 0
"""
import base64
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pyclaw_amd as pyclaw                  # noqa: E402
from pyclaw_amd import _lib, parallel       # noqa: E402
from apps import problems                   # noqa: E402
from apps import psystem as PS              # noqa: E402

STAMP = "for (int m = 0; m < MEQN; m++) q[m] = c.i[0] + 1000.0 * c.i[1] + 0.25 * m;"


def pack(a):
    return {"shape": list(a.shape), "data": base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii")}


def unpack(d):
    return np.frombuffer(base64.b64decode(d["data"]), dtype=np.float64).reshape(d["shape"])


def run_case(case, ref):
    """this block's arrays by name, and its state"""
    if case == "psystem":
        lin = int(ref["linearity"])
        claw = PS.psystem2D(pyclaw, solver_type='classic_unsplit', mx=24, my=20, linearity=lin, bc='periodic',
                            upper=(4.25, 4.25), amplitude=10.0 if lin == 1 else 1.0, run=False)
        solver, solution = claw.solver, claw.solution
        solver.dt_variable = False
        solver.setup(solution)
        solver.dt = float(ref["dt"])
        solver.evolve_to_time(solution, 8 * solver.dt)
        # the resident aux with its ghost cells: the columns next to the neighbour block come from the halo exchange
        auxbc = np.empty(solver.auxbc.shape, order='F')
        _lib.check(_lib.lib().pcl_get_aux(solver._h, _lib.d(auxbc)))
        solver.teardown()
        st = solution.state
        return {"q": st.q, "aux": st.aux, "auxbc": auxbc}, st
    if case == "stamp":
        claw = problems.acoustics2D(pyclaw, mx=65, my=3, run=False)
        solver, st = claw.solver, claw.solution.state
        solver.setup(claw.solution)
        solver._push(st)
        pyclaw.CellSource(STAMP).apply(solver, st, 0.0)
        solver._pull(st)
        solver.teardown()
        return {"q": st.q}, st
    raise SystemExit("unknown case " + case)


def main():
    case, ref = sys.argv[1], np.load(sys.argv[2])
    parallel.init()
    rank, size = parallel.rank(), parallel.world_size()
    arrays, st = run_case(case, ref)
    rng = [(d.nstart, d.nend) for d in st.grid.dimensions]
    blocks = parallel._state["group"].allgather({"rng": rng, "arrays": {k: pack(v) for k, v in arrays.items()}})
    ok = 0
    if rank == 0:
        same = len(set(tuple(map(tuple, b["rng"])) for b in blocks)) == size
        for name in arrays:
            if name == "auxbc":
                # a block's ghosted array is a window of the single block's: [nstart, nend + 2 mbc) of the ghosted index,
                # where the window does not wrap around (x is cut, so a block's outer ghost columns wrap: periodic copies
                # of the other end, compared through the index modulo the interior extent)
                full_ref, eq, mbc = ref[name], True, 2
                n = [full_ref.shape[1] - 2 * mbc, full_ref.shape[2] - 2 * mbc]
                for b in blocks:
                    got = unpack(b["arrays"][name])
                    ix = [(np.arange(lo - mbc, hi + mbc) % n[k]) + mbc for k, (lo, hi) in enumerate(b["rng"])]
                    eq = eq and np.array_equal(got, full_ref[:, ix[0][:, None], ix[1][None, :]])
                print("case %s, %s: ghosted blocks equal the single block's windows: %s" % (case, name, eq))
                same = same and eq
                continue
            full = np.full(ref[name].shape, np.nan)
            for b in blocks:
                full[(slice(None),) + tuple(slice(lo, hi) for lo, hi in b["rng"])] = unpack(b["arrays"][name])
            eq = np.array_equal(full, ref[name])
            print("case %s, %s: %d ranks, max |diff| %g, equal %s" % (case, name, size, np.nanmax(np.abs(full - ref[name])), eq))
            same = same and eq
        print("bit-identical: %s" % same)
        ok = 0 if same else 3
    parallel.barrier()
    parallel.shutdown()
    sys.exit(ok)


if __name__ == "__main__":
    main()
