// ghost_rule.hpp -- the ghost-cell rule of the built-in boundary conditions (solver.py:384-452), stated once.
// The sweep kernels evaluate it while they load their tiles (classic.hpp, classic_fused.hpp), the ghost-fill and frame
// kernels of pclaw.hip apply it in memory, and pcl_ghost_map answers it on the host (tests/test_ghost_rule_cpu.py).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#include "../../include/pyclaw_amd.h"

namespace pcl {

// Boundary condition of one side as an index remap: ghost index k of a dimension with n cells (ghosts included)
// reads interior index `src`; `neg` = reflecting (negate the normal momentum component of q; an aux array is
// copied as it is), `cst` = constant inflow state (PCL_BC_CUSTOM, or the launchers' 100).  lo / hi < 0: no fill on
// that side, and every interior cell: the cell maps to itself.
struct VbcMap { int src; bool neg, cst; int side; };
__host__ __device__ __forceinline__ VbcMap vbc_map(int k, int n, int mbc, int lo, int hi) {
    VbcMap r{k, false, false, 0};
    if (k < mbc && lo >= 0) {
        r.side = 0;
        if (lo == PCL_BC_OUTFLOW) r.src = mbc;
        else if (lo == PCL_BC_PERIODIC) r.src = n - 2 * mbc + k;
        else if (lo == PCL_BC_REFLECTING) { r.src = 2 * mbc - 1 - k; r.neg = true; }
        else r.cst = true;
    } else if (k >= n - mbc && hi >= 0) {
        r.side = 1;
        if (hi == PCL_BC_OUTFLOW) r.src = n - mbc - 1;
        else if (hi == PCL_BC_PERIODIC) r.src = k - (n - 2 * mbc);    // q[n-mbc+t] = q[mbc+t]
        else if (hi == PCL_BC_REFLECTING) { r.src = 2 * (n - mbc) - 1 - k; r.neg = true; }
        else r.cst = true;
    }
    return r;
}

}  // namespace pcl
