// kernels.hip -- the sweep kernels + their launch code, compiled ONCE PER ARITHMETIC MODE:
//   -DPCL_NS=exact -DPCL_FAST=0 -ffp-contract=off   bit-identical to the reference (no FMA,
//                                                   correctly rounded divide/sqrt)
//   -DPCL_NS=fast  -DPCL_FAST=1 -ffp-contract=fast  FMA contraction + reciprocal-multiply
//                                                   division; checked at rtol 1e-12
// Distinct namespaces keep the two sets of template instantiations apart at link time.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <string>

#include "../../include/pyclaw_amd.h"
#include "classic.hpp"
#include "sharpclaw.hpp"
#include "classic3.hpp"
#include "classic_fused.hpp"

namespace pcl {
namespace PCL_NS {

namespace {

int hip_fail(std::string &err, const char *what, hipError_t e) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return PCL_EHIP;
}

// Every built-in Riemann solver, once.  with(rp, f) calls f(RpTag<RP>{}) for the solver whose ID is rp and returns what f
// returns: a PCL_* code, or RP_NONE where that solver has no kernel of the kind asked for; RP_NONE too if no solver has
// the id.  What f instantiates under `if constexpr` on the solver's traits (rp.hpp) is all that gets built.
constexpr int RP_NONE = 1;      // no PCL_* code is positive
template <class RP> struct RpTag { using type = RP; };
template <class... RP> struct RpList {
    template <class F> static int with(int rp, F &&f) {
        int rc = RP_NONE;
        (void)((rp == RP::ID && ((rc = f(RpTag<RP>{})), true)) || ...);
        return rc;
    }
    static const RpFacts *facts(int rp) {
        static constexpr RpFacts table[] = {{RP::ID, RP::NDIM, RP::MEQN, RP::MWAVES, RP::NAUX, IsFwave<RP>::value,
                                             RP::ONEK && RP::NAUX == 0, RP::ONEK && RP::NAUX > 0, RP::SHARP,
                                             RP::SHARP_HIGH, RP::SHARP_WAVE}...};
        for (const RpFacts &f : table)
            if (f.id == rp) return &f;
        return nullptr;
    }
};
using Solvers = RpList<Advection1D, Acoustics1D, Burgers1D, Euler1D, Shallow1D, AdvectionColor1D, Elasticity1D, Acoustics2D,
                       Euler5, Advection2D, Shallow2D, VcAcoustics2D, VcAdvection2D, ShallowSphere, PSystem2D, VcAcoustics3D>;
int not_built(std::string &err, const char *why) { err = why; return PCL_EINVAL; }

// The grid of sweep_kernel<., IXY, ., ., DIM1> over l.a: the same for every solver, built in or compiled at run time
// (nblocks == 0: the tile subset is empty, nothing to launch).
struct SweepGrid { unsigned nblocks; int ntiles_across, ntiles_along; };
template <int IXY, bool DIM1> int sweep_grid(const SweepArgs &a, SweepGrid &g, std::string &err) {
    using T = TileShape<IXY>;
    const int n_across = IXY == 1 ? a.J : a.I + (LINE - a.mbc);  // y: columns counted from the line boundary
    const int m_along = IXY == 1 ? a.mx : a.my;
    g.ntiles_across = (n_across + T::ACROSS - 1) / T::ACROSS;
    g.ntiles_along = (m_along + T::NSTRIP * STRIP - 1) / (T::NSTRIP * STRIP);
    g.nblocks = (unsigned)g.ntiles_across * (unsigned)g.ntiles_along;
    if (a.sub != 0) {
        if (IXY != 1 || DIM1 || a.box[0] < 0 || a.box[1] > g.ntiles_across || a.box[2] < 0 ||
            a.box[3] > g.ntiles_along || a.box[0] >= a.box[1] || a.box[2] >= a.box[3]) {
            err = "tile subset: bad box";
            return PCL_EINVAL;
        }
        const unsigned inside = (unsigned)(a.box[1] - a.box[0]) * (unsigned)(a.box[3] - a.box[2]);
        g.nblocks = a.sub == 1 ? inside : g.nblocks - inside;
    }
    return PCL_OK;
}

// What the module of a user-written Riemann solver was compiled for against what this launch asks: the kernel's FWAVE and
// CAPA are template flags (cellrp.hpp: the handle's form), so a launch that says otherwise would run the wrong kernel.
static int user_form_check(const SweepLaunch &l, std::string &err) {
    const CellrpSpec &u = l.user;
    if ((l.fwave != 0) != u.fwave()) {
        err = u.fwave() ? "user-written Riemann solver: the attached solver was compiled for f-waves and the step is in wave form"
                        : "user-written Riemann solver: the step asks for f-waves and the attached solver was compiled in wave form";
        return PCL_EINVAL;
    }
    if ((l.a.mcapa > 0) != u.capa()) {
        err = u.capa() ? "user-written Riemann solver: the attached solver was compiled for a capacity function and the step has none"
                       : "user-written Riemann solver: the step has a capacity function and the attached solver was compiled without one";
        return PCL_EINVAL;
    }
    if ((u.naux > 0 || u.capa()) && !l.a.aux) {
        err = u.naux > 0 ? "user-written Riemann solver: this solver reads aux arrays and there are none (pcl_put_aux)"
                         : "user-written Riemann solver: the capacity function is a component of the aux arrays and there are none (pcl_put_aux)";
        return PCL_EINVAL;
    }
    return PCL_OK;
}

// A user-written Riemann solver (cellrp.hpp): l.user_fn is sweep_kernel<UserRp, IXY, CAPA, FWAVE, DIM1> of a module compiled
// at run time from the text of classic.hpp for the form of l.user, so the kernel's parameters are those of the launches below.
template <int IXY, bool DIM1> int launch_user(const SweepLaunch &l, std::string &err) {
    if (!l.user_fn) { err = "user-written Riemann solver: no compiled solver is attached (pcl_cellrp_attach)"; return PCL_ESTATE; }
    if (l.user.sharp()) { err = "user-written Riemann solver: the attached solver was compiled for SharpClaw and holds no classic sweep"; return PCL_EINVAL; }
    if (l.a.src_id != 0) { err = "user-written Riemann solver: no fused source"; return PCL_EINVAL; }
    if (int rc = user_form_check(l, err)) return rc;
    SweepGrid g;
    if (int rc = sweep_grid<IXY, DIM1>(l.a, g, err)) return rc;
    if (g.nblocks == 0) return PCL_OK;
    SweepArgs a = l.a;
    void *params[] = {&a, &g.ntiles_across, &g.ntiles_along};
    hipError_t e = hipModuleLaunchKernel(l.user_fn, g.nblocks, 1, 1, 256, 1, 1, 0, l.stream, params, nullptr);
    return e == hipSuccess ? PCL_OK : hip_fail(err, "sweep launch (user-written Riemann solver)", e);
}

template <class RP, int IXY, bool DIM1> int launch(const SweepLaunch &l, std::string &err) {
    const SweepArgs &a = l.a;
    SweepGrid g;
    if (int rc = sweep_grid<IXY, DIM1>(a, g, err)) return rc;
    if (g.nblocks == 0) return PCL_OK;
    const int ntiles_across = g.ntiles_across, ntiles_along = g.ntiles_along;
    const dim3 grid(g.nblocks);
    constexpr bool FW = IsFwave<RP>::value;       // f-wave solvers run the flux2fw.f / step1fw.f form of the kernel
    if ((l.fwave != 0) != FW) {
        err = FW ? "this Riemann solver returns f-waves: set solver.fwave = True (classic1fw / classic2fw)"
                 : "solver.fwave = True needs an f-wave Riemann solver (elasticity_fwave_1d, psystem_fwave_2d)";
        return PCL_EINVAL;
    }
    if (a.src_id != 0) {      // fused source term: its own instantiation (classic.hpp), Euler y pass without capa
        if constexpr (IXY == 2 && !DIM1 && std::is_same<RP, Euler5>::value) {
            if (a.src_id != 1 || a.mcapa > 0) { err = "fused source: Euler radial source, no capacity function"; return PCL_EINVAL; }
            hipLaunchKernelGGL((sweep_kernel<RP, IXY, false, FW, DIM1, true>), grid, dim3(256), 0, l.stream, a,
                               ntiles_across, ntiles_along);
            hipError_t e = hipGetLastError();
            return e == hipSuccess ? PCL_OK : hip_fail(err, "sweep launch", e);
        } else {
            err = "fused source: only the y pass of the Euler solver has it";
            return PCL_EINVAL;
        }
    }
    if (a.mcapa > 0)
        hipLaunchKernelGGL((sweep_kernel<RP, IXY, true, FW, DIM1>), grid, dim3(256), 0, l.stream, a,
                           ntiles_across, ntiles_along);
    else
        hipLaunchKernelGGL((sweep_kernel<RP, IXY, false, FW, DIM1>), grid, dim3(256), 0, l.stream, a,
                           ntiles_across, ntiles_along);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "sweep launch", e);
}

}  // namespace

// one directional sweep qin -> qout; ids 1 = x (or the 1-D step), 2 = y
int launch_sweep(const SweepLaunch &l, std::string &err) {
    if (l.rp == PCL_RP_CELL)
        return l.ndim == 1 ? launch_user<1, true>(l, err) : l.ids == 1 ? launch_user<1, false>(l, err) : launch_user<2, false>(l, err);
    const int rc = Solvers::with(l.rp, [&](auto tag) {
        using RP = typename decltype(tag)::type;
        if constexpr (RP::NDIM == 1) return l.ndim == 1 ? launch<RP, 1, true>(l, err) : RP_NONE;
        else if constexpr (RP::NDIM == 2)
            return l.ndim == 1 ? RP_NONE : l.ids == 1 ? launch<RP, 1, false>(l, err) : launch<RP, 2, false>(l, err);
        else return RP_NONE;
    });
    if (rc != RP_NONE) return rc;
    return not_built(err, l.ndim == 1 ? "Riemann solver id is not a 1-D solver" : "Riemann solver id is not a 2-D solver");
}

// the whole dimension-split 2-D step, qin -> qout (classic_fused.hpp); l.a as for the x pass + a.dtd_t = dt/dy and
// a.src_id of the step.  The host (pclaw.hip: fused_step_ok) only sends what the kernel covers.
namespace {
static_assert(F_OWN_C == TILE_OWN_C && F_OWN_R == TILE_OWN_R, "the host counts tiles with TILE_OWN_* (sweep_args.hpp)");
// What a one-kernel launch asks of l whatever the solver, built in or compiled at run time (naux: the aux components its
// normal solver reads), and the grid: ntx x nty tiles, nblocks workgroups (0: the tile subset is empty, nothing to launch).
struct Step2dsGrid { int ntx, nty; unsigned nblocks; };
int step2ds_grid(const SweepLaunch &l, int naux, Step2dsGrid &g, std::string &err) {
    const SweepArgs &a = l.a;
    if (a.mbc != HALO) { err = "step2ds kernel: mbc = 2"; return PCL_EINVAL; }
    const bool capa = a.mcapa > 0;
    if ((capa || naux > 0) && !a.aux) { err = "step2ds kernel: this solver reads aux arrays and there are none"; return PCL_EINVAL; }
    // quiet tiles: the bookkeeping of the aux-free instantiations without a capacity function only (classic_fused.hpp)
    if ((capa || naux > 0) && (l.tq_out || l.tq_list)) { err = "step2ds kernel: no quiet-tile bookkeeping with aux arrays"; return PCL_EINVAL; }
    g.ntx = (a.mx + F_OWN_C - 1) / F_OWN_C;
    g.nty = (a.my + F_OWN_R - 1) / F_OWN_R;
    g.nblocks = (unsigned)g.ntx * (unsigned)g.nty;
    if (a.sub != 0) {
        if (a.box[0] < 0 || a.box[1] > g.nty || a.box[2] < 0 || a.box[3] > g.ntx || a.box[0] >= a.box[1] || a.box[2] >= a.box[3]) {
            err = "step2ds tile subset: bad box";
            return PCL_EINVAL;
        }
        const unsigned inside = (unsigned)(a.box[1] - a.box[0]) * (unsigned)(a.box[3] - a.box[2]);
        g.nblocks = a.sub == 1 ? inside : g.nblocks - inside;
        if (g.nblocks == 0) return PCL_OK;
    }
    // a list launch: the tiles the hand-over+list kernel behind the previous launch listed (classic_fused.hpp); one
    // workgroup per tile of the grid, those past the list's end return at once
    const bool list = l.tq_list != nullptr;
    if ((list && (a.sub != 0 || !l.tq_out || !l.tq_cfl || !l.tq_next)) || (l.tq_ring && !list)) {
        err = "step2ds tile list: the whole block, with its bookkeeping";
        return PCL_EINVAL;
    }
    return PCL_OK;
}

// A user-written Riemann solver compiled with the one-kernel step (cellrp.hpp: spec.onek): l.user_fn is
// step2ds_kernel<UserRp, FWAVE, false, CAPA> of the module compiled at run time from the text of classic_fused.hpp, FWAVE
// and CAPA the form of l.user, so the grid, the block and the thirteen parameters are those of launch_step2ds_t below.
int launch_step2ds_user(const SweepLaunch &l, std::string &err) {
    if (!l.user_fn || !l.user.onek) {
        err = "user-written Riemann solver: no solver compiled with the one-kernel step is attached (pcl_cellrp_compile_onek, pcl_cellrp_attach)";
        return PCL_ESTATE;
    }
    if (l.user.sharp()) { err = "user-written Riemann solver: the attached solver was compiled for SharpClaw and holds no classic step"; return PCL_EINVAL; }
    if (l.a.src_id != 0) { err = "user-written Riemann solver: no fused source"; return PCL_EINVAL; }
    if (int rc = user_form_check(l, err)) return rc;
    Step2dsGrid g;
    if (int rc = step2ds_grid(l, l.user.naux, g, err)) return rc;
    if (g.nblocks == 0) return PCL_OK;
    SweepArgs a = l.a;
    unsigned *tq_out = l.tq_out, *tq_ring = l.tq_ring, *tq_reuse = l.tq_reuse, *tq_ycol = l.tq_ycol;
    double2 *tq_cfl = l.tq_cfl;
    const int *tq_list = l.tq_list;
    const TileNext *tq_next = l.tq_next;
    unsigned ring_seq = l.ring_seq;
    int rowreuse = l.rowreuse, ycol = l.ycol;
    void *params[] = {&a, &g.ntx, &g.nty, &tq_out, &tq_cfl, &tq_list, &tq_next, &tq_ring, &ring_seq, &tq_reuse, &rowreuse, &tq_ycol, &ycol};
    hipError_t e = hipModuleLaunchKernel(l.user_fn, g.nblocks, 1, 1, F_THREADS, 1, 1, 0, l.stream, params, nullptr);
    return e == hipSuccess ? PCL_OK : hip_fail(err, "step2ds launch (user-written Riemann solver)", e);
}

template <class RP> int launch_step2ds_t(const SweepLaunch &l, std::string &err) {
    const SweepArgs &a = l.a;
    constexpr bool FW = IsFwave<RP>::value;
    if ((l.fwave != 0) != FW) { err = "solver.fwave does not match the Riemann solver"; return PCL_EINVAL; }
    Step2dsGrid g;
    if (int rc = step2ds_grid(l, RP::NAUX, g, err)) return rc;
    if (g.nblocks == 0) return PCL_OK;
    const int ntx = g.ntx, nty = g.nty;
    const bool capa = a.mcapa > 0;
    if (a.src_id != 0 && !(std::is_same<RP, Euler5>::value && a.src_id == 1 && !capa)) {
        err = "fused source: only the Euler solver's radial source, no capacity function";
        return PCL_EINVAL;
    }
    const dim3 grid(g.nblocks);
    if (a.src_id != 0) {
        if constexpr (std::is_same<RP, Euler5>::value)
            hipLaunchKernelGGL((step2ds_kernel<RP, FW, true>), grid, dim3(F_THREADS), 0, l.stream, a, ntx, nty, l.tq_out,
                               l.tq_cfl, l.tq_list, l.tq_next, l.tq_ring, l.ring_seq, l.tq_reuse, l.rowreuse, l.tq_ycol, l.ycol);
    } else if (capa)
        hipLaunchKernelGGL((step2ds_kernel<RP, FW, false, true>), grid, dim3(F_THREADS), 0, l.stream, a, ntx, nty, l.tq_out,
                           l.tq_cfl, l.tq_list, l.tq_next, l.tq_ring, l.ring_seq, l.tq_reuse, l.rowreuse, l.tq_ycol, l.ycol);
    else
        hipLaunchKernelGGL((step2ds_kernel<RP, FW, false>), grid, dim3(F_THREADS), 0, l.stream, a, ntx, nty, l.tq_out,
                           l.tq_cfl, l.tq_list, l.tq_next, l.tq_ring, l.ring_seq, l.tq_reuse, l.rowreuse, l.tq_ycol, l.ycol);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "step2ds launch", e);
}
}  // namespace
int launch_step2ds(const SweepLaunch &l, std::string &err) {
    if (l.rp == PCL_RP_CELL) return launch_step2ds_user(l, err);
    const int rc = Solvers::with(l.rp, [&](auto tag) {
        using RP = typename decltype(tag)::type;
        if constexpr (RP::ONEK) return launch_step2ds_t<RP>(l, err);
        else return RP_NONE;
    });
    return rc != RP_NONE ? rc : not_built(err, "step2ds kernel: no instantiation for this Riemann solver");
}

// The grid of sweep3_kernel<., DIR, .> over l.a, DIR = l.ids: the same for the built-in solver and one compiled at run time
namespace {
struct Sweep3Grid { int ntiles_ac, ntiles_al; };
Sweep3Grid sweep3_grid(const SweepLaunch &l) {
    const SweepArgs &a = l.a;
    const int n_ac = l.ids == 1 ? a.n_ac : a.n_ac + (LINE - a.mbc);  // y, z: columns counted from the line boundary
    const int ac = l.ids == 1 ? Tile3Shape<1>::AC : Tile3Shape<2>::AC, adv = l.ids == 1 ? Tile3Shape<1>::ADV : Tile3Shape<2>::ADV;
    static_assert(Tile3Shape<3>::AC == Tile3Shape<2>::AC && Tile3Shape<3>::ADV == Tile3Shape<2>::ADV, "y and z: one tile shape");
    return {(n_ac + ac - 1) / ac, (a.m_al + adv - 1) / adv};
}

// A user-written Riemann solver (cellrp.hpp) in 3-D: l.user_fn is sweep3_kernel<UserRp, l.ids, CAPA> of a module compiled at
// run time from the text of classic.hpp, so the kernel's parameters and grid are those of the built-in launch below.
int launch_sweep3_user(const SweepLaunch &l, std::string &err) {
    if (!l.user_fn) { err = "user-written Riemann solver: no compiled solver is attached (pcl_cellrp_attach)"; return PCL_ESTATE; }
    if (l.user.sharp()) { err = "user-written Riemann solver: the attached solver was compiled for SharpClaw and holds no classic sweep"; return PCL_EINVAL; }
    if (l.user.ndim != 3) { err = "user-written Riemann solver: the attached solver was not compiled for the 3-D sweeps (pcl_cellrp_compile3)"; return PCL_EINVAL; }
    if (l.ids < 1 || l.ids > 3) { err = "3-D sweep: direction must be 1, 2 or 3"; return PCL_EINVAL; }
    if (l.a.src_id != 0) { err = "user-written Riemann solver: no fused source"; return PCL_EINVAL; }
    if (l.a.mbc != HALO) { err = "3-D sweep: mbc = 2"; return PCL_EINVAL; }
    if (int rc = user_form_check(l, err)) return rc;
    const Sweep3Grid g = sweep3_grid(l);
    SweepArgs a = l.a;
    int ntiles_ac = g.ntiles_ac, ntiles_al = g.ntiles_al;
    void *params[] = {&a, &ntiles_ac, &ntiles_al};
    hipError_t e = hipModuleLaunchKernel(l.user_fn, (unsigned)ntiles_ac * (unsigned)ntiles_al, (unsigned)a.n_b, 1, 256, 1, 1, 0,
                                         l.stream, params, nullptr);
    return e == hipSuccess ? PCL_OK : hip_fail(err, "sweep3 launch (user-written Riemann solver)", e);
}
}  // namespace

// 3-D dimension-split sweep along direction l.ids (classic.hpp: sweep3_kernel)
int launch_sweep3(const SweepLaunch &l, std::string &err) {
    const SweepArgs &a = l.a;
    if (l.rp == PCL_RP_CELL) return launch_sweep3_user(l, err);
    if (l.fwave) { err = "fwave: no 3-D f-wave Riemann solver is built in"; return PCL_EINVAL; }
    if (l.rp != VcAcoustics3D::ID) { err = "Riemann solver id is not a 3-D solver"; return PCL_EINVAL; }
    const Sweep3Grid g = sweep3_grid(l);
    const int ntiles_ac = g.ntiles_ac, ntiles_al = g.ntiles_al;
    const dim3 grid((unsigned)ntiles_ac * (unsigned)ntiles_al, (unsigned)a.n_b);
    if (a.mcapa > 0) {      // capacity function (step3ds.f:138-141,196-200)
        if (l.ids == 1) hipLaunchKernelGGL((sweep3_kernel<VcAcoustics3D, 1, true>), grid, dim3(256), 0, l.stream, a, ntiles_ac, ntiles_al);
        else if (l.ids == 2) hipLaunchKernelGGL((sweep3_kernel<VcAcoustics3D, 2, true>), grid, dim3(256), 0, l.stream, a, ntiles_ac, ntiles_al);
        else hipLaunchKernelGGL((sweep3_kernel<VcAcoustics3D, 3, true>), grid, dim3(256), 0, l.stream, a, ntiles_ac, ntiles_al);
    } else if (l.ids == 1) hipLaunchKernelGGL((sweep3_kernel<VcAcoustics3D, 1>), grid, dim3(256), 0, l.stream, a, ntiles_ac, ntiles_al);
    else if (l.ids == 2) hipLaunchKernelGGL((sweep3_kernel<VcAcoustics3D, 2>), grid, dim3(256), 0, l.stream, a, ntiles_ac, ntiles_al);
    else hipLaunchKernelGGL((sweep3_kernel<VcAcoustics3D, 3>), grid, dim3(256), 0, l.stream, a, ntiles_ac, ntiles_al);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "sweep3 launch", e);
}

// unsplit 3-D step, one direction: march3p_kernel (classic3.hpp), one launch per direction
namespace {
template <class RP, int DIR> int launch_unsplit3_t(const Unsplit3Launch &l, std::string &err) {
    static_assert(RP::T3_PRESSURE, "the marching kernel takes the pressure-driven pieces");
    const SweepArgs &a = l.a;
    Slices3Args t;
    t.s_e = l.s_e; t.s_f = l.s_f; t.n_e = l.n_e; t.n_f = l.n_f;
    t.lo_e = a.mbc - 1; t.hi_e = a.mbc + l.m_e; t.lo_f = a.mbc - 1; t.hi_f = a.mbc + l.m_f;
    t.m3 = l.m3; t.m4 = l.m4; t.dty = l.dty; t.dtz = l.dtz;
    constexpr int NW = 8;
    March3Args g;
    g.qsrc = DIR == 1 ? a.qin : l.qacc;
    g.qacc = l.qacc;
    const bool e_outer = DIR == 2;
    g.s_w = e_outer ? l.s_f : l.s_e; g.s_m = e_outer ? l.s_e : l.s_f;
    g.n_w = e_outer ? l.n_f : l.n_e; g.n_m = e_outer ? l.n_e : l.n_f;
    g.m_w = e_outer ? l.m_f : l.m_e; g.m_m = e_outer ? l.m_e : l.m_f;
    g.ntiles_al = (a.m_al + STRIP - 1) / STRIP;
    g.ntiles_w = (g.m_w + (NW - 2) - 1) / (NW - 2);
    // march segments: enough workgroups to fill the 256 CUs in whole rounds, not so many that the two extra source
    // planes per segment cost more than the idle CUs would
    const long per = (long)g.ntiles_al * g.ntiles_w;
    int best = 1;
    double best_eff = 0.0;
    for (int ns = 1; ns <= (g.m_m + 7) / 8; ns++) {
        const int seg = (g.m_m + ns - 1) / ns;
        const long wgs = per * ((g.m_m + seg - 1) / seg);
        const double eff = (double)wgs / (256.0 * ((wgs + 255) / 256)) * seg / (seg + 2.0);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = ns; }
    }
    g.seg = (g.m_m + best - 1) / best;
    const int nseg = (g.m_m + g.seg - 1) / g.seg;
    if (DIR == 1) {     // the first direction writes interior cells only: the ghost frame of the result := qold's
        const int I = a.n_al, J = l.n_e, K = l.n_f;
        hipLaunchKernelGGL(ghost3_copy_kernel, dim3((unsigned)((I + 255) / 256), (unsigned)J, (unsigned)K), dim3(256), 0,
                           l.stream, a.qin, l.qacc, (int)RP::MEQN, a.plane, I, J, K, l.s_e, a.mbc);
    }
    if (l.m3 == 2 && l.m4 == 2)      // the solver default, method(3) = 22, as constants
        hipLaunchKernelGGL((march3p_kernel<RP, DIR, NW, 22>), dim3((unsigned)(per * nseg)), dim3(NW * WAVE), 0, l.stream, a, t, g);
    else
        hipLaunchKernelGGL((march3p_kernel<RP, DIR, NW>), dim3((unsigned)(per * nseg)), dim3(NW * WAVE), 0, l.stream, a, t, g);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "march3 launch", e);
}
}  // namespace

int launch_unsplit3(const Unsplit3Launch &l, std::string &err) {
    if (l.rp != VcAcoustics3D::ID) { err = "Riemann solver id is not a 3-D solver with transverse solvers"; return PCL_EINVAL; }
    if (l.a.mcapa > 0) { err = "3-D: capacity function not implemented"; return PCL_EINVAL; }
    if (l.dir == 1) return launch_unsplit3_t<VcAcoustics3D, 1>(l, err);
    if (l.dir == 2) return launch_unsplit3_t<VcAcoustics3D, 2>(l, err);
    return launch_unsplit3_t<VcAcoustics3D, 3>(l, err);
}

#if !PCL_FAST
// the host layer's view of the solver list (sweep_args.hpp: RpFacts; nothing in it depends on the arithmetic mode)
const RpFacts *rp_facts(int rp) { return Solvers::facts(rp); }
// planes (q components + staged aux components) the LDS tile of sweep_kernel holds within a workgroup's 64 KB, for both
// tile shapes: what a user-written Riemann solver's meqn + naux may come to (cellrp.hpp)
int sweep_tile_max_planes() {
    constexpr int PLANE = TileShape<1>::PLANE > TileShape<2>::PLANE ? TileShape<1>::PLANE : TileShape<2>::PLANE;
    // (a user-written solver compiled with the one-kernel step meets this limit first: it must lie inside that tile's)
    static_assert(65536 / ((int)sizeof(double) * PLANE) <= ONEK_MAX_PLANES, "the sweep tile's plane limit lies inside the one-kernel tile's");
    return 65536 / ((int)sizeof(double) * PLANE);
}
// the same for the 3-D sweeps (sweep3_kernel: Tile3Shape<1..3>::PLANE against 64 KB, classic.hpp): meqn + naux + capa
int sweep3_tile_max_planes() { return sweep3_tile_planes(); }
// the same for the SharpClaw kernels of a user-written Riemann solver: sharp_kernel's tile is static LDS of TA * 64 doubles
// per plane, TA = sharp_tile_across (16; 8 in the y pass from six aux components on).  The y pass (ixy 2) stages meqn + capa
// + naux planes, the x pass (ixy 1; the 1-D pass too) meqn + capa: it reads aux from global memory.
int sharp_tile_max_planes(int ixy, int naux) { return 65536 / ((int)sizeof(double) * sharp_tile_across_n(ixy, naux) * WAVE); }
// the same for the one-kernel step (classic_fused.hpp): tile (ty, tx) reads rows mbc-2+F_OWN_R*ty .. +F_ROWS-1 and columns
// mbc-2+60*tx .. +63; box = [ty_lo, ty_hi) x [tx_lo, tx_hi), ntiles = (nty, ntx)
bool step2ds_interior_box(const BlockGeom &a, int box[4], int ntiles[2]) {
    const int ntx = (a.mx + F_OWN_C - 1) / F_OWN_C, nty = (a.my + F_OWN_R - 1) / F_OWN_R;
    box[0] = 1;
    const int roomy = a.my + HALO - F_ROWS;       // F_OWN_R*ty + F_ROWS <= my + 2
    box[1] = roomy < 0 ? 0 : std::min(nty, roomy / F_OWN_R + 1);
    box[2] = 1;
    const int roomx = a.mx + HALO - F_COLS;
    box[3] = roomx < 0 ? 0 : std::min(ntx, roomx / F_OWN_C + 1);
    ntiles[0] = nty;
    ntiles[1] = ntx;
    return box[0] < box[1] && box[2] < box[3];
}
// the Courant hand-over behind a one-kernel launch of the whole block, with the next launch's tile list
// (classic_fused.hpp: handover_list_kernel; no arithmetic, the same in every mode)
int launch_tile_handover(const TileHandover &h, std::string &err) {
    if (!h.cfl || !h.host || !h.tq_in || !h.tq_out || !h.tq_cfl || !h.tq_list || !h.next || !h.other || h.next == h.other ||
        h.ntx <= 0 || h.nty <= 0) {
        err = "tile hand-over: bad arguments";
        return PCL_EINVAL;
    }
    const unsigned nt = (unsigned)h.ntx * (unsigned)h.nty;
    // workgroup 0: the hand-over; workgroups 1..: the tiles
    hipLaunchKernelGGL(handover_list_kernel, dim3(1 + (nt + TL_THREADS - 1) / TL_THREADS), dim3(TL_THREADS), 0, h.stream,
                       h.cfl, h.host, h.seq, h.ntx, h.nty, h.mbc, h.mx, h.my, h.tq_in, h.tq_out, h.tq_cfl, h.tq_list,
                       h.next, h.other, h.ran);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "tile hand-over launch", e);
}
bool x_interior_box(const BlockGeom &a, int box[4], int ntiles[2]) {
    using T = TileShape<1>;
    constexpr int ADV = T::NSTRIP * STRIP;  // cells a tile advances along the row
    const int ntb = (a.J + T::ACROSS - 1) / T::ACROSS, nta = (a.mx + ADV - 1) / ADV;
    // rows b0 = ACROSS*tb .. b0+ACROSS-1 inside [mbc, J-mbc); cells a0 = mbc-HALO+ADV*ta .. a0+ALONG-1 inside [mbc, I-mbc)
    box[0] = (a.mbc + T::ACROSS - 1) / T::ACROSS;
    box[1] = std::min(ntb, (a.J - a.mbc) / T::ACROSS);
    box[2] = (HALO + ADV - 1) / ADV;
    const int room = a.I - a.mbc - T::ALONG - (a.mbc - HALO);  // ADV*ta <= room
    box[3] = room < 0 ? 0 : std::min(nta, room / ADV + 1);
    ntiles[0] = ntb;
    ntiles[1] = nta;
    return box[0] < box[1] && box[2] < box[3];
}
#endif

// unsplit step (step2.f / step2qcor.f): both phases without scratch planes (classic.hpp: unsplit_x/y_kernel)
namespace {
template <class RP, int UX, int UY> int launch_unsplit_u(const SweepLaunch &l, const double *qx, std::string &err) {
    SweepArgs a = l.a;
    if (l.ids == 1) {
        const int nstrips = (a.mx + STRIP - 1) / STRIP;
        const int ntr = (a.my + (UX - 2) - 1) / (UX - 2);
        if (a.sub != 0) {
            // tiles whose 64 cells x UX rows lie inside the interior: cells mbc-2+60*ta .. +63 within [mbc, mbc+mx),
            // rows mbc-1+(UX-2)*tr .. +UX-1 within [mbc, mbc+my)
            a.box[0] = 1;
            a.box[1] = a.my - UX + 1 >= 0 ? (a.my - UX + 1) / (UX - 2) + 1 : 0;
            a.box[2] = 1;
            a.box[3] = a.mx >= 62 ? (a.mx - 62) / STRIP + 1 : 0;
        }
        if (a.mcapa > 0)
            hipLaunchKernelGGL((unsplit_x_kernel<RP, IsFwave<RP>::value, UX, true>), dim3((unsigned)nstrips * ntr),
                               dim3(UX * WAVE), 0, l.stream, a, nstrips);
        else
            hipLaunchKernelGGL((unsplit_x_kernel<RP, IsFwave<RP>::value, UX>), dim3((unsigned)nstrips * ntr),
                               dim3(UX * WAVE), 0, l.stream, a, nstrips);
    } else {
        const int nti = (a.mx + (UY - 2) - 1) / (UY - 2);
        const int ntj = (a.my + STRIP - 1) / STRIP;
        if constexpr (RP::NAUX == 0 && UY == 16) {
            // marching y phase (classic.hpp: unsplit_ym_kernel): segments of `seg` lines of 16 columns; enough
            // workgroups for ~4 rounds over the 256 CUs, warm-up step of a segment <= 1/8 of its work
            const int nlines = (a.mx + 15) / 16;
            int nseg = (1024 + ntj - 1) / ntj;
            if (nseg > (nlines + 7) / 8) nseg = (nlines + 7) / 8;
            if (nseg < 1) nseg = 1;
            const int seg = (nlines + nseg - 1) / nseg;
            nseg = (nlines + seg - 1) / seg;
            // a small grid cannot give every CU two marching workgroups (1024^2: 18 bands x 8 segments = 144; 2048^2: 560): the tile
            // kernel's many independent workgroups are the better shape there (C2, acoustics 1024^2: 103 vs 131 us per step; 2048^2: 240 vs 249; 4096^2: 731 vs 702, same box)
            const bool big = (long)ntj * nseg >= 1024;
            if (big && a.mcapa <= 0 && (a.src_id == 0 || std::is_same<RP, Euler5>::value)) {
                // wavefronts per workgroup: 8 (two slices each per step, 256 VGPRs: no spills) for the register-heavy
                // Euler core, 16 for the small systems
                constexpr int NWY = RP::MEQN >= 5 ? 8 : 16;
                if (a.src_id != 0) {
                    if constexpr (std::is_same<RP, Euler5>::value)
                        hipLaunchKernelGGL((unsplit_ym_kernel<RP, false, true, NWY>), dim3((unsigned)ntj * nseg),
                                           dim3(NWY * WAVE), 0, l.stream, a, ntj, seg, qx);
                } else
                    hipLaunchKernelGGL((unsplit_ym_kernel<RP, IsFwave<RP>::value, false, NWY>), dim3((unsigned)ntj * nseg),
                                       dim3(NWY * WAVE), 0, l.stream, a, ntj, seg, qx);
                hipError_t e = hipGetLastError();
                if (e != hipSuccess) return hip_fail(err, "unsplit y (marching) launch", e);
                return PCL_OK;
            }
        }
        if (a.src_id != 0) {       // fused source term: Euler solver without a capacity function
            if constexpr (std::is_same<RP, Euler5>::value) {
                if (a.src_id != 1 || a.mcapa > 0) { err = "fused source: Euler radial source, no capacity function"; return PCL_EINVAL; }
                hipLaunchKernelGGL((unsplit_y_kernel<RP, false, UY, false, true>), dim3((unsigned)nti * ntj),
                                   dim3(UY * WAVE), 0, l.stream, a, nti, qx);
            } else {
                err = "fused source: only the Euler solver has it";
                return PCL_EINVAL;
            }
        } else if (a.mcapa > 0)
            hipLaunchKernelGGL((unsplit_y_kernel<RP, IsFwave<RP>::value, UY, true>), dim3((unsigned)nti * ntj),
                               dim3(UY * WAVE), 0, l.stream, a, nti, qx);
        else
            hipLaunchKernelGGL((unsplit_y_kernel<RP, IsFwave<RP>::value, UY>), dim3((unsigned)nti * ntj),
                               dim3(UY * WAVE), 0, l.stream, a, nti, qx);
    }
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "unsplit launch", e);
}
template <class RP> int launch_unsplit_t(const SweepLaunch &l, const double *qx, std::string &err) {
    // slices per workgroup in the x / y phase.  16 wavefronts per workgroup leave 128 VGPRs per lane.  The Euler kernels
    // spill ~20 registers there and are still 4 % faster than with 12 wavefronts (170 VGPRs, no spills) -- except with a
    // capacity function, where the spill stores reach HBM (2.4 GB written per x launch at 4096^2 for 0.67 GB of results,
    // profiles/r02_pmc_hbm.json) at equal speed: 12 there.  The sphere solver (9 + 27 aux values per lane) takes 8.
    if constexpr (RP::NAUX >= 9) return launch_unsplit_u<RP, 8, 8>(l, qx, err);
    else if constexpr (RP::MEQN >= 5) {
        if (l.a.mcapa > 0) return launch_unsplit_u<RP, 12, 12>(l, qx, err);
        return launch_unsplit_u<RP, 16, 16>(l, qx, err);
    } else return launch_unsplit_u<RP, 16, 16>(l, qx, err);
}
// A user-written Riemann solver with a transverse body (cellrp.hpp): l.user_fn is unsplit_x_kernel<UserRp, FWAVE, U, CAPA>
// or unsplit_y_kernel<UserRp, FWAVE, U, CAPA, false> of the module compiled at run time, FWAVE and CAPA the form of l.user,
// U = l.user.slices(); the parameters and grids are those of launch_unsplit_u.  Always the tile form of the y phase: the
// marching kernel stays with the built-in solvers.
int launch_unsplit_user(const SweepLaunch &l, const double *qx, std::string &err) {
    const int U = l.user.slices();
    if (!l.user_fn || U < 3) {
        err = "user-written Riemann solver: no compiled solver with a transverse body is attached (pcl_cellrp_attach)";
        return PCL_ESTATE;
    }
    if (l.a.src_id != 0 || l.a.sub != 0) {
        err = "user-written Riemann solver, unsplit step: no fused source, whole blocks";
        return PCL_EINVAL;
    }
    if (int rc = user_form_check(l, err)) return rc;
    SweepArgs a = l.a;
    hipError_t e;
    if (l.ids == 1) {
        int nstrips = (a.mx + STRIP - 1) / STRIP;
        const int ntr = (a.my + (U - 2) - 1) / (U - 2);
        void *params[] = {&a, &nstrips};
        e = hipModuleLaunchKernel(l.user_fn, (unsigned)nstrips * ntr, 1, 1, (unsigned)U * WAVE, 1, 1, 0, l.stream, params, nullptr);
    } else {
        int nti = (a.mx + (U - 2) - 1) / (U - 2);
        const int ntj = (a.my + STRIP - 1) / STRIP;
        void *params[] = {&a, &nti, &qx};
        e = hipModuleLaunchKernel(l.user_fn, (unsigned)nti * ntj, 1, 1, (unsigned)U * WAVE, 1, 1, 0, l.stream, params, nullptr);
    }
    return e == hipSuccess ? PCL_OK : hip_fail(err, "unsplit launch (user-written Riemann solver)", e);
}
}  // namespace

int launch_unsplit(const SweepLaunch &l, const double *qx, std::string &err) {
    if (l.rp == PCL_RP_CELL) return launch_unsplit_user(l, qx, err);
    const RpFacts *f = Solvers::facts(l.rp);       // the flag follows the solver, among those this step has
    if ((l.fwave != 0) != (f && f->ndim == 2 && f->fwave))
        return not_built(err, "solver.fwave must be True for an f-wave Riemann solver and only for one");
    const int rc = Solvers::with(l.rp, [&](auto tag) {
        using RP = typename decltype(tag)::type;
        if constexpr (RP::NDIM == 2) return launch_unsplit_t<RP>(l, qx, err);
        else return RP_NONE;
    });
    return rc != RP_NONE ? rc : not_built(err, "Riemann solver id is not a 2-D solver");
}

// SharpClaw: dq of one direction (x writes dq, y accumulates)
namespace {
// The grid of sharp_kernel<., ixy, ., ., K> with ta strips per tile over a, the same for every solver, built in or compiled
// at run time; the tile subset of a decomposed x pass gets its box here (a.sub is dropped where there is none).
struct SharpGrid { unsigned nblocks; int ntiles_across, ntiles_along; };
SharpGrid sharp_grid(SweepArgs &a, int ixy, int K, int ta) {
    const int SH = K, SS = sstrip(K);
    if (ixy == 1 && a.sub != 0) {
        // x-pass tiles whose 16 rows x 64 cells lie inside the interior: rows 16*tb .. +15 within [mbc, mbc+my), cells
        // mbc-K+SS*ta .. +63 within [mbc, mbc+mx)
        a.box[0] = (a.mbc + T_ACROSS_S - 1) / T_ACROSS_S;
        a.box[1] = a.mbc + a.my >= T_ACROSS_S ? (a.mbc + a.my - T_ACROSS_S) / T_ACROSS_S + 1 : 0;
        a.box[2] = 1;
        a.box[3] = a.mx >= WAVE - SH ? (a.mx - (WAVE - SH)) / SS + 1 : 0;
    } else a.sub = 0;
    const int n_across = ixy == 1 ? a.J : a.I + (LINE - a.mbc);
    const int m_along = ixy == 1 ? a.mx : a.my;
    SharpGrid g;
    g.ntiles_across = (n_across + ta - 1) / ta;
    g.ntiles_along = (m_along + SS - 1) / SS;
    g.nblocks = (unsigned)g.ntiles_across * (unsigned)g.ntiles_along;
    return g;
}
// sharp1w_kernel: strips of sstrip(3) cells, four to a workgroup
struct Sharp1wGrid { unsigned nblocks; int nstrips; };
Sharp1wGrid sharp1w_grid(const SweepArgs &a) {
    const int nstrips = (a.mx + sstrip(3) - 1) / sstrip(3);
    return {(unsigned)((nstrips + 3) / 4), nstrips};
}

template <class RP, int IXY, int K> int launch_sharp_k(const SweepLaunch &l, std::string &err) {
    SweepArgs a = l.a;
    const SharpGrid g = sharp_grid(a, IXY, K, sharp_tile_across<RP, IXY>());
    const int ntiles_across = g.ntiles_across, ntiles_along = g.ntiles_along;
    const dim3 grid(g.nblocks);
    const bool capa = a.mcapa > 0;
#define PCL_SHARP_LAUNCH(CAPA_, LIM_)                                                                  \
    hipLaunchKernelGGL((sharp_kernel<RP, IXY, CAPA_, LIM_, K>), grid, dim3(256), 0, l.stream, a, ntiles_across, \
                       ntiles_along)
    if (a.src_id != 0) {
        // deltaq += dq_src inside the last pass: built for the shock-bubble configuration only
        if constexpr (std::is_same<RP, Euler5>::value && IXY == 2 && K == 3) {
            if (a.src_id != 1 || capa || l.lim_type != 2) { err = "SharpClaw: the fused dq source needs euler_5wave_2d, WENO5 (lim_type 2), no capacity function"; return PCL_EINVAL; }
            hipLaunchKernelGGL((sharp_kernel<RP, IXY, false, 2, K, true>), grid, dim3(256), 0, l.stream, a, ntiles_across,
                               ntiles_along);
            hipError_t e = hipGetLastError();
            return e == hipSuccess ? PCL_OK : hip_fail(err, "sharp launch", e);
        } else {
            err = "SharpClaw: the fused dq source needs euler_5wave_2d, WENO5 (lim_type 2), no capacity function";
            return PCL_EINVAL;
        }
    }
    if constexpr (K > 3) {
        if (l.lim_type != 2) { err = "SharpClaw: weno_order > 5 needs lim_type 2"; return PCL_EINVAL; }
        if (capa) PCL_SHARP_LAUNCH(true, 2); else PCL_SHARP_LAUNCH(false, 2);
    } else {
        if (l.lim_type == 1) { if (capa) PCL_SHARP_LAUNCH(true, 1); else PCL_SHARP_LAUNCH(false, 1); }
        else if (l.lim_type == 2) { if (capa) PCL_SHARP_LAUNCH(true, 2); else PCL_SHARP_LAUNCH(false, 2); }
        else if (l.lim_type == 3) { if (capa) PCL_SHARP_LAUNCH(true, 3); else PCL_SHARP_LAUNCH(false, 3); }
        else { err = "SharpClaw: lim_type must be 1 (tvd2), 2 (WENO5) or 3 (legacy WENO5)"; return PCL_EINVAL; }
    }
#undef PCL_SHARP_LAUNCH
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "sharp launch", e);
}
// mbc = (weno_order+1)/2 (sharpclaw.py:479).  HIGH = this solver also has the kernels of weno_order 7..17 (mbc 4..9):
// the 1-D solvers, 2-D advection, acoustics and Euler; the others are built for mbc = 3 only.
template <class RP, int IXY, bool HIGH> int launch_sharp_t(const SweepLaunch &l, std::string &err) {
    if (l.a.mbc == 3) return launch_sharp_k<RP, IXY, 3>(l, err);
    if constexpr (HIGH) {
        switch (l.a.mbc) {
        case 4: return launch_sharp_k<RP, IXY, 4>(l, err);
        case 5: return launch_sharp_k<RP, IXY, 5>(l, err);
        case 6: return launch_sharp_k<RP, IXY, 6>(l, err);
        case 7: return launch_sharp_k<RP, IXY, 7>(l, err);
        case 8: return launch_sharp_k<RP, IXY, 8>(l, err);
        case 9: return launch_sharp_k<RP, IXY, 9>(l, err);
        }
        err = "SharpClaw: mbc must be 3..9 (weno_order 5..17)";
        return PCL_EINVAL;
    }
    err = "SharpClaw: this Riemann solver is built for weno_order 5 (mbc 3) only; orders 7..17 exist for the 1-D solvers "
          "and for advection_2d, acoustics_2d, euler_5wave_2d";
    return PCL_EINVAL;
}
}  // namespace

namespace {
template <class RP> int launch_sharp1w(const SweepLaunch &l, std::string &err) {
    const SweepArgs &a = l.a;
    const Sharp1wGrid g = sharp1w_grid(a);
    const int nstrips = g.nstrips;
    const dim3 grid(g.nblocks);
    const bool capa = a.mcapa > 0;
#define PCL_SHARP1W_LAUNCH(LIM_, CAPA_) \
    hipLaunchKernelGGL((sharp1w_kernel<RP, LIM_, CAPA_>), grid, dim3(256), 0, l.stream, a, nstrips)
    if (l.lim_type == 1) { if (capa) PCL_SHARP1W_LAUNCH(1, true); else PCL_SHARP1W_LAUNCH(1, false); }
    else { if (capa) PCL_SHARP1W_LAUNCH(2, true); else PCL_SHARP1W_LAUNCH(2, false); }
#undef PCL_SHARP1W_LAUNCH
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "sharp (wave-based) launch", e);
}
}  // namespace

namespace {
// A user-written Riemann solver under SharpClaw (cellrp.hpp): l.user_fn is sharp_kernel<UserRp, ids, CAPA, LIM, K> or, with
// char_decomp = 1, sharp1w_kernel<UserRp, LIM, CAPA> of the module compiled at run time -- one (LIM, K, char_decomp), the
// ones of l.user, with CAPA its form's -- so this launch must ask for exactly that; the parameters and grids are those of
// launch_sharp_k / launch_sharp1w.  Whole blocks, no fused dq source.
int launch_sharp_user(const SweepLaunch &l, std::string &err) {
    const CellrpSpec &u = l.user;
    if (!l.user_fn || !u.sharp()) {
        err = "user-written Riemann solver: no solver compiled for SharpClaw is attached (pcl_cellrp_compile_sharp, pcl_create_cellrp)";
        return PCL_ESTATE;
    }
    if (l.a.src_id != 0 || l.a.sub != 0) {
        err = "user-written Riemann solver under SharpClaw: no fused dq source, whole blocks";
        return PCL_EINVAL;
    }
    if (int rc = user_form_check(l, err)) return rc;
    if (l.lim_type != u.lim_type) {
        err = "user-written Riemann solver: the attached solver was compiled for lim_type " + std::to_string(u.lim_type) +
              " and the stage asks for lim_type " + std::to_string(l.lim_type);
        return PCL_EINVAL;
    }
    if (l.a.mbc != u.mbc()) {
        err = "user-written Riemann solver: the attached solver was compiled for weno_order " + std::to_string(u.weno_order) +
              " (mbc " + std::to_string(u.mbc()) + ") and the stage runs with mbc " + std::to_string(l.a.mbc);
        return PCL_EINVAL;
    }
    if (l.char_decomp != u.char_decomp) {
        err = "user-written Riemann solver: the attached solver was compiled for char_decomp " + std::to_string(u.char_decomp) +
              " and the stage asks for char_decomp " + std::to_string(l.char_decomp);
        return PCL_EINVAL;
    }
    SweepArgs a = l.a;
    hipError_t e;
    if (l.char_decomp == 1) {
        if (l.ndim != 1 || l.a.mbc != 3) { err = "SharpClaw char_decomp = 1: 1-D, mbc 3"; return PCL_EINVAL; }
        Sharp1wGrid g = sharp1w_grid(a);
        void *params[] = {&a, &g.nstrips};
        e = hipModuleLaunchKernel(l.user_fn, g.nblocks, 1, 1, 256, 1, 1, 0, l.stream, params, nullptr);
    } else {
        const int ixy = l.ndim == 1 ? 1 : l.ids;
        SharpGrid g = sharp_grid(a, ixy, u.mbc(), sharp_tile_across_n(ixy, u.naux));
        void *params[] = {&a, &g.ntiles_across, &g.ntiles_along};
        e = hipModuleLaunchKernel(l.user_fn, g.nblocks, 1, 1, 256, 1, 1, 0, l.stream, params, nullptr);
    }
    return e == hipSuccess ? PCL_OK : hip_fail(err, "sharp launch (user-written Riemann solver)", e);
}
}  // namespace

int launch_sharp(const SweepLaunch &l, std::string &err) {
    if (l.rp == PCL_RP_CELL) return launch_sharp_user(l, err);
    const RpFacts *f = Solvers::facts(l.rp);       // the flag follows the solver, among those with SharpClaw kernels
    if ((l.fwave != 0) != (f && f->sharp && f->fwave))
        return not_built(err, "solver.fwave must be True for an f-wave Riemann solver and only for one");
    if (l.char_decomp == 1) {
        // 1d/sharpclaw/flux1.f90:80-107 (the 2-D flux1.f90 calls rpn2 with a wrong argument list there and cannot run)
        if (l.ndim != 1 || l.a.mbc != 3 || (l.lim_type != 1 && l.lim_type != 2) || l.fwave || l.a.src_id != 0)
            return not_built(err, "SharpClaw char_decomp = 1: 1-D, lim_type 1 (tvd2_wave) or 2 (weno5_wave), mbc 3, no f-wave solver");
        const int rc = Solvers::with(l.rp, [&](auto tag) {
            using RP = typename decltype(tag)::type;
            if constexpr (RP::SHARP_WAVE) return launch_sharp1w<RP>(l, err);
            else return RP_NONE;
        });
        return rc != RP_NONE ? rc
                             : not_built(err, "SharpClaw char_decomp = 1: advection, colour equation, acoustics, Burgers, Euler, shallow water in 1-D");
    }
    const int rc = Solvers::with(l.rp, [&](auto tag) {
        using RP = typename decltype(tag)::type;
        if constexpr (RP::SHARP && RP::NDIM == 1) return l.ndim == 1 ? launch_sharp_t<RP, 1, RP::SHARP_HIGH>(l, err) : RP_NONE;
        else if constexpr (RP::SHARP && RP::NDIM == 2)
            return l.ndim == 1 ? RP_NONE
                 : l.ids == 1 ? launch_sharp_t<RP, 1, RP::SHARP_HIGH>(l, err) : launch_sharp_t<RP, 2, RP::SHARP_HIGH>(l, err);
        else return RP_NONE;
    });
    return rc != RP_NONE ? rc : not_built(err, "Riemann solver id does not match the grid dimension");
}

int launch_rk(const RkLaunch &r, hipStream_t stream, std::string &err) {
    RkOp o;
    o.d = r.d; o.a = r.a; o.b = r.b; o.c = r.c; o.ca = r.ca; o.cb = r.cb; o.cc = r.cc; o.n = r.n; o.op = r.op;
    hipLaunchKernelGGL(rk_kernel, dim3(2048), dim3(256), 0, stream, o);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "rk launch", e);
}

#if !PCL_FAST
__global__ void shift_test_kernel(const double *in, double *l, double *r) {
    const int t = threadIdx.x;
    const double x = in[t];
    l[t] = from_left(x);
    r[t] = from_right(x);
}
void launch_shift_test(const double *in, double *l, double *r) {
    hipLaunchKernelGGL(shift_test_kernel, dim3(1), dim3(64), 0, 0, in, l, r);
}
#endif

}  // namespace PCL_NS
}  // namespace pcl
