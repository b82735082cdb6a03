// kernels.hip -- the sweep kernels + their launch code, compiled ONCE PER ARITHMETIC MODE:
//   -DPCL_NS=exact -DPCL_FAST=0 -ffp-contract=off   bit-identical to the reference (no FMA,
//                                                   correctly rounded divide/sqrt)
//   -DPCL_NS=fast  -DPCL_FAST=1 -ffp-contract=fast  FMA contraction + reciprocal-multiply
//                                                   division; checked at rtol 1e-12
// Distinct namespaces keep the two sets of template instantiations apart at link time.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>

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

// One launch, stated once: the grid, the block, the stream and the kernel's arguments as a tuple of the kernel's own parameter
// types.  fire() sends it to a kernel of this file -- A... is deduced from the kernel's function type, so a plan that does
// not match the kernel's signature does not compile -- or to a function of the module of a user-written Riemann solver
// (cellrp.hpp): an instantiation of the same kernel template, so its parameters are the ones the built-in launch was checked
// against.  Each kernel family has one function that fills its plan, for the built-in and the user launcher alike.
// grid.x == 0: nothing to launch.
template <class... A> struct Plan { dim3 grid, block; hipStream_t stream; std::tuple<A...> args; };
template <class... A> hipError_t fire(void (*kern)(A...), Plan<A...> &p) {
    std::apply([&](A &...a) { hipLaunchKernelGGL(kern, p.grid, p.block, 0, p.stream, a...); }, p.args);
    return hipGetLastError();
}
template <class... A> hipError_t fire(hipFunction_t f, Plan<A...> &p) {
    return std::apply([&](A &...a) {
        void *params[] = {(void *)&a...};
        return hipModuleLaunchKernel(f, p.grid.x, p.grid.y, p.grid.z, p.block.x, p.block.y, p.block.z, 0, p.stream, params, nullptr);
    }, p.args);
}
int launched(hipError_t e, const char *what, std::string &err) { return e == hipSuccess ? PCL_OK : hip_fail(err, what, e); }
// a run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{})
template <class F> auto with_flag(bool on, F &&f) { return on ? f(std::true_type{}) : f(std::false_type{}); }

using SweepPlan = Plan<SweepArgs, int, int>;    // sweep_kernel, sweep3_kernel, sharp_kernel: (a, tiles across, tiles along)
using StripPlan = Plan<SweepArgs, int>;         // unsplit_x_kernel, sharp1w_kernel: (a, strips)

// sweep_kernel<., IXY, ., ., DIM1> over l.a
template <int IXY, bool DIM1> int sweep_plan(const SweepLaunch &l, SweepPlan &p, std::string &err) {
    using T = TileShape<IXY>;
    const SweepArgs &a = l.a;
    const int n_across = IXY == 1 ? a.J : a.I + (LINE - a.mbc);  // y: columns counted from the line boundary
    const int m_along = IXY == 1 ? a.mx : a.my;
    const int ntiles_across = (n_across + T::ACROSS - 1) / T::ACROSS;
    const int ntiles_along = (m_along + T::NSTRIP * STRIP - 1) / (T::NSTRIP * STRIP);
    unsigned nblocks = (unsigned)ntiles_across * (unsigned)ntiles_along;
    if (a.sub != 0) {
        if (IXY != 1 || DIM1 || a.box[0] < 0 || a.box[1] > ntiles_across || a.box[2] < 0 ||
            a.box[3] > ntiles_along || a.box[0] >= a.box[1] || a.box[2] >= a.box[3]) {
            err = "tile subset: bad box";
            return PCL_EINVAL;
        }
        const unsigned inside = (unsigned)(a.box[1] - a.box[0]) * (unsigned)(a.box[3] - a.box[2]);
        nblocks = a.sub == 1 ? inside : nblocks - inside;
    }
    p = {dim3(nblocks), dim3(256), l.stream, {a, ntiles_across, ntiles_along}};
    return PCL_OK;
}

// ---- what every launch of a user-written Riemann solver (rp == PCL_RP_CELL, cellrp.hpp) checks -------------------------
// the kernel in `slot` of the attached module (sweep_args.hpp: CellrpSlot); null: nothing attached, or no such kernel in it
hipFunction_t user_kernel(const SweepLaunch &l, int slot) {
    return l.user_fns && slot >= 0 && slot < CELLRP_NSLOTS ? l.user_fns[slot] : nullptr;
}
int sweep_slot(int ids) { return ids >= 1 && ids <= 3 ? SLOT_SWEEP_X + ids - 1 : -1; }
const char *const USER_NONE = "user-written Riemann solver: no compiled solver is attached (pcl_cellrp_attach)";
const char *const USER_NO_SRC = "user-written Riemann solver: no fused source";
// What a family asks beyond the form: the refusal where no kernel of the family is attached (PCL_ESTATE); the noun by which a
// classic family refuses a SharpClaw handle (null: the family's `have` test covers it); the refusal of a fused source -- and,
// for a family of whole blocks, of a tile subset.
struct UserFamily { const char *none, *classic, *src; bool whole; };
// have: a kernel in the family's slot, of a handle compiled for the family.  handle, step: a refusal of the family's own
// about the handle / the step's geometry, found by the caller (null: none), in its place in the order.  Then the form: the
// kernel's FWAVE and CAPA are template flags (cellrp.hpp: the handle's form), so a launch that says otherwise would run the
// wrong kernel.
int user_check(const SweepLaunch &l, bool have, const UserFamily &fam, std::string &err, const char *handle = nullptr,
               const char *step = nullptr) {
    const CellrpSpec &u = l.user;
    const auto no = [&err](const std::string &why) { err = why; return PCL_EINVAL; };
    if (!have) { err = fam.none; return PCL_ESTATE; }
    if (fam.classic && u.sharp())
        return no(std::string("user-written Riemann solver: the attached solver was compiled for SharpClaw and holds no classic ") + fam.classic);
    if (handle) return no(handle);
    if (l.a.src_id != 0 || (fam.whole && l.a.sub != 0)) return no(fam.src);
    if (step) return no(step);
    if ((l.fwave != 0) != u.fwave())
        return no(u.fwave() ? "user-written Riemann solver: the attached solver was compiled for f-waves and the step is in wave form"
                            : "user-written Riemann solver: the step asks for f-waves and the attached solver was compiled in wave form");
    if ((l.a.mcapa > 0) != u.capa())
        return no(u.capa() ? "user-written Riemann solver: the attached solver was compiled for a capacity function and the step has none"
                           : "user-written Riemann solver: the step has a capacity function and the attached solver was compiled without one");
    if ((u.naux > 0 || u.capa()) && !l.a.aux)
        return no(u.naux > 0 ? "user-written Riemann solver: this solver reads aux arrays and there are none (pcl_put_aux)"
                             : "user-written Riemann solver: the capacity function is a component of the aux arrays and there are none (pcl_put_aux)");
    return PCL_OK;
}

// sweep_kernel<UserRp, IXY, CAPA, FWAVE, DIM1> of the attached module
template <int IXY, bool DIM1> int launch_user(const SweepLaunch &l, std::string &err) {
    const hipFunction_t f = user_kernel(l, IXY == 1 ? SLOT_SWEEP_X : SLOT_SWEEP_Y);
    if (int rc = user_check(l, f != nullptr, {USER_NONE, "sweep", USER_NO_SRC, false}, err)) return rc;
    SweepPlan p;
    if (int rc = sweep_plan<IXY, DIM1>(l, p, err)) return rc;
    if (p.grid.x == 0) return PCL_OK;
    return launched(fire(f, p), "sweep launch (user-written Riemann solver)", err);
}

template <class RP, int IXY, bool DIM1> int launch(const SweepLaunch &l, std::string &err) {
    const SweepArgs &a = l.a;
    SweepPlan p;
    if (int rc = sweep_plan<IXY, DIM1>(l, p, err)) return rc;
    if (p.grid.x == 0) return PCL_OK;
    constexpr bool FW = IsFwave<RP>::value;       // f-wave solvers run the flux2fw.f / step1fw.f form of the kernel
    if ((l.fwave != 0) != FW) {
        err = FW ? "this Riemann solver returns f-waves: set solver.fwave = True (classic1fw / classic2fw)"
                 : "solver.fwave = True needs an f-wave Riemann solver (elasticity_fwave_1d, psystem_fwave_2d)";
        return PCL_EINVAL;
    }
    if (a.src_id != 0) {      // fused source term: its own instantiation (classic.hpp), Euler y pass without capa
        if constexpr (IXY == 2 && !DIM1 && std::is_same<RP, Euler5>::value) {
            if (a.src_id != 1 || a.mcapa > 0) { err = "fused source: Euler radial source, no capacity function"; return PCL_EINVAL; }
            return launched(fire(sweep_kernel<RP, IXY, false, FW, DIM1, true>, p), "sweep launch", err);
        } else {
            err = "fused source: only the y pass of the Euler solver has it";
            return PCL_EINVAL;
        }
    }
    return launched(with_flag(a.mcapa > 0, [&](auto C) { return fire(sweep_kernel<RP, IXY, decltype(C)::value, FW, DIM1>, p); }),
                    "sweep launch", err);
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
// step2ds_kernel<., ., ., .> over l: what a one-kernel launch asks of l whatever the solver, built in or compiled at run time
// (naux: the aux components its normal solver reads), the grid of ntx x nty tiles and the kernel's thirteen arguments.
using Step2dsPlan = Plan<SweepArgs, int, int, unsigned *, double2 *, const int *, const TileNext *, unsigned *, unsigned,
                         unsigned *, int, unsigned *, int>;
int step2ds_plan(const SweepLaunch &l, int naux, Step2dsPlan &p, std::string &err) {
    const SweepArgs &a = l.a;
    if (a.mbc != HALO) { err = "step2ds kernel: mbc = 2"; return PCL_EINVAL; }
    const bool capa = a.mcapa > 0;
    if ((capa || naux > 0) && !a.aux) { err = "step2ds kernel: this solver reads aux arrays and there are none"; return PCL_EINVAL; }
    // quiet tiles: the bookkeeping of the aux-free instantiations without a capacity function only (classic_fused.hpp)
    if ((capa || naux > 0) && (l.tq_out || l.tq_list)) { err = "step2ds kernel: no quiet-tile bookkeeping with aux arrays"; return PCL_EINVAL; }
    const int ntx = (a.mx + F_OWN_C - 1) / F_OWN_C, nty = (a.my + F_OWN_R - 1) / F_OWN_R;
    unsigned nblocks = (unsigned)ntx * (unsigned)nty;
    if (a.sub != 0) {
        if (a.box[0] < 0 || a.box[1] > nty || a.box[2] < 0 || a.box[3] > ntx || a.box[0] >= a.box[1] || a.box[2] >= a.box[3]) {
            err = "step2ds tile subset: bad box";
            return PCL_EINVAL;
        }
        const unsigned inside = (unsigned)(a.box[1] - a.box[0]) * (unsigned)(a.box[3] - a.box[2]);
        nblocks = a.sub == 1 ? inside : nblocks - inside;
    }
    p = {dim3(nblocks), dim3(F_THREADS), l.stream,
         {a, ntx, nty, l.tq_out, l.tq_cfl, l.tq_list, l.tq_next, l.tq_ring, l.ring_seq, l.tq_reuse, l.rowreuse, l.tq_ycol, l.ycol}};
    if (a.sub != 0 && nblocks == 0) return PCL_OK;       // the tile subset is empty
    // a list launch: the tiles the hand-over+list kernel behind the previous launch listed (classic_fused.hpp); one
    // workgroup per tile of the grid, those past the list's end return at once
    const bool list = l.tq_list != nullptr;
    if ((list && (a.sub != 0 || !l.tq_out || !l.tq_cfl || !l.tq_next)) || (l.tq_ring && !list)) {
        err = "step2ds tile list: the whole block, with its bookkeeping";
        return PCL_EINVAL;
    }
    return PCL_OK;
}

// step2ds_kernel<UserRp, FWAVE, false, CAPA> of a module compiled with the one-kernel step (cellrp.hpp: spec.onek)
int launch_step2ds_user(const SweepLaunch &l, std::string &err) {
    const hipFunction_t f = user_kernel(l, SLOT_ONEK);
    const UserFamily fam = {"user-written Riemann solver: no solver compiled with the one-kernel step is attached (pcl_cellrp_compile_onek, pcl_cellrp_attach)",
                            "step", USER_NO_SRC, false};
    if (int rc = user_check(l, f && l.user.onek, fam, err)) return rc;
    Step2dsPlan p;
    if (int rc = step2ds_plan(l, l.user.naux, p, err)) return rc;
    if (p.grid.x == 0) return PCL_OK;
    return launched(fire(f, p), "step2ds launch (user-written Riemann solver)", err);
}

template <class RP> int launch_step2ds_t(const SweepLaunch &l, std::string &err) {
    const SweepArgs &a = l.a;
    constexpr bool FW = IsFwave<RP>::value;
    if ((l.fwave != 0) != FW) { err = "solver.fwave does not match the Riemann solver"; return PCL_EINVAL; }
    Step2dsPlan p;
    if (int rc = step2ds_plan(l, RP::NAUX, p, err)) return rc;
    if (p.grid.x == 0) return PCL_OK;
    const bool capa = a.mcapa > 0;
    if (a.src_id != 0 && !(std::is_same<RP, Euler5>::value && a.src_id == 1 && !capa)) {
        err = "fused source: only the Euler solver's radial source, no capacity function";
        return PCL_EINVAL;
    }
    hipError_t e = hipSuccess;
    if (a.src_id != 0) {
        if constexpr (std::is_same<RP, Euler5>::value) e = fire(step2ds_kernel<RP, FW, true>, p);
    } else
        e = with_flag(capa, [&](auto C) { return fire(step2ds_kernel<RP, FW, false, decltype(C)::value>, p); });
    return launched(e, "step2ds launch", err);
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

// sweep3_kernel<., DIR, .> over l.a, DIR = l.ids
namespace {
SweepPlan sweep3_plan(const SweepLaunch &l) {
    const SweepArgs &a = l.a;
    const int n_ac = l.ids == 1 ? a.n_ac : a.n_ac + (LINE - a.mbc);  // y, z: columns counted from the line boundary
    const int ac = l.ids == 1 ? Tile3Shape<1>::AC : Tile3Shape<2>::AC, adv = l.ids == 1 ? Tile3Shape<1>::ADV : Tile3Shape<2>::ADV;
    static_assert(Tile3Shape<3>::AC == Tile3Shape<2>::AC && Tile3Shape<3>::ADV == Tile3Shape<2>::ADV, "y and z: one tile shape");
    const int ntiles_ac = (n_ac + ac - 1) / ac, ntiles_al = (a.m_al + adv - 1) / adv;
    return {dim3((unsigned)ntiles_ac * (unsigned)ntiles_al, (unsigned)a.n_b), dim3(256), l.stream, {a, ntiles_ac, ntiles_al}};
}

// sweep3_kernel<UserRp, l.ids, CAPA> of a module compiled for the 3-D sweeps
int launch_sweep3_user(const SweepLaunch &l, std::string &err) {
    const hipFunction_t f = user_kernel(l, sweep_slot(l.ids));
    const char *handle = l.user.ndim != 3 ? "user-written Riemann solver: the attached solver was not compiled for the 3-D sweeps (pcl_cellrp_compile3)"
                         : (l.ids < 1 || l.ids > 3) ? "3-D sweep: direction must be 1, 2 or 3" : nullptr;
    if (int rc = user_check(l, f != nullptr, {USER_NONE, "sweep", USER_NO_SRC, false}, err, handle,
                            l.a.mbc != HALO ? "3-D sweep: mbc = 2" : nullptr))
        return rc;
    SweepPlan p = sweep3_plan(l);
    return launched(fire(f, p), "sweep3 launch (user-written Riemann solver)", err);
}
}  // namespace

// 3-D dimension-split sweep along direction l.ids (classic.hpp: sweep3_kernel)
int launch_sweep3(const SweepLaunch &l, std::string &err) {
    if (l.rp == PCL_RP_CELL) return launch_sweep3_user(l, err);
    if (l.fwave) { err = "fwave: no 3-D f-wave Riemann solver is built in"; return PCL_EINVAL; }
    if (l.rp != VcAcoustics3D::ID) { err = "Riemann solver id is not a 3-D solver"; return PCL_EINVAL; }
    SweepPlan p = sweep3_plan(l);
    using RP = VcAcoustics3D;
    const hipError_t e = with_flag(l.a.mcapa > 0, [&](auto C) {      // capacity function (step3ds.f:138-141,196-200)
        constexpr bool CAPA = decltype(C)::value;
        return l.ids == 1 ? fire(sweep3_kernel<RP, 1, CAPA>, p) : l.ids == 2 ? fire(sweep3_kernel<RP, 2, CAPA>, p) : fire(sweep3_kernel<RP, 3, CAPA>, p);
    });
    return launched(e, "sweep3 launch", err);
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

// The general unsplit 3-D step of one direction around a user-written solver with rpt3 / rptt3 bodies (classic3.hpp):
// pieces3_kernel<UserRp, DIR> of the attached module, then the library's gather3_kernel.  One plan per kernel, stated once.
namespace {
using Pieces3Plan = Plan<SweepArgs, Slices3Args, Pieces3Args>;
using Gather3Plan = Plan<Gather3Args>;
int unsplit3_general_plans(const Unsplit3Launch &l, Pieces3Plan &pp, Gather3Plan &gp, std::string &err) {
    const SweepArgs &a = l.a;
    const auto no = [&err](const char *why) { err = why; return PCL_EINVAL; };
    if (l.dir < 1 || l.dir > 3) return no("unsplit 3-D step: direction must be 1, 2 or 3");
    if (a.mbc != HALO) return no("unsplit 3-D step: mbc = 2");
    if (!l.scratch) return no("unsplit 3-D step (user-written Riemann solver): no scratch planes were allocated");
    const int d = l.dir - 1, e = (d + 1) % 3, f = (d + 2) % 3;
    if (l.n3[d] != a.n_al || l.n3[e] != l.n_e || l.n3[f] != l.n_f) return no("unsplit 3-D step: the scratch extents are not the block's");
    if (((long)a.m_al / STRIP + 1) * (l.m_e + 2) * (l.m_f + 2) > 0x7fffffffL || l.m_e > 65535 || l.m_f > 65535)
        return no("unsplit 3-D step: the block is too large for one launch");
    const long sc[3] = {1, (long)l.n3[0], (long)l.n3[0] * l.n3[1]};
    const long cells = sc[2] * l.n3[2];
    Slices3Args t;
    t.s_e = l.s_e; t.s_f = l.s_f; t.n_e = l.n_e; t.n_f = l.n_f;
    t.lo_e = a.mbc - 1; t.hi_e = a.mbc + l.m_e; t.lo_f = a.mbc - 1; t.hi_f = a.mbc + l.m_f;
    t.m3 = l.m3; t.m4 = l.m4; t.dty = l.dty; t.dtz = l.dtz;
    Pieces3Args p;
    p.scr = l.scratch; p.s_al = sc[d]; p.s_e = sc[e]; p.s_f = sc[f]; p.cells = cells;
    const int nstrips = (a.m_al + STRIP - 1) / STRIP;
    const bool on_f = l.dir == 2;       // p3_waves_on_f: which transverse direction a workgroup's wavefronts lie along
    const int ge = on_f ? l.m_e + 2 : (l.m_e + 2 + P3_NW - 1) / P3_NW, gf = on_f ? (l.m_f + 2 + P3_NW - 1) / P3_NW : l.m_f + 2;
    static_assert(!p3_waves_on_f<1>() && p3_waves_on_f<2>() && !p3_waves_on_f<3>(), "the grid follows the kernel's wave axis");
    // (the fastest index runs along i in every direction: pieces3_kernel's b0, b1, b2)
    p.g0 = l.dir == 1 ? nstrips : l.dir == 2 ? gf : ge;
    p.g1 = l.dir == 3 ? gf : ge;
    p.g2 = l.dir == 1 ? gf : nstrips;
    pp = {dim3((unsigned)p.g0 * (unsigned)p.g1 * (unsigned)p.g2), dim3(WAVE * P3_NW), l.stream, {a, t, p}};
    Gather3Args g;
    g.scr = l.scratch; g.qsrc = l.dir == 1 ? a.qin : l.qacc; g.qacc = l.qacc;
    g.plane = a.plane;
    const long sq[3] = {a.s_al, l.s_e, l.s_f};      // (sweep, y-like, z-like) -> (x, y, z)
    const int mq[3] = {a.m_al, l.m_e, l.m_f};
    const int axis[3] = {d, e, f};
    for (int k = 0; k < 3; k++) { g.s[axis[k]] = sq[k]; g.m[axis[k]] = mq[k]; g.c[k] = sc[k]; }
    g.cells = cells; g.c_e = sc[e]; g.c_f = sc[f];
    g.mbc = a.mbc; g.meqn = l.user->meqn;
    g.dtd = a.dtd; g.dty = l.dty; g.dtz = l.dtz;
    gp = {dim3((unsigned)((g.m[0] + 255) / 256), (unsigned)g.m[1], (unsigned)g.m[2]), dim3(256), l.stream, {g}};
    return PCL_OK;
}

int launch_unsplit3_user(const Unsplit3Launch &l, std::string &err) {
    const auto no = [&err](const char *why) { err = why; return PCL_EINVAL; };
    const int slot = l.dir >= 1 && l.dir <= 3 ? SLOT_PIECES3_X + l.dir - 1 : -1;
    const hipFunction_t f = l.user_fns && l.user && slot >= 0 ? l.user_fns[slot] : nullptr;
    if (!f || !l.user->trans3) {
        err = "user-written Riemann solver: no solver compiled with rpt3 / rptt3 bodies is attached (pcl_cellrp_compile3t, pcl_cellrp_attach)";
        return PCL_ESTATE;
    }
    const CellrpSpec &u = *l.user;
    if (l.m4 > 0 && u.trans3 < 2) return no("user-written Riemann solver: the attached solver has no rptt3 body and method[2] asks for double-transverse terms");
    if (l.fwave || u.fwave()) return no("user-written Riemann solver: no f-waves in 3-D");
    if (l.a.mcapa > 0 || u.capa()) return no("3-D: capacity function not implemented in the unsplit step");
    if (l.a.src_id != 0) return no(USER_NO_SRC);
    if (u.naux > 0 && !l.a.aux) return no("user-written Riemann solver: this solver reads aux arrays and there are none (pcl_put_aux)");
    Pieces3Plan pp;
    Gather3Plan gp;
    if (int rc = unsplit3_general_plans(l, pp, gp, err)) return rc;
    if (l.dir == 1) {     // the first direction writes interior cells only: the ghost frame of the result := qold's
        const int I = l.a.n_al, J = l.n_e, K = l.n_f;
        hipLaunchKernelGGL(ghost3_copy_kernel, dim3((unsigned)((I + 255) / 256), (unsigned)J, (unsigned)K), dim3(256), 0,
                           l.stream, l.a.qin, l.qacc, u.meqn, l.a.plane, I, J, K, l.s_e, l.a.mbc);
    }
    if (int rc = launched(fire(f, pp), "pieces3 launch (user-written Riemann solver)", err)) return rc;
    return launched(l.dir == 2 ? fire(gather3_kernel<true>, gp) : fire(gather3_kernel<false>, gp), "gather3 launch", err);
}
}  // namespace

int launch_unsplit3(const Unsplit3Launch &l, std::string &err) {
    if (l.rp == PCL_RP_CELL) return launch_unsplit3_user(l, err);
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
// the same for the three passes of a 3-D SharpClaw stage (sharp3_kernel): one rule, meqn + capa + naux, set by the 16-strip tile
int sharp3_tile_max_planes() {
    static_assert(sizeof(double) * SHARP3_MAX_PLANES * sharp3_tile_across_n(1, 0) * WAVE <= 65536 &&
                  sizeof(double) * SHARP3_MAX_PLANES * sharp3_tile_across_n(2, 5) * WAVE <= 65536, "the 3-D SharpClaw tile fits 64 KB");
    return SHARP3_MAX_PLANES;
}
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
// The tile form of the two phases, U slices per workgroup: unsplit_x_kernel<., ., U, .> and unsplit_y_kernel<., ., U, ., .>
StripPlan unsplit_x_plan(const SweepArgs &a, int U, hipStream_t stream) {
    const int nstrips = (a.mx + STRIP - 1) / STRIP, ntr = (a.my + (U - 2) - 1) / (U - 2);
    return {dim3((unsigned)nstrips * ntr), dim3((unsigned)U * WAVE), stream, {a, nstrips}};
}
using UnsplitYPlan = Plan<SweepArgs, int, const double *>;      // (a, tiles along x, the x phase's result)
UnsplitYPlan unsplit_y_plan(const SweepArgs &a, int U, const double *qx, hipStream_t stream) {
    const int nti = (a.mx + (U - 2) - 1) / (U - 2), ntj = (a.my + STRIP - 1) / STRIP;
    return {dim3((unsigned)nti * ntj), dim3((unsigned)U * WAVE), stream, {a, nti, qx}};
}

template <class RP, int UX, int UY> int launch_unsplit_u(const SweepLaunch &l, const double *qx, std::string &err) {
    SweepArgs a = l.a;
    constexpr bool FW = IsFwave<RP>::value;
    hipError_t e;
    if (l.ids == 1) {
        if (a.sub != 0) {
            // tiles whose 64 cells x UX rows lie inside the interior: cells mbc-2+60*ta .. +63 within [mbc, mbc+mx),
            // rows mbc-1+(UX-2)*tr .. +UX-1 within [mbc, mbc+my)
            a.box[0] = 1;
            a.box[1] = a.my - UX + 1 >= 0 ? (a.my - UX + 1) / (UX - 2) + 1 : 0;
            a.box[2] = 1;
            a.box[3] = a.mx >= 62 ? (a.mx - 62) / STRIP + 1 : 0;
        }
        StripPlan p = unsplit_x_plan(a, UX, l.stream);
        e = with_flag(a.mcapa > 0, [&](auto C) { return fire(unsplit_x_kernel<RP, FW, UX, decltype(C)::value>, p); });
    } else {
        if constexpr (RP::NAUX == 0 && UY == 16) {
            // marching y phase (classic.hpp: unsplit_ym_kernel): segments of `seg` lines of 16 columns; enough
            // workgroups for ~4 rounds over the 256 CUs, warm-up step of a segment <= 1/8 of its work
            const int nlines = (a.mx + 15) / 16, ntj = (a.my + STRIP - 1) / STRIP;
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
                return launched(hipGetLastError(), "unsplit y (marching) launch", err);
            }
        }
        UnsplitYPlan p = unsplit_y_plan(a, UY, qx, l.stream);
        if (a.src_id != 0) {       // fused source term: Euler solver without a capacity function
            if constexpr (std::is_same<RP, Euler5>::value) {
                if (a.src_id != 1 || a.mcapa > 0) { err = "fused source: Euler radial source, no capacity function"; return PCL_EINVAL; }
                e = fire(unsplit_y_kernel<RP, false, UY, false, true>, p);
            } else {
                err = "fused source: only the Euler solver has it";
                return PCL_EINVAL;
            }
        } else
            e = with_flag(a.mcapa > 0, [&](auto C) { return fire(unsplit_y_kernel<RP, FW, UY, decltype(C)::value>, p); });
    }
    return launched(e, "unsplit launch", err);
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
// unsplit_x_kernel<UserRp, FWAVE, U, CAPA> or unsplit_y_kernel<UserRp, FWAVE, U, CAPA, false> of a module compiled with a
// transverse body, U = l.user.slices().  Always the tile form of the y phase: the marching kernel stays with the built-in
// solvers.
int launch_unsplit_user(const SweepLaunch &l, const double *qx, std::string &err) {
    const int U = l.user.slices();
    const hipFunction_t f = user_kernel(l, l.ids == 1 ? SLOT_UNSPLIT_X : SLOT_UNSPLIT_Y);
    const UserFamily fam = {"user-written Riemann solver: no compiled solver with a transverse body is attached (pcl_cellrp_attach)", nullptr,
                            "user-written Riemann solver, unsplit step: no fused source, whole blocks", true};
    if (int rc = user_check(l, f && U >= 3, fam, err)) return rc;
    hipError_t e;
    if (l.ids == 1) {
        StripPlan p = unsplit_x_plan(l.a, U, l.stream);
        e = fire(f, p);
    } else {
        UnsplitYPlan p = unsplit_y_plan(l.a, U, qx, l.stream);
        e = fire(f, p);
    }
    return launched(e, "unsplit launch (user-written Riemann solver)", err);
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
// sharp_kernel<., ixy, ., ., K> with ta strips per tile over l.a; the tile subset of a decomposed x pass gets its box here
// (a.sub is dropped where there is none).
SweepPlan sharp_plan(const SweepLaunch &l, int ixy, int K, int ta) {
    SweepArgs a = l.a;
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
    const int ntiles_across = (n_across + ta - 1) / ta, ntiles_along = (m_along + SS - 1) / SS;
    return {dim3((unsigned)ntiles_across * (unsigned)ntiles_along), dim3(256), l.stream, {a, ntiles_across, ntiles_along}};
}
// sharp3_kernel<., l.ids, ., ., K> with ta strips per tile over l.a: (tiles, batch), the batch index every k (x, y passes) or j
// (z pass) of the array -- the kernel leaves at once where that index is not swept
SweepPlan sharp3_plan(const SweepLaunch &l, int K, int ta) {
    const SweepArgs &a = l.a;
    const int n_across = l.ids == 1 ? a.n_ac : a.n_ac + (LINE - a.mbc);     // y, z: columns counted from the line boundary
    const int ntiles_across = (n_across + ta - 1) / ta, ntiles_along = (a.m_al + sstrip(K) - 1) / sstrip(K);
    return {dim3((unsigned)ntiles_across * (unsigned)ntiles_along, (unsigned)a.n_b), dim3(256), l.stream, {a, ntiles_across, ntiles_along}};
}
// sharp1w_kernel: strips of sstrip(3) cells, four to a workgroup
StripPlan sharp1w_plan(const SweepLaunch &l) {
    const int nstrips = (l.a.mx + sstrip(3) - 1) / sstrip(3);
    return {dim3((unsigned)((nstrips + 3) / 4)), dim3(256), l.stream, {l.a, nstrips}};
}

template <class RP, int IXY, int K> int launch_sharp_k(const SweepLaunch &l, std::string &err) {
    const SweepArgs &a = l.a;
    SweepPlan p = sharp_plan(l, IXY, K, sharp_tile_across<RP, IXY>());
    const bool capa = a.mcapa > 0;
    const auto go = [&](auto LIM) {
        return with_flag(capa, [&](auto C) { return fire(sharp_kernel<RP, IXY, decltype(C)::value, decltype(LIM)::value, K>, p); });
    };
    using std::integral_constant;
    hipError_t e;
    if (a.src_id != 0) {
        // deltaq += dq_src inside the last pass: built for the shock-bubble configuration only
        if constexpr (std::is_same<RP, Euler5>::value && IXY == 2 && K == 3) {
            if (a.src_id != 1 || capa || l.lim_type != 2) { err = "SharpClaw: the fused dq source needs euler_5wave_2d, WENO5 (lim_type 2), no capacity function"; return PCL_EINVAL; }
            e = fire(sharp_kernel<RP, IXY, false, 2, K, true>, p);
        } else {
            err = "SharpClaw: the fused dq source needs euler_5wave_2d, WENO5 (lim_type 2), no capacity function";
            return PCL_EINVAL;
        }
    } else if constexpr (K > 3) {
        if (l.lim_type != 2) { err = "SharpClaw: weno_order > 5 needs lim_type 2"; return PCL_EINVAL; }
        e = go(integral_constant<int, 2>{});
    } else {
        if (l.lim_type == 1) e = go(integral_constant<int, 1>{});
        else if (l.lim_type == 2) e = go(integral_constant<int, 2>{});
        else if (l.lim_type == 3) e = go(integral_constant<int, 3>{});
        else { err = "SharpClaw: lim_type must be 1 (tvd2), 2 (WENO5) or 3 (legacy WENO5)"; return PCL_EINVAL; }
    }
    return launched(e, "sharp launch", err);
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
    StripPlan p = sharp1w_plan(l);
    const auto go = [&](auto LIM) {
        return with_flag(l.a.mcapa > 0, [&](auto C) { return fire(sharp1w_kernel<RP, decltype(LIM)::value, decltype(C)::value>, p); });
    };
    const hipError_t e = l.lim_type == 1 ? go(std::integral_constant<int, 1>{}) : go(std::integral_constant<int, 2>{});
    return launched(e, "sharp (wave-based) launch", err);
}

// sharp_kernel<UserRp, ids, CAPA, LIM, K> or, with char_decomp = 1, sharp1w_kernel<UserRp, LIM, CAPA> of a module compiled for
// SharpClaw -- one (LIM, K, char_decomp), the ones of l.user, with CAPA its form's -- so this launch must ask for exactly
// that.  Whole blocks, no fused dq source.
int launch_sharp_user(const SweepLaunch &l, std::string &err) {
    const CellrpSpec &u = l.user;
    const hipFunction_t f = user_kernel(l, sweep_slot(l.ids));
    const UserFamily fam = {"user-written Riemann solver: no solver compiled for SharpClaw is attached (pcl_cellrp_compile_sharp, pcl_create_cellrp)", nullptr,
                            "user-written Riemann solver under SharpClaw: no fused dq source, whole blocks", true};
    if (int rc = user_check(l, f && u.sharp(), fam, err)) return rc;
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
    if ((l.ndim == 3) != (u.ndim == 3)) {
        err = u.ndim == 3 ? "user-written Riemann solver: the attached solver holds the 3-D SharpClaw kernels (pcl_cellrp_compile3_sharp) and the stage is not 3-D"
                          : "user-written Riemann solver: a 3-D SharpClaw stage needs a solver compiled by pcl_cellrp_compile3_sharp";
        return PCL_EINVAL;
    }
    hipError_t e;
    if (l.ndim == 3) {
        // sharp3_kernel<UserRp, ids, CAPA, LIM, K>: the fused Runge-Kutta store phase exists in the z pass alone
        if (l.ids < 1 || l.ids > 3 || l.char_decomp != 0 || (l.a.rk_op != 0 && l.ids != 3) || l.a.n_b < 1 || l.a.n_b > 65535) {
            err = "SharpClaw 3-D pass: direction 1..3, char_decomp 0, the Runge-Kutta combination in the z pass only, at most 65535 batch indices";
            return PCL_EINVAL;
        }
        SweepPlan p = sharp3_plan(l, u.mbc(), sharp3_tile_across_n(l.ids, u.naux));
        e = fire(f, p);
    } else if (l.char_decomp == 1) {
        if (l.ndim != 1 || l.a.mbc != 3) { err = "SharpClaw char_decomp = 1: 1-D, mbc 3"; return PCL_EINVAL; }
        StripPlan p = sharp1w_plan(l);
        e = fire(f, p);
    } else {
        const int ixy = l.ndim == 1 ? 1 : l.ids;
        SweepPlan p = sharp_plan(l, ixy, u.mbc(), sharp_tile_across_n(ixy, u.naux));
        e = fire(f, p);
    }
    return launched(e, "sharp launch (user-written Riemann solver)", err);
}
}  // namespace

int launch_sharp(const SweepLaunch &l, std::string &err) {
    if (l.rp == PCL_RP_CELL) return launch_sharp_user(l, err);
    if (l.ndim == 3)
        return not_built(err, "SharpClaw in 3-D: no kernel of a built-in Riemann solver is instantiated; it runs a solver compiled at "
                              "run time (pcl_cellrp_compile3_sharp, pcl_create_cellrp)");
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

// one instantiation per number of terms, so that the loads of an element are independent and unrolled
template <int... N>
static auto rk_lincomb_kernels(std::integer_sequence<int, N...>) {
    static void (*const table[])(RkLincomb) = {rk_lincomb_kernel<N>...};
    return table;
}
int launch_rk_lincomb(const RkLincombLaunch &r, hipStream_t stream, std::string &err) {
    if (!r.d || !r.a || r.n <= 0 || r.nterms < 0 || r.nterms > RK_LINCOMB_MAX) {
        err = "launch_rk_lincomb: bad arguments";
        return PCL_EINVAL;
    }
    RkLincomb o;
    o.d = r.d; o.a = r.a; o.n = r.n;
    const uintptr_t align = (uintptr_t)r.d & 15;
    bool same = ((uintptr_t)r.a & 15) == align && (align == 0 || align == 8);
    for (int t = 0; t < RK_LINCOMB_MAX; t++) {
        o.k[t] = t < r.nterms ? r.k[t] : r.a;
        o.c[t] = t < r.nterms ? r.c[t] : 0.0;
        if (t < r.nterms && (!r.k[t] || r.k[t] == r.d)) {
            err = "launch_rk_lincomb: a term is null or the destination";
            return PCL_EINVAL;
        }
        same = same && ((uintptr_t)o.k[t] & 15) == align;
    }
    o.head = !same ? -1 : align ? 1 : 0;
    // 16 bytes per thread and trip; at most 2048 workgroups (eight per CU), the rest by the grid stride
    const long pairs = (r.n + 1) / 2;
    const int blocks = (int)std::min<long>(2048, (pairs + 255) / 256);
    const auto table = rk_lincomb_kernels(std::make_integer_sequence<int, RK_LINCOMB_MAX + 1>());
    hipLaunchKernelGGL(table[r.nterms], dim3(blocks), dim3(256), 0, stream, o);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "rk_lincomb launch", e);
}

#if !PCL_FAST
// The second pass of a functional (sweep_args.hpp: ReduceFinal; the first is the run-time wrapper of cellfn.hpp).
// Workgroup m reduces output m.  The order is a function of npart alone: thread t folds partials t, t + 256, t + 512, ...
// in eight interleaved chains, each in ascending order, and adds the chains up in order; the wavefront combines its 64 values in a butterfly at distances 1, 2, ... 32, thread 0 combines the four
// wavefronts in order through LDS and stores out[m].  No atomics: the same partials give the same bits on every launch.
struct ReduceOps { int op[8]; };
__device__ __forceinline__ double reduce_combine(int op, double a, double b) {
    return op == PCL_REDUCE_MAX ? fmax(a, b) : op == PCL_REDUCE_MIN ? fmin(a, b) : a + b;
}
__global__ void __launch_bounds__(REDUCE_FINAL_THREADS) reduce_partials_kernel(const double *__restrict__ part,
                                                                               double *__restrict__ out, long npart,
                                                                               ReduceOps ops) {
    static_assert(REDUCE_FINAL_THREADS == 256, "four wavefronts of 64");
    __shared__ double wsum[REDUCE_FINAL_THREADS / 64];
    const int m = blockIdx.x, op = ops.op[m];
    const double *p = part + (long)m * npart;
    const double identity = op == PCL_REDUCE_MAX ? -__builtin_huge_val() : op == PCL_REDUCE_MIN ? __builtin_huge_val() : 0.0;
    // eight chains per thread, so that eight loads are in flight (one chain waits a memory latency per partial): chain i
    // folds partials t + 256 (8 j + i), j = 0, 1, ..., and the chains are combined in the order 0 .. 7
    constexpr int CHAINS = 8;
    double acc[CHAINS];
    for (int i = 0; i < CHAINS; i++) acc[i] = identity;
    for (long base = threadIdx.x; base < npart; base += (long)REDUCE_FINAL_THREADS * CHAINS) {
#pragma unroll
        for (int i = 0; i < CHAINS; i++) {
            const long k = base + (long)REDUCE_FINAL_THREADS * i;
            if (k < npart) acc[i] = reduce_combine(op, acc[i], p[k]);
        }
    }
    double v = acc[0];
    for (int i = 1; i < CHAINS; i++) v = reduce_combine(op, v, acc[i]);
    for (int w = 1; w < 64; w <<= 1) v = reduce_combine(op, v, __shfl_xor(v, w, 64));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = wsum[0];
        for (int w = 1; w < REDUCE_FINAL_THREADS / 64; w++) r = reduce_combine(op, r, wsum[w]);
        out[m] = r;
    }
}
int launch_reduce_partials(const ReduceFinal &r, std::string &err) {
    if (!r.part || !r.out || r.npart <= 0 || r.nout < 1 || r.nout > 8) {
        err = "launch_reduce_partials: bad arguments";
        return PCL_EINVAL;
    }
    ReduceOps ops;
    for (int m = 0; m < 8; m++) ops.op[m] = r.op[m];
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(r.nout), dim3(REDUCE_FINAL_THREADS), 0, r.stream, r.part, r.out, r.npart, ops);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCL_OK : hip_fail(err, "reduce_partials launch", e);
}

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
