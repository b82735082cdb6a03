// sweep_args.hpp -- plain launch descriptor shared by the host TU (pclaw.hip) and the two
// kernel TUs (kernels.hip compiled once per arithmetic mode).
// The run-time compile of a user-written Riemann solver (cellrp.hpp) reads this text too: what hiprtc cannot take --
// the standard headers and the host-side launch descriptors -- sits behind __HIPCC_RTC__.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <string>
#endif

namespace pcl {

constexpr int MAX_WAVES_K = 8;  // == PCL_MAX_WAVES of the C ABI

// Slices per workgroup U of the unsplit kernels compiled around a user-written Riemann solver with a transverse body
// (cellrp.hpp): the one rule, read by the host (it names the instantiations and records U in the handle, from which
// the launcher sizes its grids) and by the run-time text (a static_assert there ties the two).  What decides it is the
// static LDS of the two kernels (classic.hpp) against the 160 KB of a workgroup: unsplit_x_kernel holds gm and gp,
// unsplit_y_kernel the q tile of U + 1 columns as well (staged aux planes come on top only where they still fit).
// 16 slices up to meqn = 6 (147 KB), 12 above (meqn = 8: 148 KB; with 16 the y kernel of meqn = 7 would need 171.5 KB).
constexpr int unsplit_user_slices(int meqn) { return meqn <= 6 ? 16 : 12; }
constexpr long unsplit_x_lds_bytes(int meqn, int u) { return 8L * 2 * u * meqn * 64; }
constexpr long unsplit_y_lds_bytes(int meqn, int u) { return 8L * meqn * 64 * (u + 1) + unsplit_x_lds_bytes(meqn, u); }   // 512 meqn (3u + 1)
constexpr long UNSPLIT_LDS_LIMIT = 160 * 1024;
constexpr bool unsplit_user_slices_fit() {
    for (int m = 1; m <= MAX_WAVES_K; m++)
        if (unsplit_y_lds_bytes(m, unsplit_user_slices(m)) > UNSPLIT_LDS_LIMIT || unsplit_x_lds_bytes(m, unsplit_user_slices(m)) > UNSPLIT_LDS_LIMIT)
            return false;
    return true;
}
static_assert(unsplit_user_slices_fit(), "unsplit_user_slices: the static LDS of unsplit_x/y_kernel must fit 160 KB for every meqn");

// The general unsplit 3-D step (classic3.hpp: pieces3_kernel, gather3_kernel) passes the pieces of every slice through
// scratch planes: per cell with ghost cells and per component qadd, fadd(i+1) - fadd(i), gadd(1:2, -1:1) and hadd(1:2, -1:1).
// The one size rule, read by the host when it allocates (pclaw.hip) and by pcl_unsplit3_scratch_bytes.
constexpr int UNSPLIT3_VALUES = 14;
constexpr long long unsplit3_scratch_bytes(int meqn, int nx, int ny, int nz, int mbc) {
    return 8LL * UNSPLIT3_VALUES * meqn * (nx + 2 * mbc) * (long long)(ny + 2 * mbc) * (nz + 2 * mbc);
}

struct RpParams {
    double v[8];
};

// Source term of the 2-D Euler equations with radial symmetry (test/euler/2d/shockbubble.py:59-94, the app's
// step_Euler_radial): two-stage Runge-Kutta on one cell, in the operation order of the numpy callback.  Shared by the
// stand-alone source kernel (pclaw.hip) and the y pass that applies it while storing its results (classic.hpp).
__host__ __device__ inline void euler_radial_source(double &q0, double &q1, double &q2, double &q3, double rad, double dt,
                                                    double gamma1, double ndm1) {
    const double dt2 = dt / 2.0;
    double rho = q0;
    double u = q1 / rho;
    double v = q2 / rho;
    double press = gamma1 * (q3 - 0.5 * rho * (u * u + v * v));
    const double k2 = dt2 * ndm1 / rad;
    const double s0 = q0 - k2 * q2;
    const double s1 = q1 - k2 * rho * u * v;
    const double s2 = q2 - k2 * rho * v * v;
    const double s3 = q3 - k2 * v * (q3 + press);
    rho = s0;
    u = s1 / rho;
    v = s2 / rho;
    press = gamma1 * (s3 - 0.5 * rho * (u * u + v * v));
    const double k1 = dt * ndm1 / rad;
    const double n0 = q0 - k1 * s2;
    const double n1 = q1 - k1 * rho * u * v;
    const double n2 = q2 - k1 * rho * v * v;
    const double n3 = q3 - k1 * v * (s3 + press);
    q0 = n0; q1 = n1; q2 = n2; q3 = n3;
}

// A cell euler_radial_source returns bit for bit, for every dt in (0, 2^20], |gamma1|, |ndm1| <= 2^20 (checked by the
// host per launch) and any contraction of its expressions: v = +0 makes every increment a signed zero, q0 and q3 are
// non-zero and q1 is not -0 (q - (+-0) = q), and the bounds keep every factor in front of that zero finite
// (|k| <= 2^740, |k rho u| <= 2^920, |press| <= 2^320).  Proof in DESIGN.md 4.1a.  Quiet tiles of the one-kernel step
// under the fused source require it of every cell they store.
__host__ __device__ inline bool euler_radial_source_fixed(double q0, double q1, double q2, double q3, double rad) {
    return __builtin_bit_cast(unsigned long long, q2) == 0ull && __builtin_bit_cast(unsigned long long, q1) != (1ull << 63) &&
           q0 >= 0x1p-60 && q0 <= 0x1p60 && q1 >= -0x1p60 && q1 <= 0x1p60 && q3 > 0.0 && q3 <= 0x1p60 &&
           (rad >= 0x1p-700 || rad <= -0x1p-700);
}
constexpr double SRC_FIXED_BOUND = 0x1p20;   // the host's per-launch bound on dt, |gamma1| and |ndim - 1|

// SharpClaw form of the same source (apps/euler/2d/shockbubble/shockbubble.py:95-122, dq_Euler_radial): the increment
// dt * psi(q) of one cell, in the operation order of the numpy callback (-dt*(ndim-1)/rad is one array, then the
// products left to right); the energy-equation tracer component gets 0.
__host__ __device__ inline void euler_radial_dq(double q0, double q1, double q2, double q3, double rad, double dt,
                                                double gamma1, double ndm1, double (&d)[4]) {
    const double rho = q0;
    const double u = q1 / rho;
    const double v = q2 / rho;
    const double press = gamma1 * (q3 - 0.5 * rho * (u * u + v * v));
    const double c = -dt * ndm1 / rad;
    d[0] = c * q2;
    d[1] = c * rho * u * v;
    d[2] = c * rho * v * v;
    d[3] = c * v * (q3 + press);
}

struct SweepArgs {
    const double *qin;
    double *qout;
    const double *aux;
    long pitch;       // doubles between rows
    long plane;       // doubles between components
    int I, J;         // cells per row / rows, ghost cells included
    int mbc, mx, my;  // interior extents
    int mcapa;        // 0 = none, else 1-based aux component (method(6))
    int order;        // method(2)
    int mthlim[MAX_WAVES_K];
    double dtd;       // dt/dx of the sweep direction
    double dt, dx;    // separately, for the 1-D capa form dt/(dx*capa) (step1.f:70)
    RpParams par;
    unsigned long long *cfl;  // device word holding the running max (as ordered bits)
    // "virtual ghost cells": the x pass of the dim-split step evaluates the boundary conditions while it
    // loads (a ghost cell is an index remap of an interior cell, or a constant): no ghost-fill launches.
    // vbc[2*idim+side] = -1 (read memory) | PCL_BC_OUTFLOW | PERIODIC | REFLECTING | PCL_BC_CUSTOM (= vconst)
    int vbc_on;
    int vbc[4];
    double vconst[4][8];
    // Tile subset of the x pass, for overlapping the halo exchange with the interior (pclaw.hip,
    // step_split_overlapped): 0 = every tile, 1 = only tiles inside box = [tb_lo,tb_hi) x [ta_lo,ta_hi)
    // (they read no ghost cell), 2 = only the tiles outside the box.
    int sub;
    int box[4];
    // 3-D dimension-split sweeps (sweep3_kernel) only: strides in doubles along the sweep / across a tile /
    // per batch (blockIdx.y), extents with ghost cells, interior cells along the sweep, and the inclusive
    // ranges of across / batch indices whose slices are swept (the others are copied through)
    long s_al, s_ac, s_b;
    int n_al, n_ac, n_b, m_al;
    int lo_ac, hi_ac, lo_b, hi_b;
    // SharpClaw: Runge-Kutta combination fused into the LAST directional pass (sharp_kernel store phase):
    // rk_d = op(rk_a, rk_b, dq) per interior cell instead of writing dq (ops 1, 2, 5 of rk_kernel)
    int rk_op;
    const double *rk_a, *rk_b;
    double *rk_d;
    double rk_ca, rk_cb, rk_cc;
    // unsplit algorithm (step2.f) only:
    int trans;        // method(3): 0 no transverse terms, 1 increment waves, 2 + correction waves
    double dtd_t;     // dt/d of the transverse direction
    // (kept at the END of the block: the kernels' scalar loads of the fields above keep their offsets)
    // source term applied by the LAST pass of a dimension-split step while it stores its results (Godunov splitting,
    // clawpack.py:156-159): 0 none, 1 euler_radial_source(gamma1, ndim-1), aux plane 0 = radial coordinate.  SharpClaw:
    // 1 = euler_radial_dq added to deltaq by the last pass of a stage (sharpclaw.py:232-235, dq_src)
    int src_id;
    double src_p[2];
};

// The tile list's small state (classic_fused.hpp): the number of listed tiles of class A (they computed something in the
// launch before; from the list's front) and of class Q (quiet there; from its back), and the largest cached Courant
// maxima (bit patterns of doubles >= +0, before dt/d) of the x and y sweeps over the tiles it skips.  Three of them, rotating:
// a hand-over+list launch fills one and zeroes the one the hand-over after it fills; the third keeps the list the last
// launch ran over (pcl_tile_skip_stats).
struct TileNext {
    int na, nq;
    unsigned long long cx, cy;
};
// cells a tile of the one-kernel step owns, for the host's tile counts (kernels.hip ties them to F_OWN_C, F_OWN_R)
constexpr int TILE_OWN_C = 60, TILE_OWN_R = 12;
// The one-kernel step (classic_fused.hpp) holds q of up to ONEK_MAX_MEQN equations and up to ONEK_MAX_PLANES planes in all
// (q, the capacity function, staged aux components: two 80 KB workgroups per CU at least).  The one rule for every solver,
// built in or compiled at run time: read by fused_step_ok (pclaw.hip) and by cellrp_spec_check (cellrp.hpp), restated by
// the kernel's own static_assert.
constexpr int ONEK_MAX_MEQN = 5, ONEK_MAX_PLANES = 10;

#ifndef __HIPCC_RTC__       // from here on: host-side launch descriptors and the launchers' declarations
// unsplit 3-D (classic3.hpp): one direction's slices, applied in the reference's order by the marching kernel
struct Unsplit3Launch {
    SweepArgs a;          // qin = qold; s_al/n_al/m_al, dtd, par, mthlim, order, cfl as for sweep3
    double *qacc;         // the new state being accumulated
    long s_e, s_f;
    int n_e, n_f, m_e, m_f;
    int m3, m4;
    double dty, dtz;
    int dir;              // 1..3
    int rp;
    hipStream_t stream;
    // rp == PCL_RP_CELL (a user-written solver with rpt3 / rptt3 bodies, cellrp.hpp): the kernel table of the attached
    // module by CellrpSlot, what it was compiled for (as SweepLaunch::user_fns / user), and the solver's scratch planes
    // (unsplit3_scratch_bytes) with the extents, ghost cells included, they are laid out over
    const hipFunction_t *user_fns = nullptr;
    const struct CellrpSpec *user = nullptr;
    double *scratch = nullptr;
    int fwave = 0;
    int n3[3] = {0, 0, 0};
};

struct RkLaunch {
    double *d;
    const double *a, *b, *c;
    double ca, cb, cc;
    long n;
    int op;
};

// D = A + c[0]*K[0] + ... + c[nterms-1]*K[nterms-1] over n doubles (sharpclaw.hpp: rk_lincomb_kernel), nterms <= 16; the
// caller has dropped the terms whose coefficient is zero and has checked that d is none of the k
struct RkLincombLaunch {
    double *d = nullptr;
    const double *a = nullptr;
    const double *k[16] = {};
    double c[16] = {};
    int nterms = 0;
    long n = 0;
};

// What a user-written Riemann solver (cellrp.hpp) is compiled for: the one record that travels from a pcl_cellrp_compile*
// call through the cache entry and the loaded module to the launchers.  Every field is part of the cache key and decides
// which kernels the code object holds.  A default-constructed one is "nothing attached".
#define PCL_CELLRP_MAX_AUX 8       // what pcl_cellrp_aux writes at most; the tile limits are tighter (cellrp_spec_check)
struct CellrpSpec {
    int meqn = 0, mwaves = 0, ndim = 0, math = 0;   // ndim 3: the three sweep3_kernel passes and nothing else (pcl_cellrp_compile3)
    int naux = 0, aux[PCL_CELLRP_MAX_AUX] = {0};    // the aux components the body reads, in the body's order
    int trans = 0;                                  // 1: a transverse body, the code object holds the unsplit kernels too
    int trans3 = 0;                                 // 3-D: 1 an rpt3 body, 2 rpt3 and rptt3; the code object holds pieces3_kernel too
    int form = 0;                                   // PCL_CELLRP_FORM_* bits
    int lim_type = 0, weno_order = 0, char_decomp = 0;      // a SharpClaw handle (lim_type 0: a classic one); with ndim 3 the
                                                            // three sharp3_kernel passes and nothing else (pcl_cellrp_compile3_sharp)
    int onek = 0;                                   // 1: the code object holds the one-kernel dimension-split 2-D step too
    bool fwave() const { return (form & PCL_CELLRP_FORM_FWAVE) != 0; }
    bool capa() const { return (form & PCL_CELLRP_FORM_CAPA) != 0; }
    bool sharp() const { return lim_type != 0; }
    int mbc() const { return sharp() ? (weno_order + 1) / 2 : 0; }
    int slices() const { return trans ? unsplit_user_slices(meqn) : 0; }   // per workgroup of the unsplit kernels
};

// The kernels a module of a user-written Riemann solver can hold, by what launches them.  A classic handle fills the sweeps of
// its dimension (1-D: SWEEP_X alone; 3-D: the three sweep3_kernel passes), with a transverse body the unsplit phases, with
// spec.onek the one-kernel step, with spec.trans3 the pieces kernels of the three directions of the unsplit 3-D step; a
// SharpClaw handle holds its kernels in the sweep slots (char_decomp = 1: SWEEP_X alone).  The order is that of cellrp_exprs.
enum CellrpSlot { SLOT_SWEEP_X, SLOT_SWEEP_Y, SLOT_SWEEP_Z, SLOT_UNSPLIT_X, SLOT_UNSPLIT_Y, SLOT_ONEK,
                  SLOT_PIECES3_X, SLOT_PIECES3_Y, SLOT_PIECES3_Z, CELLRP_NSLOTS };

struct SweepLaunch {
    SweepArgs a;
    int ndim;   // 1, 2 or 3
    int rp;     // PCL_RP_*
    int ids;    // 1 = x pass (or the 1-D step), 2 = y pass, 3 = z pass (launch_sweep3)
    int fwave;
    int lim_type;  // SharpClaw reconstruction (2 PyWENO weno5, 3 legacy weno5)
    int char_decomp = 0;   // SharpClaw: 1 = wave-based reconstruction (1-D: tvd2_wave / weno5_wave)
    hipStream_t stream;
    // rp == PCL_RP_CELL (a user-written Riemann solver, cellrp.hpp): user_fns is the kernel table of the module the solver handle
    // has loaded, indexed by CellrpSlot (null: nothing attached), and user what that module was compiled for.  Each launcher
    // takes the slot of its own family and direction, refuses a launch the module was not compiled for and fires the plan of
    // the built-in solvers at that kernel (kernels.hip: Plan)
    const hipFunction_t *user_fns = nullptr;
    CellrpSpec user;
    // one-kernel step only (classic_fused.hpp, quiet tiles): this launch's per-tile words and per-wavefront Courant
    // maxima (tq_out null: no bookkeeping).  A list launch (tq_list set) computes the tq_next->na + nq tiles a
    // hand-over+list kernel listed behind the previous launch and publishes the Courant number of those it skips.
    unsigned *tq_out = nullptr;
    double2 *tq_cfl = nullptr;
    const int *tq_list = nullptr;
    const TileNext *tq_next = nullptr;
    // the ring check of a list launch's class-Q tiles (null: off): a tile settled by it leaves ring_seq, the number of
    // this launch, in its word of tq_ring (pcl_tile_ring_stats)
    unsigned *tq_ring = nullptr;
    unsigned ring_seq = 0;
    // row reuse of the x sweeps (classic_fused.hpp; 0: off).  tq_reuse (null: not counted): two words per tile, a computed
    // tile leaves ring_seq in the first and its wavefronts their reused sweeps in the bytes of the second
    // (pcl_tile_rowreuse_stats)
    int rowreuse = 1;
    unsigned *tq_reuse = nullptr;
    // column shortcut of the y sweeps (classic_fused.hpp; 0: off).  tq_ycol (null: not counted): two words per tile, as
    // tq_reuse -- ring_seq and, a byte per wavefront, its y-sweep calls that took the shortcut (pcl_tile_ycol_stats)
    int ycol = 1;
    unsigned *tq_ycol = nullptr;
};

// The Courant hand-over behind a one-kernel launch of the whole block, with the next launch's tile list
// (classic_fused.hpp: handover_list_kernel): the words of the launch just enqueued (tq_in), the next launch's words
// (tq_out, TQ_ALL for the tiles it skips), the list, and two TileNext blocks (next is filled, other zeroed); ran is the
// block of the list the launch just enqueued ran over (null: it computed every tile).
struct TileHandover {
    unsigned long long *cfl = nullptr;      // the device Courant word (read, re-zeroed)
    unsigned long long *host = nullptr;     // device view of the host block: [0] value, [1] sequence number, [2] tiles dispatched
    unsigned long long seq = 0;
    int ntx = 0, nty = 0, mbc = 0, mx = 0, my = 0;
    const unsigned *tq_in = nullptr;
    unsigned *tq_out = nullptr;
    const double2 *tq_cfl = nullptr;
    int *tq_list = nullptr;
    TileNext *next = nullptr, *other = nullptr;
    const TileNext *ran = nullptr;
    hipStream_t stream;
};

// The second pass of a functional (cellfn.hpp: pcl_cellfn_red leaves part[m * npart + w], the partial of output m from
// workgroup w): nout workgroups of REDUCE_FINAL_THREADS threads, one per output, each combining its npart partials in an
// order fixed by npart alone, into out[m].  op[m] is a PCL_REDUCE_* (the partials of a sum of |f| are summed).
constexpr int REDUCE_FINAL_THREADS = 256;
struct ReduceFinal {
    const double *part = nullptr;
    double *out = nullptr;
    long npart = 0;
    int nout = 0;
    int op[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipStream_t stream;
};

// What the host layer knows about a built-in Riemann solver, read off its struct in rp.hpp through the solver list of
// kernels.hip: the sizes pcl_create insists on, and which kernels have an instantiation of it -- onek / onek_aux: the
// one-kernel step (launch_step2ds) without aux planes / with the solver's cell-wise coefficients staged next to q;
// sharp: the SharpClaw kernels, sharp_high: those of weno_order 7..17 too, sharp_wave: the wave-based 1-D kernel.
struct RpFacts { int id, ndim, meqn, mwaves, naux; bool fwave, onek, onek_aux, sharp, sharp_high, sharp_wave; };

// A 2-D block as the interior-box functions see it: interior cells, ghost layers, cells with ghosts.
struct BlockGeom { int mx, my, mbc, I, J; };
// The tiles of a pass that read no ghost cell: box = [lo, hi) of the tile rows, [lo, hi) of the tiles along a row;
// ntiles = the counts of either; any: the box is not empty.
struct InteriorBox { bool any = false; int box[4] = {0, 0, 0, 0}, ntiles[2] = {0, 0}; };

// defined in kernels.hip, once per arithmetic mode; returns 0 or a PCL_E* code + message:
//   launch_sweep     one directional sweep, l.ids 1 = x (or the 1-D step), 2 = y
//   launch_step2ds   whole dim-split 2-D step in one kernel (classic_fused.hpp)
//   launch_sweep3    3-D dim-split sweep, l.ids = direction 1..3
//   launch_unsplit3  unsplit 3-D: slices + combine of one direction
//   launch_unsplit   scratch-free unsplit phase
//   launch_sharp     SharpClaw dq of one direction
//   launch_rk / launch_rk_lincomb   register arithmetic of the Runge-Kutta schemes
#define PCL_LAUNCHERS                                                              \
    int launch_sweep(const SweepLaunch &l, std::string &err);                      \
    int launch_step2ds(const SweepLaunch &l, std::string &err);                    \
    int launch_sweep3(const SweepLaunch &l, std::string &err);                     \
    int launch_unsplit3(const Unsplit3Launch &l, std::string &err);                \
    int launch_unsplit(const SweepLaunch &l, const double *qx, std::string &err);  \
    int launch_sharp(const SweepLaunch &l, std::string &err);                      \
    int launch_rk(const RkLaunch &r, hipStream_t stream, std::string &err);       \
    int launch_rk_lincomb(const RkLincombLaunch &r, hipStream_t stream, std::string &err);
namespace exact {
PCL_LAUNCHERS
// what does not depend on the arithmetic mode: exact alone has it
const RpFacts *rp_facts(int rp);    // null: no built-in solver has this id
int sweep_tile_max_planes();        // q + aux planes a sweep_kernel tile may hold (TileShape<1/2>::PLANE against 64 KB)
int sweep3_tile_max_planes();       // q + aux + capa planes a sweep3_kernel tile may hold (Tile3Shape<1..3>::PLANE against 64 KB)
int sharp3_tile_max_planes();        // q + capa + aux planes a sharp3_kernel tile may hold, one rule for the three passes
int sharp_tile_max_planes(int ixy, int naux);   // planes a sharp_kernel tile of pass ixy may hold for a solver with naux aux components
// x-pass tiles [tb_lo,tb_hi) x [ta_lo,ta_hi) that read no ghost cell; false if there are none
// ntiles[0], ntiles[1] = row tiles / tiles along a row of the x pass
bool x_interior_box(const BlockGeom &a, int box[4], int ntiles[2]);
bool step2ds_interior_box(const BlockGeom &a, int box[4], int ntiles[2]);   // the same for the one-kernel step: (nty, ntx)
int launch_tile_handover(const TileHandover &h, std::string &err);   // Courant hand-over + next tile list (bit-only)
int launch_reduce_partials(const ReduceFinal &r, std::string &err);  // a functional's second pass (adds, fmax, fmin: no mode)
}
namespace fast { PCL_LAUNCHERS }
// exact + IEEE quotients for underflow-range numerators as well (rp.hpp PCL_DENORM_GUARD), PCL_MATH_STRICT
namespace strict { PCL_LAUNCHERS }
#undef PCL_LAUNCHERS
#endif  // !__HIPCC_RTC__

}  // namespace pcl
