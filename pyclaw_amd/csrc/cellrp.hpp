// cellrp.hpp -- user-written Riemann solvers: the NORMAL solver of one interface (Clawpack's rp1 / rpn2) given as the
// text of a C++ function body, compiled at run time into the project's own sweep kernel (pyclaw.CellRiemann,
// cfg.rp = PCL_RP_CELL).
//
// Nothing of the sweep is restated here.  The Makefile embeds the headers the sweep is written in -- sweep_args.hpp,
// ghost_rule.hpp, rp.hpp, classic.hpp and include/pyclaw_amd.h -- as text (cellrp_headers.inc), hiprtc gets them as named
// headers, and the program below wraps the user's body in a solver struct of the shape rp.hpp documents and asks for
//     sweep_kernel<UserRp, 1, false, false, true>                                   the 1-D step
//     sweep_kernel<UserRp, 1, false, false, false>, <UserRp, 2, false, false, false>  the x and y passes of step2ds
// compiled with the flags of the library's own arithmetic mode (PCL_RTC_FLAGS_*, from the Makefile).  A user solver
// thereby runs with the LDS tiles, DPP shifts, limiter, jump-free shortcut and Courant reduction of the built-in
// solvers, bit for bit; kernels.hip launches the module's functions over the grid it computes for its own.
//
// The body is the inside of solve():
//     const double ql[MEQN], qr[MEQN]      the cells left and right of the interface
//     const double p[8]                    the solver's parameters (RpParams::v; by value in SweepArgs, so changing them
//                                          compiles nothing)
//     ixy                                  compile-time constant, 1 = x sweep (always in 1-D), 2 = y sweep
//     double wave[MWAVES][MEQN], s[MWAVES], amdq[MEQN], apdq[MEQN]
//                                          the results, zero on entry: what the body never assigns is a compile-time zero
//     dmax, dmin, dsqrt, fdiv, Recip ...   the helpers rp.hpp gives the built-in solvers (a built-in solver restated as a
//                                          body gives the same bits); / and sqrt are IEEE in the exact mode
// and whatever `preamble` declares in front of the struct (helper functions, inside namespace pcl::<mode>).
// Diagnostics carry the user's line numbers: "riemann:3:...", "preamble:1:...".
//
// The wrapper: Cell { double q[MEQN]; } with NCELL = MEQN and a copying precell; nz() is true everywhere; speeds() runs
// the same body and keeps s alone (the compiler drops the rest), so the speeds of a jump-free wavefront are the bits of
// solve() by construction; NAUX = 0, ONEK and SHARP* false.
// Contract: for bitwise-equal ql and qr the waves and fluctuations are zero -- the jump-free shortcut (classic.hpp,
// DESIGN.md 4.1) copies such a wavefront through and takes only the speeds, as any consistent solver has it.
// (This contract is the wave form's.  An f-wave body, below, is not held to it.)
// Limits: meqn, mwaves <= 8 (MAX_WAVES_K; the y tile of meqn = 8 is the 64 KB a workgroup may declare), 8 parameters.
//
// A solver with cell-wise coefficients lists the components of the aux array its body reads (pcl_cellrp_compile_aux,
// CellRiemann(aux=...)): the program is then the second wrapper below, compiled with -DPCL_CELLRP_NAUX=<n> behind a
// generated constexpr table of the list.  NAUX = NAUX_T = n, aux_index<IXY>(k) = auxt_index<IXY>(k) = the k-th listed
// component (0-based; one list for both sweeps), so the sweep stages those n planes next to q in its LDS tile exactly as
// it does for advection_color_1d, vc_advection_2d and vc_acoustics_2d; Cell { double q[MEQN]; double aux[NAUX]; } and
// the three-argument precell copy both.  The body gains
//     const double auxl[NAUX], auxr[NAUX]  the listed components, in list order, of the cell LEFT and of the cell RIGHT of
//                                          the interface (Clawpack's "aux(1) is the value at the left edge of cell i" is
//                                          auxr[0]); a body that needs another component per direction branches on ixy
// Contract with aux: for bitwise-equal ql and qr the waves and fluctuations are zero WHATEVER aux holds -- the jump-free
// shortcut of the solvers with aux (classic.hpp, lane_core: `!FWAVE && RP::NAUX > 0`) compares cL.q with cR.q alone and
// takes speeds(cL, cR), each interface with its own auxl / auxr, on such a wavefront.  A flux-difference form over
// varying coefficients breaks this: that is an f-wave solver, compiled with the f-wave form below.
// Limit with aux: the tile holds MEQN + NAUX planes of TileShape<IXY>::PLANE doubles, so meqn + naux <=
// cellrp_max_planes() = 65536 / (8 * max PLANE) -- 8, set by the 1024-double y tile; refused on the host with that sum
// and by the static_assert below.  The list is part of the cache key; without one the program text, the key and the
// handle are those of the first wrapper.
//
// A second, optional text is the TRANSVERSE solver (Clawpack's rpt2; pcl_cellrp_compile_t, CellRiemann(transverse=...)):
// two more members of the same struct (kCellrpTrans* below, where the body's interface and contract are written down),
// and two more name expressions, unsplit_x_kernel<UserRp, false, U, false> and unsplit_y_kernel<UserRp, false, U, false,
// false> -- the unsplit step (classic.hpp) around the user's two bodies, launched by launch_unsplit (kernels.hip) with
// the parameters and grids of the built-in solvers.  U, the slices per workgroup, is unsplit_user_slices(meqn)
// (sweep_args.hpp: the one rule, read here to name the instantiations and by the run-time text to check them); the
// handle records it and the launcher sizes its grids from the handle.  Always the tile form of the y phase: the marching
// kernel (its static LDS is 29184 * meqn bytes) stays with the built-in solvers.  Without a transverse text the program
// text, the key, the handle and the symbols are what they were.
//
// The FORM of a solver (pcl_cellrp_compile_form, CellRiemann(fwave=..., capa=...)) is the pair of template flags the
// kernels are instantiated with: sweep_kernel<UserRp, IXY, CAPA, FWAVE, DIM1> and, with a transverse text,
// unsplit_x_kernel<UserRp, FWAVE, U, CAPA>, unsplit_y_kernel<UserRp, FWAVE, U, CAPA, false>.  A handle serves one form --
// only that form's instantiations are compiled -- and records it; the solver's cfg.fwave and method[5] must say the same
// (pcl_create_cellrp, pcl_cellrp_attach, and once more the launchers of kernels.hip).  Form 0 is the program text, key,
// handle and symbols of before there were forms.
//   PCL_CELLRP_FORM_FWAVE: the body assigns F-WAVES, and the array is named fwave[MWAVES][MEQN] as in Clawpack's f-wave
//     solvers (a body that assigns `wave` does not compile: "riemann:<n>: ... undeclared identifier 'wave'"); s, amdq,
//     apdq, ql, qr, auxl, auxr, p, ixy, the preamble and the helpers are unchanged, everything is zero on entry, and the
//     transverse body's interface is what it is in wave form.  The "equal q => zero waves" contract does NOT apply: the
//     f-waves of a flux-difference solver over varying coefficients are non-zero between equal cells, and lane_core takes
//     neither jump-free shortcut when FWAVE is set (both sit behind `if constexpr (!FWAVE && ...)`): every interface is
//     solved.  UserRp::IS_FWAVE is true.  The limiter and the second-order correction are flux2fw.f's (dsign(1, s)).
//   PCL_CELLRP_FORM_CAPA: the sweeps divide dt/dx by aux(mcapa) per cell and accumulate the reference's Courant expression
//     (cfl_accumulate<true>); the body does not change.  The component is a run-time value, SweepArgs::mcapa, so one handle
//     serves any mcapa.  The sweep tile holds the capacity function's plane next to q and the listed aux components:
//     meqn + 1 + naux <= cellrp_max_planes() = 8, refused on the host with the sum and by the static_assert of kCellrpForm.
//     The unsplit kernels read capa from global memory per lane (classic.hpp: unsplit_x_kernel, unsplit_y_kernel, `if
//     constexpr (CAPA)`) and declare no LDS for it, so unsplit_user_slices(meqn) stands as it is.
//
// A SHARPCLAW handle (pcl_cellrp_compile_sharp, CellRiemann(sharpclaw=True)) is the same struct inside another text: the
// program includes sharpclaw.hpp (embedded with weno_tables.hpp) in place of classic.hpp and asks for the SharpClaw
// kernels of the one reconstruction the run needs and for no classic kernel --
//     sharp_kernel<UserRp, 1, CAPA, LIM, K>                                       1-D
//     sharp_kernel<UserRp, 1, CAPA, LIM, K>, sharp_kernel<UserRp, 2, CAPA, LIM, K>  the x and y passes in 2-D
//     sharp1w_kernel<UserRp, LIM, CAPA>                                           char_decomp = 1 (1-D, LIM 1 or 2, K 3)
// LIM = lim_type 1..3, K = mbc = (weno_order + 1) / 2 = 3, or 4..9 with LIM 2: any system gets every order, since only one
// (LIM, K, CAPA) is instantiated.  The kernels ask of RP what the wrapper has (Cell, precell<IXY> with and without aux,
// solve<IXY>, MEQN, MWAVES, NAUX, aux_index<IXY>) and have no FWAVE flag -- they read s, amdq, apdq alone -- so the struct
// gets no member for them and the form's members (kCellrpForm) are left out; an f-wave body still names its array fwave.
// The "equal q => zero waves" contract is not relied on: every interface and the problem inside every cell are solved.
// The handle records (lim_type, weno_order, char_decomp), part of its key ("rps<lim>.<order>.<cd>,..."); it serves
// pcl_create_cellrp with cfg.kind = PCL_KIND_SHARPCLAW whose lim_type, mbc, method[4], fwave and method[5] > 0 say the same,
// and nothing else; launch_sharp (kernels.hip) checks the same once more and launches over the built-in grids.
// Limit: sharp_kernel's tile is static LDS of TA * 64 doubles per plane, TA = sharp_tile_across (16; 8 in the y pass from
// six aux components on); the x pass stages meqn + capa planes, the y pass meqn + capa + naux, each within 64 KB
// (sharp_tile_max_planes, kernels.hip, next to sweep_tile_max_planes): refused on the host with the sum and by the
// static_assert of kCellrpCloseSharp.  A classic handle's program text, key and symbols are what they were.
// Not served under SharpClaw: a fused dq source (a source term runs as its own pass), char_decomp 2 / 3, tfluct.
// Not served in any form: HAS_QCOR (the sphere solver's conservation fix), a transverse body with both cells and aux, the
// marching y phase, the one-kernel step, 3-D, more than one block.
#pragma once
#include "cellfn.hpp"
// generated by the Makefile (embed_headers.py): PCL_RTC_FLAGS_EXACT / _FAST / _STRICT, the flags kernels_<mode>.o is built
// with, and kCellrpHeaderNames[], kCellrpHeaderTexts[], kCellrpHeaderCount
#include "cellrp_headers.inc"

#define PCL_CELLRP_MAX_PARAMS 8
#define PCL_CELLRP_MAX_AUX 8       // what pcl_cellrp_aux writes at most; the tile limit is tighter (cellrp_max_planes)

struct pcl_cellrp {
    long id = 0;                // never reused, from the counter of the cell functions
    int meqn = 0, mwaves = 0, ndim = 0, math = 0;
    int refs = 0;
    int naux = 0, aux[PCL_CELLRP_MAX_AUX] = {0};     // the aux components the body reads, in the body's order
    std::string key;
    std::vector<char> code;     // the code object
    std::string sym[2];         // lowered names: [0] the 1-D step or the x pass, [1] the y pass (2-D)
    // a transverse body was given (2-D): the unsplit kernels are in the code object too, compiled with `slices` slices per
    // workgroup (unsplit_user_slices, sweep_args.hpp); sym_u: [0] unsplit_x_kernel, [1] unsplit_y_kernel
    bool trans = false;
    int slices = 0;
    std::string sym_u[2];
    // PCL_CELLRP_FORM_* bits: what the kernels in the code object were instantiated for (f-waves, a capacity function)
    int form = 0;
    // a SharpClaw handle (pcl_cellrp_compile_sharp): the code object holds sharp_kernel<UserRp, 1 / 2, CAPA, lim_type, mbc>
    // (sym[0], sym[1]) or, with char_decomp = 1, sharp1w_kernel<UserRp, lim_type, CAPA> (sym[0]) and no classic kernel
    bool sharp = false;
    int lim_type = 0, weno_order = 0, char_decomp = 0;
};

namespace pcl {

// what a SharpClaw handle is compiled for (lim_type 0: a classic handle)
struct CellrpSharp {
    int lim_type = 0, weno_order = 0, char_decomp = 0;
    bool on() const { return lim_type != 0; }
    int mbc() const { return (weno_order + 1) / 2; }
};

static const char *const kCellrpHead = R"PCLSRC(
#include "classic.hpp"
namespace pcl {
namespace PCL_NS {
)PCLSRC";

// a SharpClaw handle: the same wrapper struct inside the text of the SharpClaw kernels
static const char *const kCellrpHeadSharp = R"PCLSRC(
#include "sharpclaw.hpp"
namespace pcl {
namespace PCL_NS {
)PCLSRC";

static const char *const kCellrpOpen = R"PCLSRC(
struct UserRp : RpDefaults {
    static constexpr int ID = PCL_RP_CELL, NDIM = PCL_CELLRP_NDIM;
    static constexpr int MEQN = PCL_CELLRP_MEQN, MWAVES = PCL_CELLRP_MWAVES, NCELL = MEQN, NAUX = 0;
    static_assert(MEQN >= 1 && MEQN <= MAX_WAVES_K && MWAVES >= 1 && MWAVES <= MAX_WAVES_K, "1 <= meqn, mwaves <= 8");
    struct Cell { double q[MEQN]; };
    template <int IXY> __device__ static constexpr bool nz(int, int) { return true; }
    template <int IXY> __device__ static __forceinline__ Cell precell(const double *q, const RpParams &) {
        Cell c;
#pragma unroll
        for (int m = 0; m < MEQN; m++) c.q[m] = q[m];
        return c;
    }
    template <int ixy>
    __device__ static __forceinline__ void body(const double (&ql)[MEQN], const double (&qr)[MEQN], const double (&p)[8],
                                                double (&wave)[MWAVES][MEQN], double (&s)[MWAVES], double (&amdq)[MEQN],
                                                double (&apdq)[MEQN]) {
)PCLSRC";

static const char *const kCellrpTail = R"PCLSRC(
    }
#line 1 "pcl_cellrp_wrapper"
    template <int IXY>
    __device__ static __forceinline__ void solve(const Cell &L, const Cell &R, const RpParams &p, double (&wave)[MWAVES][MEQN],
                                                 double (&s)[MWAVES], double (&amdq)[MEQN], double (&apdq)[MEQN]) {
#pragma unroll
        for (int mw = 0; mw < MWAVES; mw++) {
            s[mw] = 0.0;
#pragma unroll
            for (int m = 0; m < MEQN; m++) wave[mw][m] = 0.0;
        }
#pragma unroll
        for (int m = 0; m < MEQN; m++) { amdq[m] = 0.0; apdq[m] = 0.0; }
        body<IXY>(L.q, R.q, p.v, wave, s, amdq, apdq);
    }
    // the same body; the compiler keeps what s needs
    template <int IXY>
    __device__ static __forceinline__ void speeds(const Cell &L, const Cell &R, const RpParams &p, double (&s)[MWAVES]) {
        double wave[MWAVES][MEQN], amdq[MEQN], apdq[MEQN];
        solve<IXY>(L, R, p, wave, s, amdq, apdq);
    }
)PCLSRC";

static const char *const kCellrpClose = R"PCLSRC(};
static_assert(sizeof(double) * UserRp::MEQN * TileShape<2>::PLANE <= 65536 && sizeof(double) * UserRp::MEQN * TileShape<1>::PLANE <= 65536,
              "meqn: the LDS tile of sweep_kernel (classic.hpp) does not fit a workgroup's 64 KB");
}  // namespace PCL_NS
}  // namespace pcl
)PCLSRC";

// The wrapper of a solver that reads aux (PCL_CELLRP_NAUX > 0).  cellrp_aux_component(k) is generated in front of it.
static const char *const kCellrpOpenAux = R"PCLSRC(
struct UserRp : RpDefaults {
    static constexpr int ID = PCL_RP_CELL, NDIM = PCL_CELLRP_NDIM;
    static constexpr int MEQN = PCL_CELLRP_MEQN, MWAVES = PCL_CELLRP_MWAVES, NAUX = PCL_CELLRP_NAUX, NAUX_T = NAUX, NCELL = MEQN + NAUX;
    static_assert(MEQN >= 1 && MEQN <= MAX_WAVES_K && MWAVES >= 1 && MWAVES <= MAX_WAVES_K, "1 <= meqn, mwaves <= 8");
    static_assert(NAUX >= 1, "this wrapper is the one with aux");
    template <int IXY> __host__ __device__ static constexpr int aux_index(int k) { return cellrp_aux_component(k); }
    template <int IXY> __host__ __device__ static constexpr int auxt_index(int k) { return cellrp_aux_component(k); }
    struct Cell { double q[MEQN]; double aux[NAUX]; };
    template <int IXY> __device__ static constexpr bool nz(int, int) { return true; }
    template <int IXY> __device__ static __forceinline__ Cell precell(const double *q, const RpParams &, const double *auxv) {
        Cell c;
#pragma unroll
        for (int m = 0; m < MEQN; m++) c.q[m] = q[m];
#pragma unroll
        for (int k = 0; k < NAUX; k++) c.aux[k] = auxv[k];
        return c;
    }
    template <int ixy>
    __device__ static __forceinline__ void body(const double (&ql)[MEQN], const double (&qr)[MEQN], const double (&auxl)[NAUX],
                                                const double (&auxr)[NAUX], const double (&p)[8], double (&wave)[MWAVES][MEQN],
                                                double (&s)[MWAVES], double (&amdq)[MEQN], double (&apdq)[MEQN]) {
)PCLSRC";

static const char *const kCellrpTailAux = R"PCLSRC(
    }
#line 1 "pcl_cellrp_wrapper"
    template <int IXY>
    __device__ static __forceinline__ void solve(const Cell &L, const Cell &R, const RpParams &p, double (&wave)[MWAVES][MEQN],
                                                 double (&s)[MWAVES], double (&amdq)[MEQN], double (&apdq)[MEQN]) {
#pragma unroll
        for (int mw = 0; mw < MWAVES; mw++) {
            s[mw] = 0.0;
#pragma unroll
            for (int m = 0; m < MEQN; m++) wave[mw][m] = 0.0;
        }
#pragma unroll
        for (int m = 0; m < MEQN; m++) { amdq[m] = 0.0; apdq[m] = 0.0; }
        body<IXY>(L.q, R.q, L.aux, R.aux, p.v, wave, s, amdq, apdq);
    }
    // the same body; the compiler keeps what s needs
    template <int IXY>
    __device__ static __forceinline__ void speeds(const Cell &L, const Cell &R, const RpParams &p, double (&s)[MWAVES]) {
        double wave[MWAVES][MEQN], amdq[MEQN], apdq[MEQN];
        solve<IXY>(L, R, p, wave, s, amdq, apdq);
    }
)PCLSRC";

static const char *const kCellrpCloseAux = R"PCLSRC(};
static_assert(sizeof(double) * (UserRp::MEQN + UserRp::NAUX) * TileShape<2>::PLANE <= 65536 &&
                  sizeof(double) * (UserRp::MEQN + UserRp::NAUX) * TileShape<1>::PLANE <= 65536,
              "meqn + naux: the LDS tile of sweep_kernel (classic.hpp) does not fit a workgroup's 64 KB");
}  // namespace PCL_NS
}  // namespace pcl
)PCLSRC";

// The transverse body (pcl_cellrp_compile_t, 2-D only): the inside of Clawpack's rpt2 for one interface, two more members
// of the same struct, in front of its end.  Given one, the program also asks for the two unsplit kernels.
// Without aux, transverse<IXY>(L, R, par, asdq, bm, bp) of lane_core<..., TRANS = true> (classic.hpp); the body sees
//     const double ql[MEQN], qr[MEQN]     the cells left and right of the interface whose fluctuation is split -- the same
//                                         pair for A-dq and for A+dq of one interface: there is no imp
//     const double asdq[MEQN], p[8], ixy  the fluctuation, the parameters, the direction of the NORMAL solve (the split is
//                                         across it)
//     double bmasdq[MEQN], bpasdq[MEQN]   the down- and up-going parts, zero on entry
// With an aux list, transverse_vc<IXY>(c1, auxo, auxb, auxa, par, asdq, bm, bp); the body sees
//     const double q1[MEQN], aux1[NAUX]   the cell the fluctuation belongs to: left of the interface for A-dq, right of
//                                         it for A+dq
//     const double aux_below[NAUX], aux_above[NAUX]
//                                         the listed components of its neighbours at the lower and the upper transverse
//                                         index (Clawpack's aux1 / aux3 rows)
// and asdq, p, ixy, bmasdq, bpasdq as above.  auxt_index is aux_index, so auxo repeats c1.aux and is not passed on; a
// transverse body that needs both cells AND aux is not served.
// Contract: for asdq all zero the results are zero.  A jump-free wavefront in the TRANS core sets the slice's pieces to
// zero and never calls the body (classic.hpp, lane_core: both no-jump branches).
// Diagnostics: "transverse:<n>:...", the body's own line numbers.
static const char *const kCellrpTransOpen = R"PCLSRC(
    template <int ixy>
    __device__ static __forceinline__ void tbody(const double (&ql)[MEQN], const double (&qr)[MEQN], const double (&p)[8],
                                                 const double (&asdq)[MEQN], double (&bmasdq)[MEQN], double (&bpasdq)[MEQN]) {
)PCLSRC";

static const char *const kCellrpTransTail = R"PCLSRC(
    }
#line 1 "pcl_cellrp_wrapper_t"
    template <int IXY>
    __device__ static __forceinline__ void transverse(const Cell &L, const Cell &R, const RpParams &p, const double (&asdq)[MEQN],
                                                      double (&bm)[MEQN], double (&bp)[MEQN]) {
#pragma unroll
        for (int m = 0; m < MEQN; m++) { bm[m] = 0.0; bp[m] = 0.0; }
        tbody<IXY>(L.q, R.q, p.v, asdq, bm, bp);
    }
)PCLSRC";

static const char *const kCellrpTransOpenAux = R"PCLSRC(
    template <int ixy>
    __device__ static __forceinline__ void tbody(const double (&q1)[MEQN], const double (&aux1)[NAUX], const double (&aux_below)[NAUX],
                                                 const double (&aux_above)[NAUX], const double (&p)[8], const double (&asdq)[MEQN],
                                                 double (&bmasdq)[MEQN], double (&bpasdq)[MEQN]) {
)PCLSRC";

static const char *const kCellrpTransTailAux = R"PCLSRC(
    }
#line 1 "pcl_cellrp_wrapper_t"
    // (auxo is c1.aux again: one list serves aux_index and auxt_index)
    template <int IXY>
    __device__ static __forceinline__ void transverse_vc(const Cell &c1, const double *, const double *auxb, const double *auxa,
                                                         const RpParams &p, const double (&asdq)[MEQN], double (&bm)[MEQN],
                                                         double (&bp)[MEQN]) {
        double below[NAUX], above[NAUX];
#pragma unroll
        for (int k = 0; k < NAUX; k++) { below[k] = auxb[k]; above[k] = auxa[k]; }
#pragma unroll
        for (int m = 0; m < MEQN; m++) { bm[m] = 0.0; bp[m] = 0.0; }
        tbody<IXY>(c1.q, c1.aux, below, above, p.v, asdq, bm, bp);
    }
)PCLSRC";

// A form other than 0 (pcl_cellrp_compile_form): the last members of the struct.  IS_FWAVE is what IsFwave<RP> (classic.hpp)
// reads off a solver; with a capacity function the sweep tile holds one plane more (sweep_kernel: PAUX = MEQN + 1), and the
// limit the host refused over is restated.  NAUX is 0 in the wrapper without aux.
static const char *const kCellrpForm = R"PCLSRC(
    static constexpr bool IS_FWAVE = (PCL_CELLRP_FORM & 1) != 0;
    static constexpr bool FORM_CAPA = (PCL_CELLRP_FORM & 2) != 0;
    static_assert(!FORM_CAPA || (sizeof(double) * (MEQN + 1 + NAUX) * TileShape<2>::PLANE <= 65536 &&
                                 sizeof(double) * (MEQN + 1 + NAUX) * TileShape<1>::PLANE <= 65536),
                  "meqn + 1 + naux: the LDS tile of sweep_kernel (classic.hpp) with the capacity function's plane does not fit a workgroup's 64 KB");
)PCLSRC";

// The end of a SharpClaw handle's text.  The plane limit the host refused over (kernels.hip: sharp_tile_max_planes, next to
// sweep_tile_max_planes) restated: sharp_kernel's tile is static LDS of NP * TA * WAVE doubles, NP = meqn + capa in the x
// pass and meqn + capa + naux in the y pass, TA = sharp_tile_across<UserRp, IXY>().  sharp1w_kernel declares no LDS.
static const char *const kCellrpCloseSharp = R"PCLSRC(};
static constexpr int USER_SHARP_CAPA = (PCL_CELLRP_FORM & 2) != 0 ? 1 : 0;
static_assert(PCL_CELLRP_SHARP_CD == 1 ||
                  (sizeof(double) * (UserRp::MEQN + USER_SHARP_CAPA) * sharp_tile_across<UserRp, 1>() * WAVE <= 65536 &&
                   (UserRp::NDIM == 1 ||
                    sizeof(double) * (UserRp::MEQN + USER_SHARP_CAPA + UserRp::NAUX) * sharp_tile_across<UserRp, 2>() * WAVE <= 65536)),
              "meqn + capa + naux: the LDS tile of sharp_kernel (sharpclaw.hpp) does not fit the 64 KB a workgroup may declare");
}  // namespace PCL_NS
}  // namespace pcl
)PCLSRC";

// the slices per workgroup the host named the unsplit kernels with are the rule's, and both kernels' static LDS fits
static const char *const kCellrpTransCheck = R"PCLSRC(
    static constexpr int USLICES = PCL_CELLRP_USLICES;
    static_assert(NDIM == 2, "a transverse body belongs to a 2-D solver");
    static_assert(USLICES == unsplit_user_slices(MEQN), "slices per workgroup: not the rule of sweep_args.hpp");
    static_assert(unsplit_x_lds_bytes(MEQN, USLICES) <= UNSPLIT_LDS_LIMIT && unsplit_y_lds_bytes(MEQN, USLICES) <= UNSPLIT_LDS_LIMIT,
                  "the static LDS of unsplit_x_kernel / unsplit_y_kernel (classic.hpp) does not fit a workgroup's 160 KB");
)PCLSRC";

static inline const char *cellrp_ns(int math) { return math == 1 ? "fast" : math == 2 ? "strict" : "exact"; }

// (without a list the key is what it was before there were lists: the same entry as pcl_cellrp_compile's; without a
// transverse text it is what it was before there were transverse texts; form 0 likewise)
static inline std::string cellrp_key(const char *body, const char *preamble, int meqn, int mwaves, int ndim, int math,
                                     const int *aux = nullptr, int naux = 0, const char *trans = nullptr, int form = 0,
                                     const CellrpSharp &sharp = CellrpSharp()) {
    // (a SharpClaw handle: its own prefix with lim_type, weno_order and char_decomp; a classic key is what it was)
    std::string k = sharp.on() ? "rps" + std::to_string(sharp.lim_type) + "." + std::to_string(sharp.weno_order) + "." +
                                     std::to_string(sharp.char_decomp) + ","
                               : std::string(trans ? "rpt," : "rp,");
    k += std::to_string(meqn) + "," + std::to_string(mwaves) + "," + std::to_string(ndim) + "," + std::to_string(math) + ",";
    for (int i = 0; i < naux; i++) k += (i ? "." : "aux") + std::to_string(aux[i]);
    if (naux > 0) k += ",";
    if (form) k += "form" + std::to_string(form) + ",";     // (form 0: the key of before there were forms)
    if (trans) { k += std::to_string(strlen(trans)) + ":"; k += trans; }
    k += std::to_string(strlen(preamble)) + ":";
    k += preamble;
    k += body;
    return k;
}

// the sweep kernels of a UserRp of this dimension, as hiprtc name expressions; uslices > 0 (a transverse body, 2-D): the
// x and y phases of the unsplit step behind them, the tile form of either, without a fused source.  CAPA and FWAVE of every
// one come from the form: a handle serves one form, so only that form's instantiations are compiled
// A SharpClaw handle asks for the SharpClaw kernels of its one (LIM, K, CAPA) and for no classic kernel: sharp_kernel<UserRp,
// 1, CAPA, LIM, K> (1-D), the same and <UserRp, 2, ...> (2-D), or sharp1w_kernel<UserRp, LIM, CAPA> (char_decomp = 1).  The
// kernels have no FWAVE flag: they read s, amdq and apdq alone
static inline std::vector<std::string> cellrp_exprs(int ndim, int math, int uslices = 0, int form = 0,
                                                    const CellrpSharp &sharp = CellrpSharp()) {
    const std::string ns = std::string("pcl::") + cellrp_ns(math) + "::";
    const char *fw = (form & PCL_CELLRP_FORM_FWAVE) ? "true" : "false", *capa = (form & PCL_CELLRP_FORM_CAPA) ? "true" : "false";
    if (sharp.on()) {
        const std::string lim = std::to_string(sharp.lim_type);
        if (sharp.char_decomp == 1) return {"&" + ns + "sharp1w_kernel<" + ns + "UserRp, " + lim + ", " + capa + ">"};
        auto sk = [&](int ixy) {
            return "&" + ns + "sharp_kernel<" + ns + "UserRp, " + std::to_string(ixy) + ", " + capa + ", " + lim + ", " +
                   std::to_string(sharp.mbc()) + ">";
        };
        if (ndim == 1) return {sk(1)};
        return {sk(1), sk(2)};
    }
    auto k = [&](int ixy, bool dim1) {
        return "&" + ns + "sweep_kernel<" + ns + "UserRp, " + std::to_string(ixy) + ", " + capa + ", " + fw + ", " + (dim1 ? "true" : "false") + ">";
    };
    if (ndim == 1) return {k(1, true)};
    if (uslices <= 0) return {k(1, false), k(2, false)};
    const std::string u = std::to_string(uslices);
    return {k(1, false), k(2, false), "&" + ns + "unsplit_x_kernel<" + ns + "UserRp, " + fw + ", " + u + ", " + capa + ">",
            "&" + ns + "unsplit_y_kernel<" + ns + "UserRp, " + fw + ", " + u + ", " + capa + ", false>"};
}

// hiprtc compile of the sweep kernels around body; math: 0 exact, 1 fast, 2 strict.  0 = ok, else err holds the log
// aux[0..naux): the aux components the body reads (naux == 0: the wrapper without aux, the program text of before)
// trans (null: none, the program text of before): the transverse body; uslices: the slices per workgroup of the unsplit
// kernels it is compiled into; sym[2], sym[3]: their lowered names
// form (0: the program text of before): PCL_CELLRP_FORM_* bits; with the f-wave bit the array the body assigns is `fwave`
// sharp (off: the program text of before): a SharpClaw handle; the text includes sharpclaw.hpp, the struct gets no form
// members (the SharpClaw kernels read none) and the name expressions are the SharpClaw kernels alone
static inline int cellrp_build(const char *body, const char *trans, const char *preamble, int meqn, int mwaves, int ndim, int math,
                               const int *aux, int naux, int uslices, int form, const CellrpSharp &sharp, std::vector<char> &code,
                               std::string (&sym)[4], std::string &err) {
    if (hiprtc_load(err)) return -1;
    HiprtcApi &a = hiprtc_api();
    std::string src = sharp.on() ? kCellrpHeadSharp : kCellrpHead;
    src += "#line 1 \"preamble\"\n";
    src += preamble;
    src += "\n#line 1 \"pcl_cellrp_wrapper\"\n";
    if (naux > 0) {
        // the list as a constexpr table: a loop over k unrolls it into the plane offsets of the tile loads
        src += "__host__ __device__ constexpr int cellrp_aux_component(int k) { return ";
        for (int i = 0; i < naux; i++) src += "k == " + std::to_string(i) + " ? " + std::to_string(aux[i]) + " : ";
        src += "0; }\n";
    }
    {
        std::string open = naux > 0 ? kCellrpOpenAux : kCellrpOpen;
        if (form & PCL_CELLRP_FORM_FWAVE) {     // the body's name of the array, as Clawpack's f-wave solvers have it
            const size_t at = open.find("(&wave)");
            open.replace(at, 7, "(&fwave)");
        }
        src += open;
    }
    src += "#line 1 \"riemann\"\n";
    src += body;
    src += "\n";
    src += naux > 0 ? kCellrpTailAux : kCellrpTail;
    if (trans) {
        src += naux > 0 ? kCellrpTransOpenAux : kCellrpTransOpen;
        src += "#line 1 \"transverse\"\n";
        src += trans;
        src += "\n";
        src += naux > 0 ? kCellrpTransTailAux : kCellrpTransTail;
        src += kCellrpTransCheck;
    }
    if (form && !sharp.on()) src += kCellrpForm;
    src += sharp.on() ? kCellrpCloseSharp : naux > 0 ? kCellrpCloseAux : kCellrpClose;
    hiprtcProgram prog = nullptr;
    hiprtcResult r = a.hiprtcCreateProgram(&prog, src.c_str(), "pcl_cellrp.hip", kCellrpHeaderCount, kCellrpHeaderTexts, kCellrpHeaderNames);
    if (r != HIPRTC_SUCCESS) { err = std::string("hiprtcCreateProgram: ") + a.hiprtcGetErrorString(r); return -1; }
    const std::vector<std::string> exprs = cellrp_exprs(ndim, math, trans ? uslices : 0, form, sharp);
    for (const std::string &e : exprs) {
        r = a.hiprtcAddNameExpression(prog, e.c_str());
        if (r != HIPRTC_SUCCESS) {
            err = std::string("hiprtcAddNameExpression: ") + a.hiprtcGetErrorString(r);
            a.hiprtcDestroyProgram(&prog);
            return -1;
        }
    }
    // the flags kernels_<mode>.o is built with (Makefile), then this solver's constants
    std::vector<std::string> flags;
    {
        const std::string all = math == 1 ? PCL_RTC_FLAGS_FAST : math == 2 ? PCL_RTC_FLAGS_STRICT : PCL_RTC_FLAGS_EXACT;
        size_t i = 0;
        while (i < all.size()) {
            const size_t j = all.find(' ', i);
            if (j != i) flags.push_back(all.substr(i, j == std::string::npos ? j : j - i));
            if (j == std::string::npos) break;
            i = j + 1;
        }
    }
    flags.push_back("--offload-arch=" PCL_ARCH);
    flags.push_back("-DPCL_CELLRP_MEQN=" + std::to_string(meqn));
    flags.push_back("-DPCL_CELLRP_MWAVES=" + std::to_string(mwaves));
    flags.push_back("-DPCL_CELLRP_NDIM=" + std::to_string(ndim));
    if (naux > 0) flags.push_back("-DPCL_CELLRP_NAUX=" + std::to_string(naux));
    if (trans) flags.push_back("-DPCL_CELLRP_USLICES=" + std::to_string(uslices));
    if (form || sharp.on()) flags.push_back("-DPCL_CELLRP_FORM=" + std::to_string(form));
    if (sharp.on()) flags.push_back("-DPCL_CELLRP_SHARP_CD=" + std::to_string(sharp.char_decomp));
    std::vector<const char *> opts;
    for (const std::string &f : flags) opts.push_back(f.c_str());
    r = a.hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    if (r != HIPRTC_SUCCESS) {
        size_t n = 0;
        std::string log;
        if (a.hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
            log.resize(n);
            a.hiprtcGetProgramLog(prog, &log[0]);
            while (!log.empty() && (log.back() == '\0' || log.back() == '\n')) log.pop_back();
        }
        err = std::string("Riemann solver body does not compile: ") + a.hiprtcGetErrorString(r) + "\n" + log;
        a.hiprtcDestroyProgram(&prog);
        return -1;
    }
    for (size_t k = 0; k < exprs.size(); k++) {
        const char *low = nullptr;
        r = a.hiprtcGetLoweredName(prog, exprs[k].c_str(), &low);
        if (r != HIPRTC_SUCCESS || !low) {
            err = std::string("hiprtcGetLoweredName: ") + a.hiprtcGetErrorString(r);
            a.hiprtcDestroyProgram(&prog);
            return -1;
        }
        sym[k] = low;
    }
    size_t size = 0;
    r = a.hiprtcGetCodeSize(prog, &size);
    if (r == HIPRTC_SUCCESS && size > 0) {
        code.resize(size);
        r = a.hiprtcGetCode(prog, code.data());
    }
    a.hiprtcDestroyProgram(&prog);
    if (r != HIPRTC_SUCCESS || size == 0) { err = std::string("hiprtcGetCode: ") + a.hiprtcGetErrorString(r); return -1; }
    if (const char *dir = getenv("PCL_CELLFN_DUMP")) {     // diagnostics: keep the code object for a disassembler
        static int seq = 0;
        const std::string path = std::string(dir) + "/riemann_" + std::to_string(seq++) + ".co";
        if (FILE *fp = fopen(path.c_str(), "wb")) { fwrite(code.data(), 1, code.size(), fp); fclose(fp); }
    }
    return 0;
}

// the module a PCL_RP_CELL solver handle has loaded; unloaded by pcl_destroy, never by a static destructor
struct CellrpModule {
    long id = 0;                // 0: nothing attached
    int naux = 0;               // aux components the attached solver reads: its sweeps need the aux array on the device
    hipModule_t mod = nullptr;
    hipFunction_t fn[2] = {nullptr, nullptr};      // by ids - 1
    // the unsplit phases (by ids - 1) of a solver with a transverse body, and its slices per workgroup; else null, 0
    hipFunction_t fn_u[2] = {nullptr, nullptr};
    int slices = 0;
    int form = 0;               // PCL_CELLRP_FORM_* bits of the attached solver: what its kernels were instantiated for
    // a SharpClaw handle: fn holds the SharpClaw kernels (by ids - 1; fn[0] alone with char_decomp = 1) of this lim_type,
    // mbc and char_decomp; sharp_mbc = 0: a classic handle, fn holds the sweeps
    int sharp_lim = 0, sharp_mbc = 0, sharp_cd = 0;
    void unload() {
        if (mod) (void)hipModuleUnload(mod);
        mod = nullptr; fn[0] = fn[1] = fn_u[0] = fn_u[1] = nullptr; id = 0; naux = 0; slices = 0; form = 0;
        sharp_lim = sharp_mbc = sharp_cd = 0;
    }
};

}  // namespace pcl
