// cellrp.hpp -- user-written Riemann solvers: the NORMAL solver of one interface (Clawpack's rp1 / rpn2) given as the
// text of a C++ function body, compiled at run time into the project's own kernels (pyclaw.CellRiemann,
// cfg.rp = PCL_RP_CELL).
//
// Nothing of a kernel is restated here.  The Makefile embeds the headers the kernels are written in -- sweep_args.hpp,
// ghost_rule.hpp, rp.hpp, classic.hpp, classic3.hpp, classic_fused.hpp, sharpclaw.hpp, weno_tables.hpp and include/pyclaw_amd.h -- as text
// (cellrp_headers.inc), hiprtc gets them as named headers, and the program below wraps the user's body in a solver struct
// UserRp of the shape rp.hpp documents and asks for the kernels of that struct by name expression, compiled with the flags
// of the library's own arithmetic mode (PCL_RTC_FLAGS_*, from the Makefile).  A user solver thereby runs with the LDS
// tiles, DPP shifts, limiter, jump-free shortcut and Courant reduction of the built-in solvers, bit for bit; kernels.hip
// fires the launch plan of each kernel family -- grid, block and typed arguments, stated once -- at its own kernel or at the
// module's function in the family's slot (sweep_args.hpp: CellrpSlot).
//
// What a solver is compiled for is one value, CellrpSpec (sweep_args.hpp).  It travels from the pcl_cellrp_compile* call
// through the cache entry (pcl_cellrp) and the loaded module (CellrpModule) to the launchers (SweepLaunch::user, next to the
// module's kernels by slot, SweepLaunch::user_fns); the rules over it are stated once, in cellrp_spec_check (a compile) and
// cellrp_fits (an attach).
//
// THE BODY is the inside of solve():
//     const double ql[MEQN], qr[MEQN]      the cells left and right of the interface
//     const double p[8]                    the solver's parameters (RpParams::v; by value in SweepArgs, so changing them
//                                          compiles nothing)
//     ixy                                  compile-time constant, 1 = x sweep (always in 1-D), 2 = y sweep, 3 = z sweep
//     double wave[MWAVES][MEQN], s[MWAVES], amdq[MEQN], apdq[MEQN]
//                                          the results, zero on entry: what the body never assigns is a compile-time zero
//     dmax, dmin, dsqrt, fdiv, Recip ...   the helpers rp.hpp gives the built-in solvers (a built-in solver restated as a
//                                          body gives the same bits); / and sqrt are IEEE in the exact mode
// and whatever `preamble` declares in front of the struct (helper functions, inside namespace pcl::<mode>).
// Diagnostics carry the user's line numbers: "riemann:3:...", "transverse:2:...", "preamble:1:...".
// The wrapper: Cell { double q[MEQN]; double aux[NAUX]; } with NCELL = MEQN + NAUX and a copying precell; nz() is true
// everywhere; speeds() runs the same body and keeps s alone (the compiler drops the rest), so the speeds of a jump-free
// wavefront are the bits of solve() by construction; ONEK and SHARP* false.
// Contract (wave form, classic kernels): for bitwise-equal ql and qr the waves and fluctuations are zero, whatever aux
// holds -- the jump-free shortcut (classic.hpp, lane_core) compares cL.q with cR.q alone, copies such a
// wavefront through and takes only speeds(cL, cR), each interface with its own auxl / auxr.
//
// PER FIELD OF THE SPEC: the text, the key (cellrp_key), the name expressions (cellrp_exprs), the limits (cellrp_spec_check)
//   meqn, mwaves, ndim, math
//     -DPCL_CELLRP_MEQN / _MWAVES / _NDIM and the namespace and flags of the mode.  1 <= meqn, mwaves <= 8 (MAX_WAVES_K),
//     ndim 1 or 2, 8 parameters.  Kernels: sweep_kernel<UserRp, 1, CAPA, FWAVE, true> (the 1-D step), or <UserRp, 1, ..,
//     false> and <UserRp, 2, .., false> (the x and y passes of step2ds).
//     ndim 3 (pcl_cellrp_compile3 alone; every other call refuses it): sweep3_kernel<UserRp, 1, CAPA>, <UserRp, 2, CAPA>,
//     <UserRp, 3, CAPA>, the x, y and z passes of the dimension-split step3ds -- no 2-D transverse body, no SharpClaw
//     kernels, no f-wave form (sweep3_kernel has none); with trans3 (below) the unsplit step's kernels too.  ixy is 1, 2 or
//     3.  The aux list and CAPA mean what they mean below; all three passes stage q, the listed components and the capacity function in one static tile, so
//     meqn + naux + capa <= sweep3_tile_max_planes() (7, set by the 64 x 17 doubles of the y / z tile: Tile3Shape,
//     classic.hpp).  Such a handle serves cfg.ndim = 3 with method[2] < 0 and mbc = 2 (pcl_create_cellrp), nothing else.
//   trans3   (pcl_cellrp_compile3t, CellRiemann3D(rpt3=..., rptt3=...); 3-D only: 1 an rpt3 text, 2 rpt3 and rptt3)
//     Two more texts, the TRANSVERSE and DOUBLE-TRANSVERSE solvers of the unsplit 3-D step (Clawpack's rpt3 / rptt3): members
//     transverse3<IXYZ, ICOOR> and dtransverse3<IXYZ, ICOOR> of the struct (kCellrpTrans3, where the texts' interface and
//     contract are written down), -DPCL_CELLRP_TRANS3=<n>, the text includes classic3.hpp, and three more name expressions,
//     pieces3_kernel<UserRp, 1>, <UserRp, 2>, <UserRp, 3> (SLOT_PIECES3_X / _Y / _Z): the pieces of every slice of the general
//     unsplit step, which the library's own gather3_kernel applies from scratch planes (launch_unsplit3; the scratch, 14 *
//     meqn doubles per cell with ghost cells -- sweep_args.hpp: unsplit3_scratch_bytes --, is allocated at the attach to an
//     unsplit configuration and freed with the solver).  With rpt3 alone the kernel never names dtransverse3 (UserRp::TRANS3);
//     such a handle serves method[2] = 0, 10, 20, one with both 0, 10, 11, 20, 21, 22 (cellrp_fits).  Wave form without a
//     capacity function only (step3 with mcapa is built for no solver).  pieces3_kernel has no tile: a handle whose
//     meqn + naux exceeds the sweep3 tile is compiled without the three sweeps and serves the unsplit step alone
//     (cellrp_has_sweep3).  Key: prefixes "rpt3," / "rptt3," and the texts.
//   naux, aux[]   (pcl_cellrp_compile_aux, CellRiemann(aux=...))
//     The components of the aux array the body reads.  -DPCL_CELLRP_NAUX=<n> behind a generated constexpr table of the
//     list: NAUX = NAUX_T = n, aux_index<IXY>(k) = auxt_index<IXY>(k) = the k-th listed component (0-based; one list for
//     both sweeps), so the sweep stages those n planes next to q in its LDS tile as it does for vc_acoustics_2d, and
//     precell takes the aux values too.  The body gains
//         const double auxl[NAUX], auxr[NAUX]  the listed components, in list order, of the cell LEFT and of the cell RIGHT
//                                              of the interface (Clawpack's "aux(1) is the value at the left edge of cell
//                                              i" is auxr[0]); a body that needs another component per direction branches
//                                              on ixy
//     A flux-difference form over varying coefficients breaks the contract above: that is an f-wave solver.  Key:
//     "aux<i>.<j>...,".  Limit: the tile holds MEQN + NAUX planes of TileShape<IXY>::PLANE doubles in a workgroup's 64 KB,
//     so meqn + naux <= sweep_tile_max_planes() (8, set by the 1024-double y tile); every index is checked >= 0 and
//     distinct here and the largest against cfg.maux at the attach.
//   trans   (pcl_cellrp_compile_t, CellRiemann(transverse=...); 2-D only)
//     A second text, the TRANSVERSE solver (Clawpack's rpt2): two more members of the struct (kCellrpTrans, where the
//     body's interface and contract are written down), -DPCL_CELLRP_USLICES=<U>, and two more name expressions,
//     unsplit_x_kernel<UserRp, FWAVE, U, CAPA> and unsplit_y_kernel<UserRp, FWAVE, U, CAPA, false> -- the unsplit step
//     (classic.hpp), launched by launch_unsplit with the parameters and grids of the built-in solvers.  U =
//     spec.slices() = unsplit_user_slices(meqn) (sweep_args.hpp: the one rule, read here to name the instantiations, by the
//     text to check them and by the launcher to size its grids).  Always the tile form of the y phase: the marching kernel
//     (its static LDS is 29184 * meqn bytes) stays with the built-in solvers.  Key: prefix "rpt," and the text.
//   form   (pcl_cellrp_compile_form, CellRiemann(fwave=..., capa=...))
//     The pair of template flags every kernel above is instantiated with.  A handle serves one form -- only that form's
//     instantiations are compiled; cfg.fwave and method[5] must say the same (cellrp_fits, and once more the launchers).
//     Key: "form<n>,".
//     PCL_CELLRP_FORM_FWAVE: the body assigns F-WAVES, and the array is named fwave[MWAVES][MEQN] as in Clawpack's f-wave
//       solvers (a body that assigns `wave` does not compile: "riemann:<n>: ... undeclared identifier 'wave'"); everything
//       else the body sees, and the transverse body's interface, are as in wave form.  The "equal q => zero waves"
//       contract does NOT apply: lane_core takes neither jump-free shortcut when FWAVE is set, every interface is solved.
//       UserRp::IS_FWAVE is true.  The limiter and the second-order correction are flux2fw.f's (dsign(1, s)).
//     PCL_CELLRP_FORM_CAPA: the sweeps divide dt/dx by aux(mcapa) per cell and accumulate the reference's Courant
//       expression (cfl_accumulate<true>); the body does not change.  The component is a run-time value, SweepArgs::mcapa,
//       so one handle serves any mcapa.  The sweep tile holds the capacity function's plane too: meqn + 1 + naux <=
//       sweep_tile_max_planes().  The unsplit kernels read capa from global memory per lane and declare no LDS for it, so
//       unsplit_user_slices(meqn) stands as it is.
//   lim_type, weno_order, char_decomp   (pcl_cellrp_compile_sharp, CellRiemann(sharpclaw=True); lim_type 0: a classic handle)
//     The same struct inside the text of sharpclaw.hpp (-DPCL_CELLRP_SHARP=1, -DPCL_CELLRP_SHARP_CD), and the SharpClaw
//     kernels of the one reconstruction the run needs in place of every classic kernel --
//         sharp_kernel<UserRp, 1, CAPA, LIM, K>                                       1-D
//         sharp_kernel<UserRp, 1, CAPA, LIM, K>, sharp_kernel<UserRp, 2, CAPA, LIM, K>  the x and y passes in 2-D
//         sharp1w_kernel<UserRp, LIM, CAPA>                                           char_decomp = 1 (1-D, LIM 1 or 2, K 3)
//     LIM = lim_type 1..3, K = spec.mbc() = (weno_order + 1) / 2 = 3, or 4..9 with LIM 2: any system gets every order,
//     since only one (LIM, K, CAPA) is instantiated.  The kernels have no FWAVE flag -- they read s, amdq, apdq alone; an
//     f-wave body still names its array fwave.  The "equal q => zero waves" contract is not relied on: every interface and
//     the problem inside every cell are solved.  Key: prefix "rps<lim>.<order>.<cd>,".  Such a handle serves cfg.kind =
//     PCL_KIND_SHARPCLAW whose lim_type, mbc, method[4], fwave and method[5] > 0 say the same, and nothing else.  Limit:
//     sharp_kernel's tile is static LDS of TA * 64 doubles per plane, TA = sharp_tile_across (16; 8 in the y pass from six
//     aux components on); the x pass stages meqn + capa planes, the y pass meqn + capa + naux, each within 64 KB
//     (sharp_tile_max_planes, kernels.hip).  sharp1w_kernel declares no LDS.
//     ndim 3 (pcl_cellrp_compile3_sharp alone, SharpCellRiemann3D; pcl_cellrp_compile_sharp goes on refusing ndim 3):
//         sharp3_kernel<UserRp, 1, CAPA, LIM, K>, <UserRp, 2, ..>, <UserRp, 3, ..>     the x, y and z passes of a stage
//     and nothing else -- no classic sweep, no char_decomp, no f-wave form (form may carry PCL_CELLRP_FORM_CAPA only).  One
//     rule for the three tiles: meqn + capa + naux <= SHARP3_MAX_PLANES (8; sharpclaw.hpp).  Such a handle serves cfg.ndim =
//     3 with cfg.kind = PCL_KIND_SHARPCLAW whose lim_type, mbc and method[5] > 0 say the same and method[4] = 0; it is the
//     only way SharpClaw runs in 3-D (no SharpClaw kernel of a built-in 3-D solver is instantiated).
//   onek   (pcl_cellrp_compile_onek, CellRiemann(one_kernel=True); 2-D classic handles only)
//     The dimension-split 2-D step as ONE kernel around the body, next to everything the same call without it compiles:
//     -DPCL_CELLRP_ONEK=1 makes the text include classic_fused.hpp (which includes classic.hpp) and adds one name
//     expression, step2ds_kernel<UserRp, FWAVE, false, CAPA>, behind the others (SLOT_ONEK).  The host then
//     treats the solver like a built-in one with such an instantiation (pclaw.hip: solver_facts): quiet tiles, tile lists,
//     row reuse, the y-column shortcut, the form trials and step ahead for a wave-form body without aux and capa -- all of
//     which rest on the contract above and on nothing else --, the whole block without bookkeeping with an aux list or a
//     capacity function, the FWAVE instantiation (no shortcut, so no quiet tile) for an f-wave body.  launch_step2ds
//     launches it over the grid and with the parameters of the built-in instantiations.  The hand-over and tile-list kernel
//     is not compiled into the module (classic_fused.hpp keeps it behind __HIPCC_RTC__): the library's own serves every
//     solver.  Key: "onek,".  Limits: ndim 2, no SharpClaw handle, meqn <= ONEK_MAX_MEQN (5, the rule of fused_step_ok);
//     the two-pass tile's meqn + capa + naux <= 8 lies inside the one-kernel tile's ONEK_MAX_PLANES (10).  A body heavy
//     enough to spill registers in this kernel is still correct; the form trials then keep the two passes.
// Every plane limit is refused on the host with the sum and restated by a static_assert at the end of the text.
//
// NOT SERVED under SharpClaw: a fused dq source (a source term runs as its own pass), char_decomp 2 / 3, tfluct, a
// transverse body.  Not served in any form: HAS_QCOR (the sphere solver's conservation fix), a transverse body with both
// cells and aux (2-D or 3-D), the marching y phase, f-waves in 3-D, the unsplit 3-D step with a capacity function
// (step3 with mcapa), mbc > 2 in 3-D, more than one block (decomposed runs).
#pragma once
#include "cellfn.hpp"
// generated by the Makefile (embed_headers.py): PCL_RTC_FLAGS_EXACT / _FAST / _STRICT, the flags kernels_<mode>.o is built
// with, and kCellrpHeaderNames[], kCellrpHeaderTexts[], kCellrpHeaderCount
#include "cellrp_headers.inc"

#define PCL_CELLRP_MAX_PARAMS 8

struct pcl_cellrp {
    long id = 0;                // never reused, from the counter of the cell functions
    int refs = 0;
    std::string key;
    std::vector<char> code;     // the code object
    std::string sym[pcl::CELLRP_NSLOTS];        // lowered names of cellrp_exprs(spec), by slot; the rest empty
    pcl::CellrpSpec spec;
};

namespace pcl {

// the texts of one compile, as the caller gave them (transverse null: none)
struct CellrpTexts {
    const char *body = nullptr, *transverse = nullptr, *preamble = nullptr;
    const char *rpt3 = nullptr, *rptt3 = nullptr;       // 3-D: the transverse and double-transverse bodies (null: none)
};

// ---- the program text: each piece once; the spec's -D constants choose inside it ------------------------------------
static const char *const kCellrpHead = R"PCLSRC(
#if PCL_CELLRP_SHARP
#include "sharpclaw.hpp"
#elif PCL_CELLRP_ONEK
#include "classic_fused.hpp"
#elif PCL_CELLRP_TRANS3
#include "classic3.hpp"
#else
#include "classic.hpp"
#endif
namespace pcl {
namespace PCL_NS {
#line 1 "preamble"
)PCLSRC";

// behind the preamble (and, with aux, the generated cellrp_aux_component(k)): the struct up to the body's signature
static const char *const kCellrpStruct = R"PCLSRC(
#if PCL_CELLRP_NAUX > 0
#define PCL_CELLRP_AUX(...) __VA_ARGS__
#else
#define PCL_CELLRP_AUX(...)
#endif
#if PCL_CELLRP_FORM & 1
#define PCL_CELLRP_WAVE fwave
#else
#define PCL_CELLRP_WAVE wave
#endif
struct UserRp : RpDefaults {
    static constexpr int ID = PCL_RP_CELL, NDIM = PCL_CELLRP_NDIM;
    static constexpr int MEQN = PCL_CELLRP_MEQN, MWAVES = PCL_CELLRP_MWAVES, NAUX = PCL_CELLRP_NAUX, NAUX_T = NAUX, NCELL = MEQN + NAUX;
    static constexpr bool IS_FWAVE = (PCL_CELLRP_FORM & 1) != 0;       // what IsFwave<RP> (classic.hpp) reads off a solver
    static_assert(MEQN >= 1 && MEQN <= MAX_WAVES_K && MWAVES >= 1 && MWAVES <= MAX_WAVES_K, "1 <= meqn, mwaves <= 8");
    struct Cell { double q[MEQN]; PCL_CELLRP_AUX(double aux[NAUX];) };
    template <int IXY> __device__ static constexpr bool nz(int, int) { return true; }
#if PCL_CELLRP_NAUX > 0
    template <int IXY> __host__ __device__ static constexpr int aux_index(int k) { return cellrp_aux_component(k); }
    template <int IXY> __host__ __device__ static constexpr int auxt_index(int k) { return cellrp_aux_component(k); }
#endif
    template <int IXY> __device__ static __forceinline__ Cell precell(const double *q, const RpParams & PCL_CELLRP_AUX(, const double *auxv)) {
        Cell c;
#pragma unroll
        for (int m = 0; m < MEQN; m++) c.q[m] = q[m];
#if PCL_CELLRP_NAUX > 0
#pragma unroll
        for (int k = 0; k < NAUX; k++) c.aux[k] = auxv[k];
#endif
        return c;
    }
    template <int ixy>
    __device__ static __forceinline__ void body(const double (&ql)[MEQN], const double (&qr)[MEQN],
                                                PCL_CELLRP_AUX(const double (&auxl)[NAUX], const double (&auxr)[NAUX],)
                                                const double (&p)[8], double (&PCL_CELLRP_WAVE)[MWAVES][MEQN],
                                                double (&s)[MWAVES], double (&amdq)[MEQN], double (&apdq)[MEQN]) {
#line 1 "riemann"
)PCLSRC";

// behind the body: solve() zeroes the results and calls it; speeds() is the same body, the compiler keeps what s needs
static const char *const kCellrpSolve = R"PCLSRC(
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
        body<IXY>(L.q, R.q, PCL_CELLRP_AUX(L.aux, R.aux,) p.v, wave, s, amdq, apdq);
    }
    template <int IXY>
    __device__ static __forceinline__ void speeds(const Cell &L, const Cell &R, const RpParams &p, double (&s)[MWAVES]) {
        double wave[MWAVES][MEQN], amdq[MEQN], apdq[MEQN];
        solve<IXY>(L, R, p, wave, s, amdq, apdq);
    }
)PCLSRC";

// The transverse body (spec.trans): the inside of Clawpack's rpt2 for one interface, two more members of the struct.
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
static const char *const kCellrpTrans = R"PCLSRC(
    template <int ixy>
    __device__ static __forceinline__ void tbody(
#if PCL_CELLRP_NAUX > 0
        const double (&q1)[MEQN], const double (&aux1)[NAUX], const double (&aux_below)[NAUX], const double (&aux_above)[NAUX],
#else
        const double (&ql)[MEQN], const double (&qr)[MEQN],
#endif
        const double (&p)[8], const double (&asdq)[MEQN], double (&bmasdq)[MEQN], double (&bpasdq)[MEQN]) {
#line 1 "transverse"
)PCLSRC";

// behind the transverse body; the slices per workgroup the host named the unsplit kernels with are the rule's, and both
// kernels' static LDS fits
static const char *const kCellrpTransSolve = R"PCLSRC(
    }
#line 1 "pcl_cellrp_wrapper_t"
    template <int IXY>
#if PCL_CELLRP_NAUX > 0
    // (auxo is c1.aux again: one list serves aux_index and auxt_index)
    __device__ static __forceinline__ void transverse_vc(const Cell &c1, const double *, const double *auxb, const double *auxa,
                                                         const RpParams &p, const double (&asdq)[MEQN], double (&bm)[MEQN],
                                                         double (&bp)[MEQN]) {
        double below[NAUX], above[NAUX];
#pragma unroll
        for (int k = 0; k < NAUX; k++) { below[k] = auxb[k]; above[k] = auxa[k]; }
#else
    __device__ static __forceinline__ void transverse(const Cell &L, const Cell &R, const RpParams &p, const double (&asdq)[MEQN],
                                                      double (&bm)[MEQN], double (&bp)[MEQN]) {
#endif
#pragma unroll
        for (int m = 0; m < MEQN; m++) { bm[m] = 0.0; bp[m] = 0.0; }
#if PCL_CELLRP_NAUX > 0
        tbody<IXY>(c1.q, c1.aux, below, above, p.v, asdq, bm, bp);
#else
        tbody<IXY>(L.q, R.q, p.v, asdq, bm, bp);
#endif
    }
    static constexpr int USLICES = PCL_CELLRP_USLICES;
    static_assert(NDIM == 2, "a transverse body belongs to a 2-D solver");
    static_assert(USLICES == unsplit_user_slices(MEQN), "slices per workgroup: not the rule of sweep_args.hpp");
    static_assert(unsplit_x_lds_bytes(MEQN, USLICES) <= UNSPLIT_LDS_LIMIT && unsplit_y_lds_bytes(MEQN, USLICES) <= UNSPLIT_LDS_LIMIT,
                  "the static LDS of unsplit_x_kernel / unsplit_y_kernel (classic.hpp) does not fit a workgroup's 160 KB");
)PCLSRC";

// The 3-D transverse bodies (spec.trans3): the insides of Clawpack's rpt3 and rptt3 for one interface, members
// transverse3<IXYZ, ICOOR> and dtransverse3<IXYZ, ICOOR> of the struct, which pieces3_kernel (classic3.hpp) calls.  Both see
//     ixyz (alias ixy), icoor             compile-time constants: the direction of the normal solve, 1..3; 2 = the split is in
//                                         the y-like direction ixyz + 1, 3 = in the z-like direction ixyz + 2 (cyclic)
//     const double p[8]
// and, without an aux list,
//     const double ql[MEQN], qr[MEQN]     the cells left and right of the interface -- the same pair for A-dq, A+dq and the
//                                         correction wave of one interface: there is no imp
// or, with one,
//     imp                                 1 or 2
//     const double q1[MEQN]               the cell i-2+imp the fluctuation belongs to
//     const double auxb[3][3][NAUX]       auxb[a][b][k]: listed component k of that cell's neighbour at y-like offset a-1 and
//                                         z-like offset b-1 (Clawpack's aux1 / aux2 / aux3(:, i1, 1..3))
// rpt3:   const double asdq[MEQN] in, double bmasdq[MEQN], bpasdq[MEQN] out (zero on entry).
// rptt3:  impt (1: the input came out of a split that went DOWN in the other transverse direction, 2: up), const double
//         bsasdq[MEQN] in, double cmbsasdq[MEQN], cpbsasdq[MEQN] out (zero on entry); the new split lies inside the
//         neighbouring row the input went to (oracle/classic_oracle.c: rptt3_vc_acoustics).
// Contract: for an all-zero input the results are zero.  Diagnostics: "rpt3:<n>", "rptt3:<n>".
#define PCL_CELLRP_T3_ARGS R"PCLSRC(
#if PCL_CELLRP_NAUX > 0
        const int imp, const double (&q1)[MEQN], const double (&auxb)[3][3][NAUX],
#else
        const double (&ql)[MEQN], const double (&qr)[MEQN],
#endif
        const double (&p)[8],)PCLSRC"
static const char *const kCellrpTrans3 = R"PCLSRC(
    template <int ixyz, int icoor>
    __device__ static __forceinline__ void t3body()PCLSRC" PCL_CELLRP_T3_ARGS R"PCLSRC(
        const double (&asdq)[MEQN], double (&bmasdq)[MEQN], double (&bpasdq)[MEQN]) {
        constexpr int ixy = ixyz; (void)ixy;
#line 1 "rpt3"
)PCLSRC";
static const char *const kCellrpTrans3Solve = R"PCLSRC(
    }
#line 1 "pcl_cellrp_wrapper_t3"
    template <int IXYZ, int ICOOR>
    __device__ static __forceinline__ void transverse3(
#if PCL_CELLRP_NAUX > 0
        const int imp, const double (&q1)[MEQN], const double (&auxb)[3][3][NAUX],
#else
        const double (&ql)[MEQN], const double (&qr)[MEQN],
#endif
        const RpParams &p, const double (&asdq)[MEQN], double (&bm)[MEQN], double (&bp)[MEQN]) {
#pragma unroll
        for (int m = 0; m < MEQN; m++) { bm[m] = 0.0; bp[m] = 0.0; }
#if PCL_CELLRP_NAUX > 0
        t3body<IXYZ, ICOOR>(imp, q1, auxb, p.v, asdq, bm, bp);
#else
        t3body<IXYZ, ICOOR>(ql, qr, p.v, asdq, bm, bp);
#endif
    }
)PCLSRC";
static const char *const kCellrpDtrans3 = R"PCLSRC(
    template <int ixyz, int icoor>
    __device__ static __forceinline__ void tt3body()PCLSRC" PCL_CELLRP_T3_ARGS R"PCLSRC(
        const int impt, const double (&bsasdq)[MEQN], double (&cmbsasdq)[MEQN], double (&cpbsasdq)[MEQN]) {
        constexpr int ixy = ixyz; (void)ixy;
#line 1 "rptt3"
)PCLSRC";
static const char *const kCellrpDtrans3Solve = R"PCLSRC(
    }
#line 1 "pcl_cellrp_wrapper_tt3"
    template <int IXYZ, int ICOOR>
    __device__ static __forceinline__ void dtransverse3(
#if PCL_CELLRP_NAUX > 0
        const int imp, const int impt, const double (&q1)[MEQN], const double (&auxb)[3][3][NAUX],
#else
        const int impt, const double (&ql)[MEQN], const double (&qr)[MEQN],
#endif
        const RpParams &p, const double (&bsasdq)[MEQN], double (&cm)[MEQN], double (&cp)[MEQN]) {
#pragma unroll
        for (int m = 0; m < MEQN; m++) { cm[m] = 0.0; cp[m] = 0.0; }
#if PCL_CELLRP_NAUX > 0
        tt3body<IXYZ, ICOOR>(imp, q1, auxb, p.v, impt, bsasdq, cm, cp);
#else
        tt3body<IXYZ, ICOOR>(ql, qr, p.v, impt, bsasdq, cm, cp);
#endif
    }
)PCLSRC";
// behind the 3-D transverse bodies: what pieces3_kernel reads off the struct
static const char *const kCellrpTrans3Close = R"PCLSRC(
    static constexpr int TRANS3 = PCL_CELLRP_TRANS3;
    static_assert(NDIM == 3 && (PCL_CELLRP_FORM & 3) == 0, "rpt3 / rptt3 bodies belong to a 3-D solver in wave form without a capacity function");
)PCLSRC";

// The end of the text: the plane limits the host refused over (cellrp_spec_check), restated.  The classic sweep tile holds
// q, the listed aux components and, with one, the capacity function's plane (sweep_kernel: PAUX = MEQN + 1); sharp_kernel's
// tile is static LDS of NP * TA * WAVE doubles, NP = meqn + capa in the x pass and meqn + capa + naux in the y pass, TA =
// sharp_tile_across<UserRp, IXY>(); sweep3_kernel's (NDIM == 3) is static LDS of (meqn + naux + capa) * Tile3Shape<DIR>::PLANE
// doubles, the rule sweep3_tile_planes() (classic.hpp).
static const char *const kCellrpClose = R"PCLSRC(};
static constexpr int USER_CAPA = (PCL_CELLRP_FORM & 2) != 0 ? 1 : 0;
#if PCL_CELLRP_SHARP
static_assert(UserRp::NDIM == 3 || PCL_CELLRP_SHARP_CD == 1 ||
                  (sizeof(double) * (UserRp::MEQN + USER_CAPA) * sharp_tile_across<UserRp, 1>() * WAVE <= 65536 &&
                   (UserRp::NDIM == 1 ||
                    sizeof(double) * (UserRp::MEQN + USER_CAPA + UserRp::NAUX) * sharp_tile_across<UserRp, 2>() * WAVE <= 65536)),
              "meqn + capa + naux: the LDS tile of sharp_kernel (sharpclaw.hpp) does not fit the 64 KB a workgroup may declare");
static_assert(UserRp::NDIM != 3 || (PCL_CELLRP_SHARP_CD == 0 && (PCL_CELLRP_FORM & 1) == 0 &&
                                    UserRp::MEQN + USER_CAPA + UserRp::NAUX <= SHARP3_MAX_PLANES),
              "a 3-D SharpClaw solver: wave form, char_decomp 0, meqn + capa + naux <= 8 (sharp3_kernel, sharpclaw.hpp)");
#elif PCL_CELLRP_NDIM == 3 && !PCL_CELLRP_SWEEP3
static_assert(PCL_CELLRP_TRANS3 > 0, "a 3-D handle without the three sweeps holds the unsplit step's kernels");
#elif PCL_CELLRP_NDIM == 3
static_assert(sizeof(double) * (UserRp::MEQN + USER_CAPA + UserRp::NAUX) * Tile3Shape<1>::PLANE <= 65536 &&
                  sizeof(double) * (UserRp::MEQN + USER_CAPA + UserRp::NAUX) * Tile3Shape<2>::PLANE <= 65536 &&
                  sizeof(double) * (UserRp::MEQN + USER_CAPA + UserRp::NAUX) * Tile3Shape<3>::PLANE <= 65536 &&
                  UserRp::MEQN + USER_CAPA + UserRp::NAUX <= sweep3_tile_planes(),
              "meqn + naux + capa: the LDS tile of sweep3_kernel (classic.hpp) does not fit the 64 KB a workgroup may declare");
static_assert((PCL_CELLRP_FORM & 1) == 0, "no f-wave form of sweep3_kernel");
#else
static_assert(sizeof(double) * (UserRp::MEQN + USER_CAPA + UserRp::NAUX) * TileShape<2>::PLANE <= 65536 &&
                  sizeof(double) * (UserRp::MEQN + USER_CAPA + UserRp::NAUX) * TileShape<1>::PLANE <= 65536,
              "meqn + capa + naux: the LDS tile of sweep_kernel (classic.hpp) does not fit a workgroup's 64 KB");
#if PCL_CELLRP_ONEK
static_assert(UserRp::NDIM == 2 && UserRp::MEQN <= ONEK_MAX_MEQN && UserRp::MEQN + USER_CAPA + UserRp::NAUX <= ONEK_MAX_PLANES &&
                  sizeof(double) * (UserRp::MEQN + USER_CAPA + UserRp::NAUX) * F_ROWS * F_COLS <= 80 * 1024,
              "meqn, meqn + capa + naux: the LDS tile of step2ds_kernel (classic_fused.hpp) holds up to 5 equations and 10 planes");
#endif
#endif
}  // namespace PCL_NS
}  // namespace pcl
)PCLSRC";

static inline const char *cellrp_ns(int math) { return math == 1 ? "fast" : math == 2 ? "strict" : "exact"; }

// ---- the rules, as functions of the spec alone: 0, or the reason in err ---------------------------------------------
// What no program is compiled for.  given: which pointers of the call were there (body and the handle's place; the
// transverse text; the list of naux > 0 components -- sp.aux holds it only as far as it was given and fits), and whether
// the call asked for a SharpClaw handle (behind its first refusal that is sp.sharp()) or for the 3-D sweeps
// (pcl_cellrp_compile3; every other call goes on refusing ndim == 3).
struct CellrpGiven { bool body_and_out, transverse, aux_list, sharp, dim3, rpt3, rptt3; };
// the reason a handle with the one-kernel step (spec.onek) cannot be compiled for this spec, or null.  Today's only caller
// that sets spec.onek, pcl_cellrp_compile_onek, fills ndim = 2 and no SharpClaw field, so of these only meqn > 5 can be
// reached through the C interface; the other three state the rule for the spec and guard a later entry point that fills
// it otherwise.  The plane limit needs no refusal: the sweep tile's limit, which every 2-D handle meets, lies inside the
// one-kernel tile's ONEK_MAX_PLANES (a static_assert next to sweep_tile_max_planes, kernels.hip).
static inline const char *cellrp_onek_refusal(const CellrpSpec &sp, bool dim3) {
    if (sp.sharp()) return "a SharpClaw handle holds the SharpClaw kernels alone: the one-kernel step is a classic step";
    if (dim3 || sp.ndim == 3) return "a 3-D handle holds the three sweeps alone: the one-kernel step is the dimension-split 2-D step";
    if (sp.ndim != 2) return "the one-kernel step is the dimension-split 2-D step (ndim must be 2)";
    if (sp.meqn > ONEK_MAX_MEQN) return "meqn > 5: the tile of the one-kernel step holds up to 5 equations";
    return nullptr;
}
// a 3-D handle holds the three dimension-split sweeps where their tile takes the solver's planes; one with rpt3 / rptt3 bodies
// and more planes than that is compiled without them and serves the unsplit step alone (pieces3_kernel has no tile)
static inline bool cellrp_has_sweep3(const CellrpSpec &sp) {
    return sp.ndim == 3 && !sp.sharp() && sp.meqn + sp.naux + (sp.capa() ? 1 : 0) <= exact::sweep3_tile_max_planes();
}
static inline int cellrp_spec_check(const CellrpSpec &sp, const CellrpGiven &given, std::string &err) {
    const auto no = [&err](const std::string &why) { err = why; return -1; };
    const auto n = [](int v) { return std::to_string(v); };
    if (given.sharp && given.dim3) {
        // pcl_cellrp_compile3_sharp: the three passes of sharp3_kernel and nothing else, each refusal before the compiler
        const std::string who = "pcl_cellrp_compile3_sharp: ";
        if (sp.form & ~(PCL_CELLRP_FORM_FWAVE | PCL_CELLRP_FORM_CAPA))
            return no(who + "form = " + n(sp.form) + " has a bit that is neither PCL_CELLRP_FORM_FWAVE (1) nor PCL_CELLRP_FORM_CAPA (2)");
        if (sp.fwave())
            return no(who + "PCL_CELLRP_FORM_FWAVE: no f-wave form of the 3-D SharpClaw kernel (sharp3_kernel); form may carry "
                            "PCL_CELLRP_FORM_CAPA only");
        if (sp.lim_type != 1 && sp.lim_type != 2 && sp.lim_type != 3)
            return no(who + "lim_type must be 1 (tvd2), 2 (WENO) or 3 (legacy WENO5), got " + n(sp.lim_type));
        if (sp.weno_order < 5 || sp.weno_order > 17 || sp.weno_order % 2 == 0)
            return no(who + "weno_order must be odd, 5..17, got " + n(sp.weno_order));
        if (sp.weno_order > 5 && sp.lim_type != 2)
            return no(who + "weno_order " + n(sp.weno_order) + " exists for lim_type 2 only, got lim_type " + n(sp.lim_type));
        if (sp.char_decomp != 0) return no(who + "char_decomp must be 0 in 3-D");
        if (sp.meqn < 1 || sp.meqn > PCL_MAX_WAVES || sp.mwaves < 1 || sp.mwaves > PCL_MAX_WAVES)
            return no(who + "1 <= meqn <= 8 and 1 <= mwaves <= 8");
        if (sp.naux >= 0 && sp.meqn + (sp.capa() ? 1 : 0) + sp.naux > exact::sharp3_tile_max_planes())
            return no(who + "meqn + capa + naux = " + n(sp.meqn + (sp.capa() ? 1 : 0) + sp.naux) + ", the tile of the 3-D "
                            "SharpClaw passes holds at most " + n(exact::sharp3_tile_max_planes()) + " planes (q components, the "
                            "capacity function and listed aux components) in the 64 KB a workgroup may declare");
    } else if (given.sharp) {
        // what no SharpClaw kernel exists for, with pcl_create's conditions
        if (sp.lim_type != 1 && sp.lim_type != 2 && sp.lim_type != 3)
            return no("pcl_cellrp_compile_sharp: lim_type must be 1 (tvd2), 2 (WENO) or 3 (legacy WENO5), got " + n(sp.lim_type));
        if (sp.weno_order < 5 || sp.weno_order > 17 || sp.weno_order % 2 == 0)
            return no("pcl_cellrp_compile_sharp: weno_order must be odd, 5..17, got " + n(sp.weno_order));
        if (sp.weno_order > 5 && sp.lim_type != 2)
            return no("pcl_cellrp_compile_sharp: weno_order " + n(sp.weno_order) + " exists for lim_type 2 only, got lim_type " + n(sp.lim_type));
        if (sp.char_decomp != 0 && sp.char_decomp != 1)
            return no("pcl_cellrp_compile_sharp: char_decomp must be 0 or 1 (2, 3 need a user evec routine)");
        if (sp.char_decomp == 1 && (sp.ndim != 1 || sp.lim_type == 3 || sp.weno_order != 5 || sp.fwave()))
            return no("pcl_cellrp_compile_sharp: char_decomp = 1 is the wave-based reconstruction: 1-D, lim_type 1 (tvd2_wave) or 2 "
                      "(weno5_wave), weno_order 5, no f-wave body");
    }
    if (!given.body_and_out) return no("null argument");
    if (sp.onek)
        if (const char *why = cellrp_onek_refusal(sp, given.dim3)) return no(std::string("pcl_cellrp_compile_onek: ") + why);
    if (given.transverse && sp.ndim != 2)
        return no("pcl_cellrp_compile_t: a transverse body belongs to the unsplit 2-D step (ndim must be 2)");
    if (sp.meqn < 1 || sp.meqn > PCL_MAX_WAVES || sp.mwaves < 1 || sp.mwaves > PCL_MAX_WAVES)
        return no("pcl_cellrp_compile: 1 <= meqn <= 8 and 1 <= mwaves <= 8");
    if (given.dim3 ? sp.ndim != 3 : (sp.ndim < 1 || sp.ndim > 2))
        return no("pcl_cellrp_compile: ndim must be 1 or 2 (the classic 1-D and dimension-split 2-D sweeps; the dimension-split "
                  "3-D sweeps are pcl_cellrp_compile3)");
    if (sp.math != PCL_MATH_EXACT && sp.math != PCL_MATH_FAST && sp.math != PCL_MATH_STRICT) return no("unknown math mode");
    // the list of aux components: an index past the solver's maux would be a read outside the aux allocation, so every
    // entry is checked here and the largest against cfg.maux when the handle is attached (cellrp_fits)
    if (sp.naux < 0) return no("pcl_cellrp_compile_aux: naux must be >= 0, got " + n(sp.naux));
    if (sp.naux > 0 && !given.aux_list) return no("null argument");
    const int capa = sp.capa() ? 1 : 0;
    // the 3-D transverse bodies (pcl_cellrp_compile3t): rptt3 splits what an rpt3 returned; 3-D, wave form, no capacity function
    if (given.rptt3 && !given.rpt3)
        return no("pcl_cellrp_compile3t: an rptt3 body without an rpt3 body: the double-transverse solver splits what the "
                  "transverse solver returned");
    if (sp.trans3 != (given.rptt3 ? 2 : given.rpt3 ? 1 : 0) || (sp.trans3 && sp.ndim != 3))
        return no("pcl_cellrp_compile3t: rpt3 / rptt3 bodies belong to the unsplit 3-D step (ndim must be 3)");
    if (sp.trans3 && sp.fwave())
        return no("pcl_cellrp_compile3t: PCL_CELLRP_FORM_FWAVE: no f-wave body in 3-D, with or without rpt3 / rptt3 bodies");
    if (sp.trans3 && sp.capa())
        return no("pcl_cellrp_compile3t: PCL_CELLRP_FORM_CAPA with rpt3 / rptt3 bodies: the unsplit 3-D step (step3) with a "
                  "capacity function (mcapa) is not built for any solver");
    if (sp.ndim == 3 && !sp.sharp()) {
        // the three passes of sweep3_kernel and nothing else: wave form, one tile of meqn + naux + capa planes
        if (sp.form & ~(PCL_CELLRP_FORM_FWAVE | PCL_CELLRP_FORM_CAPA))
            return no("pcl_cellrp_compile3: form = " + n(sp.form) + " has a bit that is neither "
                      "PCL_CELLRP_FORM_FWAVE (1) nor PCL_CELLRP_FORM_CAPA (2)");
        if (sp.fwave())
            return no("pcl_cellrp_compile3: PCL_CELLRP_FORM_FWAVE: no f-wave body in 3-D -- sweep3_kernel has no f-wave "
                      "instantiation, the 3-D launcher refuses an f-wave step, and there is no frozen 3-D f-wave step to check "
                      "one against; form may carry PCL_CELLRP_FORM_CAPA only");
        const int max3 = exact::sweep3_tile_max_planes();
        if (!sp.trans3 && sp.meqn + sp.naux + capa > max3)
            return no("pcl_cellrp_compile3: meqn + naux + capa = " + n(sp.meqn + sp.naux + capa) + ", the tile of the 3-D sweeps "
                      "holds at most " + n(max3) + " planes (q components, listed aux components and the capacity function) in "
                      "the 64 KB a workgroup may declare");
    }
    if (sp.sharp() && sp.char_decomp == 0 && sp.ndim != 3) {
        // the tiles of sharp_kernel: q and the capacity function in the x pass, the listed aux components too in the y
        // pass (sharp1w_kernel, char_decomp = 1, has no tile)
        const int max_x = exact::sharp_tile_max_planes(1, sp.naux), max_y = exact::sharp_tile_max_planes(2, sp.naux);
        if (sp.meqn + capa > max_x)
            return no("pcl_cellrp_compile_sharp: meqn + capa = " + n(sp.meqn + capa) + ", the tile of the SharpClaw x pass "
                      "holds at most " + n(max_x) + " planes (q components and the capacity function) in the 64 KB "
                      "a workgroup may declare");
        if (sp.ndim == 2 && sp.meqn + capa + sp.naux > max_y)
            return no("pcl_cellrp_compile_sharp: meqn + capa + naux = " + n(sp.meqn + capa + sp.naux) + ", the tile of the "
                      "SharpClaw y pass holds at most " + n(max_y) + " planes (q components, the capacity function and "
                      "listed aux components) in the 64 KB a workgroup may declare");
    }
    // the tile of sweep_kernel: q, the listed aux components and the capacity function's plane (PAUX = MEQN + 1)
    const int max_planes = exact::sweep_tile_max_planes();
    if (!sp.sharp() && sp.ndim != 3 && sp.naux > 0 && sp.meqn + sp.naux > max_planes)
        return no("pcl_cellrp_compile_aux: meqn + naux = " + n(sp.meqn + sp.naux) + ", the sweep's tile holds at most " +
                  n(max_planes) + " planes (q components and listed aux components) in a workgroup's 64 KB");
    static_assert(PCL_CELLRP_MAX_AUX >= PCL_MAX_WAVES, "pcl_cellrp_aux writes up to 8 indices");
    if (sp.naux > PCL_CELLRP_MAX_AUX) return no("pcl_cellrp_compile_aux: at most 8 aux components");
    if (sp.form & ~(PCL_CELLRP_FORM_FWAVE | PCL_CELLRP_FORM_CAPA))
        return no("pcl_cellrp_compile_form: form = " + n(sp.form) + " has a bit that is neither "
                  "PCL_CELLRP_FORM_FWAVE (1) nor PCL_CELLRP_FORM_CAPA (2)");
    if (!sp.sharp() && sp.ndim != 3 && capa && sp.meqn + 1 + sp.naux > max_planes)
        return no("pcl_cellrp_compile_form: meqn + 1 + naux = " + n(sp.meqn + 1 + sp.naux) + ", the sweep's tile holds "
                  "at most " + n(max_planes) + " planes (q components, the capacity function and listed aux "
                  "components) in a workgroup's 64 KB");
    for (int i = 0; i < sp.naux; i++) {
        if (sp.aux[i] < 0)
            return no("pcl_cellrp_compile_aux: aux index " + n(sp.aux[i]) + " is negative (0-based components of the aux array)");
        for (int j = 0; j < i; j++)
            if (sp.aux[j] == sp.aux[i]) return no("pcl_cellrp_compile_aux: aux index " + n(sp.aux[i]) + " is listed twice");
    }
    return 0;
}

// the sizes and the mode a handle was compiled for against a solver's
static inline int cellrp_sizes_check(const CellrpSpec &sp, int meqn, int mwaves, int ndim, int math, std::string &err) {
    if (sp.meqn == meqn && sp.mwaves == mwaves && sp.ndim == ndim && sp.math == math) return 0;
    const auto n = [](int v) { return std::to_string(v); };
    err = "Riemann solver was compiled for meqn=" + n(sp.meqn) + " mwaves=" + n(sp.mwaves) + " ndim=" + n(sp.ndim) + " math=" +
          n(sp.math) + ", the solver has meqn=" + n(meqn) + " mwaves=" + n(mwaves) + " ndim=" + n(ndim) + " math=" + n(math);
    return -1;
}

// what attaching a handle compiled for sp to a solver of this configuration asks of the two
static inline int cellrp_fits(const CellrpSpec &sp, const pcl_config &cfg, const char *who, std::string &err) {
    if (cellrp_sizes_check(sp, cfg.meqn, cfg.mwaves, cfg.ndim, cfg.math, err)) return -1;
    const auto no = [&err, who](const std::string &why) { err = who + why; return -1; };
    const auto n = [](int v) { return std::to_string(v); };
    // every aux plane the kernel stages must lie inside the solver's aux allocation of cfg.maux planes
    int top = -1;
    for (int i = 0; i < sp.naux; i++) top = sp.aux[i] > top ? sp.aux[i] : top;
    if (top >= cfg.maux)
        return no(": the Riemann solver reads aux component " + n(top) + " (0-based), the solver was created with maux = " + n(cfg.maux));
    // a handle holds the classic kernels or the SharpClaw kernels of one (lim_type, weno_order, char_decomp), never both
    const bool sharp_cfg = cfg.kind == PCL_KIND_SHARPCLAW;
    if (sharp_cfg != sp.sharp())
        return no(sp.sharp() ? ": PCL_RP_CELL: the handle was compiled for SharpClaw (pcl_cellrp_compile_sharp) "
                               "and the configuration is a classic solver (cfg.kind = 0)"
                             : ": PCL_RP_CELL: a SharpClaw solver (cfg.kind = 1) needs a handle compiled "
                               "for SharpClaw (pcl_cellrp_compile_sharp); this one holds the classic sweeps");
    if (sharp_cfg) {
        if (cfg.lim_type != sp.lim_type)
            return no(": PCL_RP_CELL: the handle was compiled for lim_type " + n(sp.lim_type) + " and cfg.lim_type is " + n(cfg.lim_type));
        if (cfg.mbc != sp.mbc())
            return no(": PCL_RP_CELL: the handle was compiled for weno_order " + n(sp.weno_order) + " (mbc " + n(sp.mbc()) +
                      ") and cfg.mbc is " + n(cfg.mbc) + " (weno_order " + n(2 * cfg.mbc - 1) + ")");
        if (cfg.method[4] != sp.char_decomp)
            return no(": PCL_RP_CELL: the handle was compiled for char_decomp " + n(sp.char_decomp) +
                      " and cfg.method[4] (char_decomp) is " + n(cfg.method[4]));
    }
    // 3-D (f-waves are refused for any handle where the configuration is checked, pcl_create_cellrp)
    if (!sharp_cfg && cfg.ndim == 3 && cfg.method[2] < 0 && sp.ndim == 3 && !cellrp_has_sweep3(sp))
        return no(": PCL_RP_CELL: meqn + naux + capa = " + n(sp.meqn + sp.naux + (sp.capa() ? 1 : 0)) + " is more than the tile of "
                  "the dimension-split 3-D sweeps holds (" + n(exact::sweep3_tile_max_planes()) + " planes): this handle serves the "
                  "unsplit step alone (method[2] >= 0)");
    if (!sharp_cfg && cfg.ndim == 3 && cfg.method[2] >= 0) {
        const int ot = cfg.method[2], m3 = ot / 10, m4 = ot - 10 * m3;
        if (!sp.trans3)
            return no(": PCL_RP_CELL: the unsplit 3-D step (method[2] >= 0, step3) needs a handle compiled with rpt3 and rptt3 "
                      "bodies (pcl_cellrp_compile3t); this one holds the three dimension-split sweeps only");
        if (m3 > 2 || m4 > m3)      // (m4 = 2 splits the corrected increments: it needs the correction waves of m3 = 2)
            return no(": PCL_RP_CELL: method[2] = " + n(ot) + ": the 3-D order_trans must be 0, 10, 11, 20, 21 or 22 (flux3.f:46-73)");
        if (m4 > 0 && sp.trans3 < 2)
            return no(": PCL_RP_CELL: method[2] = " + n(ot) + " asks for double-transverse terms and the handle was compiled "
                      "without an rptt3 body: it serves method[2] = 0, 10 and 20");
        if (cfg.mbc != 2) return no(": PCL_RP_CELL: the unsplit 3-D step needs mbc == 2, got " + n(cfg.mbc));
    }
    if (!sharp_cfg && cfg.ndim == 2 && cfg.method[2] >= 0 && !sp.trans)
        return no(": PCL_RP_CELL: the unsplit step (method[2] >= 0) needs a handle compiled with a transverse body (pcl_cellrp_compile_t)");
    // the kernels in the handle were instantiated for one form (FWAVE, CAPA): the configuration must say the same
    if ((cfg.fwave != 0) != sp.fwave())
        return no(sp.fwave() ? ": PCL_RP_CELL: the handle was compiled for f-waves (PCL_CELLRP_FORM_FWAVE) and cfg.fwave is 0"
                             : ": PCL_RP_CELL: cfg.fwave = 1 asks for f-waves and the handle was compiled in "
                               "wave form (pcl_cellrp_compile_form with PCL_CELLRP_FORM_FWAVE)");
    if ((cfg.method[5] > 0) != sp.capa())
        return no(sp.capa() ? ": PCL_RP_CELL: the handle was compiled for a capacity function "
                              "(PCL_CELLRP_FORM_CAPA) and the solver has none (method[5] is 0)"
                            : ": PCL_RP_CELL: method[5] > 0 asks for a capacity function and the handle "
                              "was compiled without one (pcl_cellrp_compile_form with PCL_CELLRP_FORM_CAPA)");
    return 0;
}

// ---- key, kernels, compile -------------------------------------------------------------------------------------------
static inline std::string cellrp_key(const CellrpSpec &sp, const CellrpTexts &t) {
    const auto n = [](int v) { return std::to_string(v); };
    std::string k = sp.sharp() ? "rps" + n(sp.lim_type) + "." + n(sp.weno_order) + "." + n(sp.char_decomp) + ","
                               : std::string(sp.trans ? "rpt," : "rp,");
    k += n(sp.meqn) + "," + n(sp.mwaves) + "," + n(sp.ndim) + "," + n(sp.math) + ",";
    for (int i = 0; i < sp.naux; i++) k += (i ? "." : "aux") + n(sp.aux[i]);
    if (sp.naux > 0) k += ",";
    if (sp.form) k += "form" + n(sp.form) + ",";
    if (sp.onek) k += "onek,";
    if (sp.trans) { k += n((int)strlen(t.transverse)) + ":"; k += t.transverse; }
    if (sp.trans3) { k = "rpt3," + k + n((int)strlen(t.rpt3)) + ":" + t.rpt3; }
    if (sp.trans3 > 1) { k = "rptt3," + k + n((int)strlen(t.rptt3)) + ":" + t.rptt3; }
    k += n((int)strlen(t.preamble)) + ":";
    k += t.preamble;
    k += t.body;
    return k;
}

// the kernels of a UserRp compiled for sp: the slot of each (sweep_args.hpp: CellrpSlot) and its hiprtc name expression, in
// the order hiprtc gets them (slot order; the one-kernel step behind the expressions of the same spec without it)
using CellrpExprs = std::vector<std::pair<CellrpSlot, std::string>>;
static inline CellrpExprs cellrp_exprs(const CellrpSpec &sp) {
    const auto n = [](int v) { return std::to_string(v); };
    const std::string ns = std::string("pcl::") + cellrp_ns(sp.math) + "::", rp = ns + "UserRp, ";
    const char *fw = sp.fwave() ? "true" : "false", *capa = sp.capa() ? "true" : "false";
    if (sp.sharp()) {
        if (sp.char_decomp == 1) return {{SLOT_SWEEP_X, "&" + ns + "sharp1w_kernel<" + rp + n(sp.lim_type) + ", " + capa + ">"}};
        auto sk = [&](int ixy) { return "&" + ns + "sharp_kernel<" + rp + n(ixy) + ", " + capa + ", " + n(sp.lim_type) + ", " + n(sp.mbc()) + ">"; };
        if (sp.ndim == 1) return {{SLOT_SWEEP_X, sk(1)}};
        if (sp.ndim == 3) {     // x, y, z
            auto s3 = [&](int dir) { return "&" + ns + "sharp3_kernel<" + rp + n(dir) + ", " + capa + ", " + n(sp.lim_type) + ", " + n(sp.mbc()) + ">"; };
            return {{SLOT_SWEEP_X, s3(1)}, {SLOT_SWEEP_Y, s3(2)}, {SLOT_SWEEP_Z, s3(3)}};
        }
        return {{SLOT_SWEEP_X, sk(1)}, {SLOT_SWEEP_Y, sk(2)}};
    }
    if (sp.ndim == 3) {     // x, y, z
        auto k3 = [&](int dir) { return "&" + ns + "sweep3_kernel<" + rp + n(dir) + ", " + capa + ">"; };
        CellrpExprs e3;
        if (cellrp_has_sweep3(sp)) e3 = {{SLOT_SWEEP_X, k3(1)}, {SLOT_SWEEP_Y, k3(2)}, {SLOT_SWEEP_Z, k3(3)}};
        if (sp.trans3)      // the pieces of the unsplit step's slices, x, y, z (classic3.hpp; the gather kernel is the library's)
            for (int dir = 1; dir <= 3; dir++)
                e3.push_back({(CellrpSlot)(SLOT_PIECES3_X + dir - 1), "&" + ns + "pieces3_kernel<" + rp + n(dir) + ">"});
        return e3;
    }
    auto k = [&](int ixy, bool dim1) { return "&" + ns + "sweep_kernel<" + rp + n(ixy) + ", " + capa + ", " + fw + ", " + (dim1 ? "true" : "false") + ">"; };
    if (sp.ndim == 1) return {{SLOT_SWEEP_X, k(1, true)}};
    CellrpExprs e = {{SLOT_SWEEP_X, k(1, false)}, {SLOT_SWEEP_Y, k(2, false)}};
    if (sp.trans) {
        const std::string u = n(sp.slices());
        e.push_back({SLOT_UNSPLIT_X, "&" + ns + "unsplit_x_kernel<" + rp + fw + ", " + u + ", " + capa + ">"});
        e.push_back({SLOT_UNSPLIT_Y, "&" + ns + "unsplit_y_kernel<" + rp + fw + ", " + u + ", " + capa + ", false>"});
    }
    if (sp.onek) e.push_back({SLOT_ONEK, "&" + ns + "step2ds_kernel<" + rp + fw + ", false, " + capa + ">"});
    return e;
}

// hiprtc compile of the kernels of sp around the texts.  0 = ok, else err holds the log
static inline int cellrp_build(const CellrpSpec &sp, const CellrpTexts &t, std::vector<char> &code,
                               std::string (&sym)[CELLRP_NSLOTS], std::string &err) {
    const auto n = [](int v) { return std::to_string(v); };
    HiprtcJob job;
    std::string &src = job.src;
    src = kCellrpHead;
    src += t.preamble;
    src += "\n#line 1 \"pcl_cellrp_wrapper\"\n";
    if (sp.naux > 0) {
        // the list as a constexpr table: a loop over k unrolls it into the plane offsets of the tile loads
        src += "__host__ __device__ constexpr int cellrp_aux_component(int k) { return ";
        for (int i = 0; i < sp.naux; i++) src += "k == " + n(i) + " ? " + n(sp.aux[i]) + " : ";
        src += "0; }\n";
    }
    src += kCellrpStruct;
    src += t.body;
    src += "\n";
    src += kCellrpSolve;
    if (sp.trans) {
        src += kCellrpTrans;
        src += t.transverse;
        src += "\n";
        src += kCellrpTransSolve;
    }
    if (sp.trans3) {
        src += kCellrpTrans3;
        src += t.rpt3;
        src += "\n";
        src += kCellrpTrans3Solve;
        if (sp.trans3 > 1) {
            src += kCellrpDtrans3;
            src += t.rptt3;
            src += "\n";
            src += kCellrpDtrans3Solve;
        }
        src += kCellrpTrans3Close;
    }
    src += kCellrpClose;
    job.name = "pcl_cellrp.hip";
    job.nheaders = kCellrpHeaderCount;
    job.header_texts = kCellrpHeaderTexts;
    job.header_names = kCellrpHeaderNames;
    const CellrpExprs exprs = cellrp_exprs(sp);
    for (const auto &e : exprs) job.exprs.push_back(e.second);
    // the flags kernels_<mode>.o is built with (Makefile), then this solver's constants
    const std::string all = sp.math == 1 ? PCL_RTC_FLAGS_FAST : sp.math == 2 ? PCL_RTC_FLAGS_STRICT : PCL_RTC_FLAGS_EXACT;
    for (size_t i = 0; i < all.size();) {
        const size_t j = all.find(' ', i);
        if (j != i) job.opts.push_back(all.substr(i, j == std::string::npos ? j : j - i));
        if (j == std::string::npos) break;
        i = j + 1;
    }
    job.opts.push_back("--offload-arch=" PCL_ARCH);
    const std::pair<const char *, int> defs[] = {{"MEQN", sp.meqn},        {"MWAVES", sp.mwaves}, {"NDIM", sp.ndim},
                                                 {"NAUX", sp.naux},        {"USLICES", sp.slices()}, {"FORM", sp.form},
                                                 {"SHARP", sp.sharp()},    {"SHARP_CD", sp.char_decomp},
                                                 {"ONEK", sp.onek},         {"TRANS3", sp.trans3},
                                                 {"SWEEP3", cellrp_has_sweep3(sp)}};
    for (const auto &d : defs) job.opts.push_back(std::string("-DPCL_CELLRP_") + d.first + "=" + n(d.second));
    job.what = "Riemann solver body";
    static int seq = 0;
    job.dump = "riemann";
    job.dump_seq = &seq;
    std::vector<std::string> lowered;
    if (hiprtc_compile(job, code, lowered, err)) return -1;
    for (size_t k = 0; k < lowered.size(); k++) sym[exprs[k].first] = lowered[k];
    return 0;
}

// the module a PCL_RP_CELL solver handle has loaded; unloaded by pcl_destroy, never by a static destructor
struct CellrpModule {
    long id = 0;                // 0: nothing attached
    hipModule_t mod = nullptr;
    hipFunction_t fn[CELLRP_NSLOTS] = {};       // the kernels of cellrp_exprs(spec), by slot; the rest null
    CellrpSpec spec;            // what they were compiled for
    void unload() {
        if (mod) (void)hipModuleUnload(mod);
        *this = CellrpModule();
    }
};

}  // namespace pcl
