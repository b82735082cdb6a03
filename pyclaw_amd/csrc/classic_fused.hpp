// classic_fused.hpp -- the dimension-split 2-D step (step2ds.f: x sweeps of every row, then y sweeps of every
// column of the x-swept array) in ONE kernel: q moves through HBM once per STEP instead of once per pass.
//
// Reference path: src/fortran/2d/classic/step2ds.f:83-159 (both loops), flux2.f, limiter.f; boundary conditions as
// the x pass of sweep_kernel evaluates them while loading (solver.py:354-452), the app's radial source applied to the
// finished cell while storing (clawpack.py:156-159) -- the same lane_core, the same order of operations, the same bits
// as the two-pass form (classic.hpp), which stays the path for mbc != 2, for decomposed blocks of solvers with aux arrays
// or a capacity function, and for solvers the launcher (kernels.hip: launch_step2ds) has no instantiation of.
//
// Tile: 16 rows x 64 columns of q with a 2-cell halo on every side, all MEQN planes in LDS (Euler: 40 KB, four
// workgroups of 256 threads per CU; the round's first form was 32 x 64 with 512 threads, two per CU -- measured
// slower, see the tile shape below).  Four phases, a barrier in front of the y sweeps and one behind them:
//   load   the tile, ghost cells remapped to their boundary-condition source cells (tiles on the frame only);
//   x      wavefront w sweeps the four rows it loaded (2w, 2w+1, 8+2w, 9+2w): one lane = one cell, the row is a 64-lane
//          strip exactly as in the x pass; the 60 inner lanes put the updated cell back IN PLACE (interior columns only:
//          ghost columns are copied through, step2ds.f:141-146).  All 16 rows are swept: the y sweeps below need q* two
//          rows beyond the rows they update;
//   y      a wavefront takes FOUR columns at a time, 16 rows each (lanes 16h .. 16h+15 = the rows of column c+h; the
//          wavefront shifts across those boundaries only feed halo rows): rows 2..13 of the interior columns put the
//          finished cell back in place;
//   store  rows 2..13 x columns 2..61 (interior cells only), 16 bytes per lane.
// HBM traffic per cell and step: (16*64)/(12*60) reads + 1 write of q = 96.9 B for Euler (32 x 64: 88.8 B) instead of
// 2 x 82.5 B.  The halo rows / columns are computed twice (x phase 16/12 of the rows, y phase 16/12 of the lanes), which
// the wave-uniform no-jump shortcut of lane_core makes cheap wherever the gas is undisturbed -- and there a wavefront
// remembers the last undisturbed state it met (NoJumpMemo, classic.hpp): the same state again costs MEQN compares.
// LDS layout: row-major rows of 64 doubles, the column XOR-swizzled with the row (fswz): the x phase (lanes = columns)
// touches 64 consecutive doubles, the y phase (lanes = rows) 32 distinct 8-byte banks per half-wave.
#pragma once
#include "classic.hpp"

namespace pcl {
namespace PCL_NS {

// Tile shape: 16 x 64 with 256 threads, four 40 KB workgroups per CU for Euler.  32 x 64 with 512 threads is two
// 80 KB workgroups per CU; 16 x 64 and 32 x 32 with 256 threads are four of 40 KB (shorter phases, more of them
// in flight, for 17 % / 7 % more halo work).  Same box, 4096^2 shock-bubble state, ms per step: 32 x 64 0.350, 16 x 64
// 0.331, 32 x 32 0.370 (its 256-byte row pieces stream badly: 0.376 even without arithmetic); dense state 0.835 / 0.94 /
// 0.86 -- there the solver runs the two passes anyway (pclaw.hip, form trials).
constexpr int F_ROWS = 16, F_COLS = 64;
constexpr int F_OWN_R = F_ROWS - 2 * HALO, F_OWN_C = F_COLS - 2 * HALO;
constexpr int F_THREADS = 256, F_WAVES = F_THREADS / WAVE;
constexpr int F_RX = WAVE / F_COLS;          // rows of the tile one wavefront sweeps at a time (x sweeps)
constexpr int F_CY = WAVE / F_ROWS;          // columns one wavefront sweeps at a time (y sweeps)
constexpr int F_PPR = F_COLS / 2;            // 16-byte pairs per tile row
constexpr int F_NK = F_ROWS * F_PPR / F_THREADS;        // 16-byte loads per thread and plane
constexpr int F_SPK = (WAVE / F_PPR) / F_RX;            // x sweeps that cover the rows of one such load
constexpr int F_NS = F_NK * F_SPK;                      // x sweeps per wavefront
static_assert(F_COLS * F_RX == WAVE && F_ROWS * F_CY == WAVE && F_OWN_C % 2 == 0, "tile shape");
static_assert(F_ROWS * F_PPR % F_THREADS == 0 && (WAVE / F_PPR) % F_RX == 0, "tile shape");
static_assert(F_NS * F_RX * F_WAVES == F_ROWS && (F_COLS / F_CY) % F_WAVES == 0, "tile shape");

// first row of the tile wavefront w loads and sweeps in its x sweep k = 0..F_NS-1 (16 x 64, 256 threads: 2w, 2w+1,
// 8+2w, 9+2w -- what the threads taking the tile's 16-byte pairs in order give it); lanes >= F_COLS take the next row
__device__ __forceinline__ int wave_row(int w, int k) {
    return (F_THREADS * (k / F_SPK) + WAVE * w) / F_PPR + (k % F_SPK) * F_RX;
}
// column swizzle of row r: a half-wave of the y sweeps (32 / F_ROWS columns x F_ROWS rows) must hit 32 distinct banks
__device__ __forceinline__ int fswz(int r) { return F_ROWS >= 32 ? r : r * (32 / F_ROWS); }
__device__ __forceinline__ int ftile_at(int m, int r, int c) { return (m * F_ROWS + r) * F_COLS + (c ^ fswz(r)); }

// Quiet tiles.  A tile is quiet in a launch when every x-sweep and every y-sweep wavefront took the
// no-jump shortcut (and, under the fused source, every cell it stored satisfies euler_radial_source_fixed): its owned
// cells leave the kernel as they came, whatever dt.  tq_out[tile] gets one byte per wavefront (TQ_QUIET or 0), tq_cfl
// the quiet wavefront's largest |speed| of each sweep, before the multiplication by dt/d.  A tile off the frame whose
// 3 x 3 neighbourhood was quiet in launch n reads the same 16 x 64 cells in launch n + 1 if that launch runs on the
// swapped buffer pair (its input is launch n's output, its output launch n's input) with the same solver: it would be
// quiet again, and its owned cells in qout already hold the result.  The rule reads launch n's words and the grid, not
// dt, so handover_list_kernel lists launch n + 1's tiles right behind launch n; step2ds_kernel then runs over the list.
constexpr unsigned TQ_QUIET = 1u, TQ_ALL = 0x01010101u;
static_assert(F_WAVES == 4, "one quiet byte per wavefront in a 32-bit word");

// The Courant hand-over behind a one-kernel launch of the whole block, with the next launch's tile list.  Workgroup 0
// does what cfl_handover (pclaw.hip) does and nothing else: read the step's word, re-zero it, store the value and then
// the sequence number to host memory (system-scope release), so the host's poll waits for nothing else; next to the value
// it leaves the number of tiles the launch just run was dispatched for (the na + nq of the list it ran over, *ran, or
// every tile: the host's form-trial gate, pclaw.hip), and it zeroes *other for the hand-over after next.  Workgroups 1..
// take one tile per thread (row-major): a tile off the frame whose
// 3 x 3 neighbourhood was quiet in tq_in (the launch just run) is skipped by the next launch -- its word in tq_out, the
// next launch's words, becomes TQ_ALL, and its cached Courant maxima go into next->cx / next->cy (an atomic max of bit
// patterns: doubles >= +0, dt-free; the next launch multiplies by dt/d) -- every other tile is
// listed, in two classes: class A (its own word in tq_in is not TQ_ALL: it computed something) from the front of list,
// class Q (quiet itself, listed for a neighbour or the frame) from the back, downward from index ntx * nty - 1.  Within
// a workgroup's range of tiles each class keeps their order (ballot and prefix), the ranges take their places with one
// atomic per class (next->na, next->nq).  *next was zeroed by the hand-over before the previous one.
// Every atomic of the launch lands on the one TileNext block, where they serialise, so a workgroup is
// 1024 tiles and issues at most four: the maxima of its 16 wavefronts meet in LDS behind the barrier the prefix needs
// anyway, one thread issues the max of each word, and none when it is 0 (the same word: an integer max of the same set
// of patterns, in any grouping).
// Not part of the run-time program of a user-written Riemann solver (cellrp.hpp: spec.onek): the library's own copy serves
// every solver, so the module of such a solver holds step2ds_kernel alone.
#ifndef __HIPCC_RTC__
constexpr int TL_THREADS = 1024, TL_WAVES = TL_THREADS / WAVE;
__global__ __launch_bounds__(TL_THREADS) void handover_list_kernel(unsigned long long *cfl, unsigned long long *host,
                                                                   unsigned long long seq, int ntx, int nty, int mbc,
                                                                   int mx, int my, const unsigned *__restrict__ tq_in,
                                                                   unsigned *__restrict__ tq_out,
                                                                   const double2 *__restrict__ tq_cfl,
                                                                   int *__restrict__ list, TileNext *next,
                                                                   TileNext *other, const TileNext *ran) {
    __shared__ int wbase[2][TL_WAVES];
    __shared__ int base[2];
    __shared__ unsigned long long wmax[2][TL_WAVES];
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) {
            const unsigned long long v = *cfl;
            *cfl = 0;                    // invariant: the word is zero whenever no step is in flight
            const int nt = ntx * nty;
            const int ran_over = ran ? min(ran->na + ran->nq, nt) : nt;
            __hip_atomic_store(host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host + 2, (unsigned long long)ran_over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(host + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            other->na = 0;
            other->nq = 0;
            other->cx = 0;
            other->cy = 0;
        }
        return;
    }
    const int t = (blockIdx.x - 1) * TL_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    bool skip = false, own_quiet = false;
    unsigned long long bx = 0, by = 0;               // the skipped tile's largest cached maxima (bits); 0 adds nothing
    if (t < ntx * nty) {
        // off the frame (the tile's 16 x 64 load reads interior cells only): 1 <= tx < ntx - 1, 1 <= ty < nty - 1
        const int tx = t % ntx, ty = t / ntx;
        const int x0 = mbc - HALO + tx * F_OWN_C, y0 = mbc - HALO + ty * F_OWN_R;
        own_quiet = tq_in[t] == TQ_ALL;
        if (x0 >= mbc && y0 >= mbc && x0 + F_COLS <= mbc + mx && y0 + F_ROWS <= mbc + my) {
            const unsigned *w = tq_in + t - ntx - 1;
            skip = true;
#pragma unroll
            for (int dy = 0; dy < 3; dy++)
#pragma unroll
                for (int dx = 0; dx < 3; dx++) skip = skip & (w[dy * ntx + dx] == TQ_ALL);
        }
        if (skip) {
            tq_out[t] = TQ_ALL;
#pragma unroll
            for (int wq = 0; wq < F_WAVES; wq++) {
                const double2 c = tq_cfl[t * F_WAVES + wq];
                const unsigned long long x = (unsigned long long)__double_as_longlong(c.x);
                const unsigned long long y = (unsigned long long)__double_as_longlong(c.y);
                bx = x > bx ? x : bx;
                by = y > by ? y : by;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long ox = __shfl_xor(bx, off, WAVE), oy = __shfl_xor(by, off, WAVE);
        bx = ox > bx ? ox : bx;
        by = oy > by ? oy : by;
    }
    // class A (c = 0) and class Q (c = 1): the workgroup's prefix per wavefront, one atomic per class
    const bool listed = t < ntx * nty && !skip;
    const unsigned long long keep[2] = {__ballot(listed && !own_quiet), __ballot(listed && own_quiet)};
    if (lane == 0) {
        wmax[0][wv] = bx;
        wmax[1][wv] = by;
        wbase[0][wv] = __popcll(keep[0]);
        wbase[1][wv] = __popcll(keep[1]);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int c = threadIdx.x;
        int n = 0;
#pragma unroll
        for (int k = 0; k < TL_WAVES; k++) {
            const int m = wbase[c][k];
            wbase[c][k] = n;
            n += m;
        }
        base[c] = n ? atomicAdd(c ? &next->nq : &next->na, n) : 0;
    } else if (wv == 1 && lane < 2) {        // another wavefront than the prefix': the workgroup's two maxima
        unsigned long long b = 0;
#pragma unroll
        for (int k = 0; k < TL_WAVES; k++) b = wmax[lane][k] > b ? wmax[lane][k] : b;
        if (b) atomicMax(lane ? &next->cy : &next->cx, b);
    }
    __syncthreads();
    if (listed) {
        const int c = own_quiet ? 1 : 0;
        const int i = base[c] + wbase[c][wv] + __popcll(keep[c] & ((1ull << lane) - 1));
        list[c ? ntx * nty - 1 - i : i] = t;
    }
}
#endif  // !__HIPCC_RTC__

// The ring check of a class-Q tile: its owned interior cells all compare equal to one state S (the
// launch before found the whole window uniform and left them as they were), so the window is uniform again exactly
// when every OTHER cell of it, taken as the load phase would put it into the tile, compares equal to S -- == on every
// component, as lane_core's no-jump test: a NaN is unequal, +0 equals -0.  S is the tile's first owned cell (tile row
// and column HALO: interior in every tile).  Tiles loaded straight take the ring in 16-byte pairs, rows 0-1 and 14-15
// and the two halo pairs of rows 2-13 (152 pairs, one per thread); frame and partial tiles take the cells of the
// scalar load, four per thread, less the owned interior ones.  One flag per wavefront in flags[0 .. F_WAVES-1] (the
// tile, not loaded yet), one barrier: the same answer in every thread of the workgroup.
template <int MEQN, class LOAD>
__device__ __forceinline__ bool ring_uniform(const SweepArgs &a, int x0, int y0, bool straight, bool vbc, double *flags,
                                             const LOAD &load_mapped_cell) {
    static_assert(HALO == 2, "a 16-byte pair is the halo columns of one side");
    double s[MEQN];
    const long g0 = (long)(y0 + HALO) * a.pitch + (x0 + HALO);
#pragma unroll
    for (int m = 0; m < MEQN; m++) s[m] = a.qin[m * a.plane + g0];
    bool eq = true;
    if (straight) {
        constexpr int ROWP = 2 * HALO * F_PPR, SIDEP = 2 * F_OWN_R;     // pairs of the four halo rows, of the sides
        static_assert(ROWP + SIDEP <= F_THREADS, "one pair per thread");
        const int t = threadIdx.x;
        if (t < ROWP + SIDEP) {
            const int k = t < ROWP ? t / F_PPR : (t - ROWP) / 2;
            const int r = t < ROWP ? (k < HALO ? k : F_ROWS - 2 * HALO + k) : HALO + k;
            const int c = t < ROWP ? 2 * (t % F_PPR) : (((t - ROWP) & 1) ? F_COLS - HALO : 0);
            const long g = (long)(y0 + r) * a.pitch + (x0 + c);
#pragma unroll
            for (int m = 0; m < MEQN; m++) {
                const double2 v = *reinterpret_cast<const double2 *>(&a.qin[m * a.plane + g]);
                eq = eq & (v.x == s[m]) & (v.y == s[m]);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < F_ROWS * F_COLS / F_THREADS; k++) {
            const int r = wave_row(threadIdx.x / WAVE, k) + (threadIdx.x & (WAVE - 1)) / F_COLS, c = threadIdx.x & (F_COLS - 1);
            const int gx = x0 + c, gy = y0 + r;
            const bool own = r >= HALO && r < F_ROWS - HALO && c >= HALO && c < F_COLS - HALO && gx >= a.mbc &&
                             gx < a.mbc + a.mx && gy >= a.mbc && gy < a.mbc + a.my;
            if (!own) {
                double v[MEQN];
                load_mapped_cell(vbc, gx < a.I ? gx : a.I - 1, gy < a.J ? gy : a.J - 1, v);
#pragma unroll
                for (int m = 0; m < MEQN; m++) eq = eq & (v[m] == s[m]);
            }
        }
    }
    const bool weq = __all(eq);
    if ((threadIdx.x & (WAVE - 1)) == 0) flags[threadIdx.x / WAVE] = weq ? 1.0 : 0.0;
    __syncthreads();
    bool all = true;
#pragma unroll
    for (int w = 0; w < F_WAVES; w++) all = all & (flags[w] == 1.0);
    return all;
}

// Full launches: workgroup b takes tile b (through the chunked order below).  List launches (tq_list set, one
// workgroup per tile of the grid): workgroup 0 first publishes the Courant number of the skipped tiles, dt/d times the
// maxima tq_next holds; then workgroup b takes the b-th listed tile, through the same order -- the na tiles of class A
// from the front of the list, then the nq of class Q from its back -- and the workgroups past the list's end return at
// once.  Dispatch order puts the listed tiles first and, among them, the tiles that compute (those
// set the kernel's end when they wait for a slot behind the quiet ones).
//
// Solvers with cell-wise coefficients (RP::NAUX > 0) and capacity functions (CAPA): the tile holds more planes, laid out
// as sweep_kernel's (classic.hpp) -- q (0 .. MEQN-1), the capacity function aux(mcapa) (CAPA), then the RP::NAUX aux
// components the normal solver reads -- with the same halo and the same swizzle.  aux is the same for both sweeps, is
// loaded once per tile and never written; its ghost cells are real memory (auxbc is filled at setup), so the boundary
// remap of the load applies to the q planes alone.  Each sweep hands lane_core the cell's dt/d divided by its capa and
// the staged aux values exactly as the pass of sweep_kernel does: the same bits.  A tile plane is 8 KB and a CU has
// 160 KB of LDS: up to 5 planes run four workgroups per CU, 6 three, 7 to 10 two (fused_wgs: also the register budget).
// The quiet-tile bookkeeping (tq_*) is for the aux-free instantiations without capa only: the launcher refuses it here.
template <class RP, bool CAPA> constexpr int fused_planes() { return RP::MEQN + (CAPA ? 1 : 0) + RP::NAUX; }
template <class RP> constexpr bool fused_aux_same() {
    bool ok = true;
    if constexpr (RP::NAUX > 0)
        for (int k = 0; k < RP::NAUX; k++) ok = ok && aux_idx<RP, 1>(k) == aux_idx<RP, 2>(k);
    return ok;
}
constexpr int fused_wgs(int planes) { return planes <= 5 ? 1024 / F_THREADS : (20 / planes >= 1 ? 20 / planes : 1); }
template <class RP, bool FWAVE, bool SRC, bool CAPA = false>
__global__ __launch_bounds__(F_THREADS, fused_wgs(fused_planes<RP, CAPA>())) void step2ds_kernel(SweepArgs a, int ntx, int nty,
                                                                              unsigned *__restrict__ tq_out,
                                                                              double2 *__restrict__ tq_cfl,
                                                                              const int *__restrict__ tq_list,
                                                                              const TileNext *tq_next,
                                                                              unsigned *__restrict__ tq_ring, unsigned ring_seq,
                                                                              unsigned *__restrict__ tq_reuse, int rowreuse,
                                                                              unsigned *__restrict__ tq_ycol, int ycol) {
    constexpr int MEQN = RP::MEQN;
    constexpr int NAUX = RP::NAUX, PAUX = MEQN + (CAPA ? 1 : 0), NP = PAUX + NAUX, NX = NP - MEQN;
    static_assert(!SRC || (MEQN == 5 && NX == 0), "fused source: the Euler solver, no capacity function");
    static_assert(NP * F_ROWS * F_COLS * sizeof(double) <= 80 * 1024, "two workgroups per CU at least");
    __shared__ __attribute__((aligned(16))) double tile[NP * F_ROWS * F_COLS];
    // where tile plane MEQN + e comes from in a.aux (one set for both sweeps: checked against aux_idx<RP, 2> below)
    auto xplane = [&](int e) -> long {
        if (CAPA && e == 0) return (long)(a.mcapa - 1) * a.plane;
        return (long)aux_idx<RP, 1>(e - (CAPA ? 1 : 0)) * a.plane;
    };
    static_assert(fused_aux_same<RP>(), "one staging serves both sweeps: the normal solver reads the same aux planes in x and y");

    // One cell of the tile as the load phase puts it there: array cell (gx, gy), already clamped to the array.  On a frame
    // tile of a device-side boundary condition (vbc) a ghost cell is its source cell, mirrored, or the side's constant:
    // qbc = Y(X(q)), x sides first, then y sides over the x-filled array (solver.py:354-381).  (A lambda over the kernel's
    // own argument block: through a reference parameter the selects between two constants cost every instance scratch.)
    auto load_mapped_cell = [&a](bool vbc, int gx, int gy, double (&v)[MEQN]) {
        if (vbc) {
            const VbcMap mi = vbc_map(gx, a.I, a.mbc, a.vbc[0], a.vbc[1]);
            const VbcMap mj = vbc_map(gy, a.J, a.mbc, a.vbc[2], a.vbc[3]);
            const long gs = (long)mj.src * a.pitch + mi.src;
#pragma unroll
            for (int m = 0; m < MEQN; m++) {
                double w = a.qin[m * a.plane + gs];
                if (m == 1) w = mi.neg ? -w : w;
                const double cx = mi.side ? a.vconst[1][m] : a.vconst[0][m];
                w = mi.cst ? cx : w;
                if (m == 2) w = mj.neg ? -w : w;
                const double cy = mj.side ? a.vconst[3][m] : a.vconst[2][m];
                w = mj.cst ? cy : w;
                v[m] = w;
            }
        } else {
            const long g = (long)gy * a.pitch + gx;
#pragma unroll
            for (int m = 0; m < MEQN; m++) v[m] = a.qin[m * a.plane + g];
        }
    };

    // Chunked order: the hardware deals consecutive workgroups to the 8 XCDs in turn; in every window of 64 tiles each
    // XCD takes 8 CONSECUTIVE tiles of a tile row (they share partial lines and halo columns in that XCD's L2) while the
    // windows still walk the grid in row order: without arithmetic 0.288 -> 0.274 ms, the shock-bubble step 0.331 ->
    // 0.330 (16 x 64, before the memo).  The XCD-contiguous order of xcd_logical_block costs this kernel 2-3 % although
    // it saves HBM reads; column bands per XCD (a tile's four neighbours on the same XCD) measured 25 % slower on the
    // shock-bubble state, equal without arithmetic.  A list launch takes its list entries in the same order.
    int bid = blockIdx.x;
    if (tq_list && bid == 0 && threadIdx.x == 0) {
        // the skipped tiles' Courant number: max over tiles and wavefronts of dmax(fl(dtd * cx), fl(dtd_t * cy)) is
        // dmax(fl(dtd * max cx), fl(dtd_t * max cy)) (the same bits); 0 publishes nothing
        const double c = dmax(a.dtd * __longlong_as_double((long long)tq_next->cx),
                              a.dtd_t * __longlong_as_double((long long)tq_next->cy));
        const unsigned long long bits = (unsigned long long)__double_as_longlong(c);
        if (bits) atomicMax(a.cfl, bits);
    }
    const int nt = ntx * nty;
    const int na = tq_list ? min(tq_next->na, nt) : 0;
    const int nb = tq_list ? min(na + tq_next->nq, nt) : (int)gridDim.x;
    if (bid >= nb) return;                           // past the list: the whole workgroup, before any barrier
    const int win = bid >> 6;
    if ((win + 1) << 6 <= nb) bid = (win << 6) + ((bid & 7) << 3) + ((bid >> 3) & 7);
    // class Q: the tile's own word was TQ_ALL in the launch before (handover_list_kernel)
    const bool class_q = tq_list && bid >= na;
    if (tq_list) bid = tq_list[class_q ? nt - 1 - (bid - na) : bid];
    int tx = bid % ntx, ty = bid / ntx;
    if (a.sub != 0) {
        // decomposed block (pclaw.hip): the tiles inside box = [ty_lo, ty_hi) x [tx_lo, tx_hi) read no ghost cell a
        // neighbour block has to send -- sub 1 = those (they run beside the halo exchange), 2 = the others
        const int bw = a.box[3] - a.box[2];
        if (a.sub == 1) {
            ty = a.box[0] + bid / bw;
            tx = a.box[2] + bid % bw;
        } else {
            const int top = a.box[0] * ntx, bot = (nty - a.box[1]) * ntx;
            if (bid < top) {
                ty = bid / ntx;
                tx = bid % ntx;
            } else if (bid < top + bot) {
                bid -= top;
                ty = a.box[1] + bid / ntx;
                tx = bid % ntx;
            } else {
                bid -= top + bot;
                const int side = ntx - bw;
                const int k = bid % side;
                ty = a.box[0] + bid / side;
                tx = k < a.box[2] ? k : a.box[3] + (k - a.box[2]);
            }
        }
    }
    const int x0 = a.mbc - HALO + tx * F_OWN_C;      // array column of tile column 0 (a.mbc == HALO: checked by the launcher)
    const int y0 = a.mbc - HALO + ty * F_OWN_R;
    const int tile_id = ty * ntx + tx;

    // ---- load ----------------------------------------------------------------------------------------------------
    const bool full_tile = x0 + F_COLS <= a.I && y0 + F_ROWS <= a.J;
    const bool vbc_tile = a.vbc_on && ((x0 < a.mbc && a.vbc[0] >= 0) || (x0 + F_COLS > a.I - a.mbc && a.vbc[1] >= 0) ||
                                       (y0 < a.mbc && a.vbc[2] >= 0) || (y0 + F_ROWS > a.J - a.mbc && a.vbc[3] >= 0));
    if constexpr (!SRC && !FWAVE && NX == 0) {
        // A class-Q tile whose ring compares equal to its owned cells is quiet again: every sweep would
        // take the shortcut, qout holds the result, and the wavefronts' cached maxima are what they would compute.  Each
        // wavefront leaves its quiet byte and publishes its Courant number; tq_ring gets the launch's number (the test
        // hook pcl_tile_ring_stats counts them).  tq_ring null: the check is switched off (pcl_tile_ring).
        if (class_q && tq_ring) {                     // workgroup-uniform
            if (ring_uniform<MEQN>(a, x0, y0, full_tile && !vbc_tile, vbc_tile, tile, load_mapped_cell)) {
                const int wv = threadIdx.x / WAVE;
                const double2 c = tq_cfl[tile_id * F_WAVES + wv];
                if ((threadIdx.x & (WAVE - 1)) == 0) {
                    reinterpret_cast<unsigned char *>(tq_out + tile_id)[wv] = TQ_QUIET;
                    if (wv == 0) tq_ring[tile_id] = ring_seq;
                }
                cfl_publish(a.cfl, dmax(a.dtd * c.x, a.dtd_t * c.y));
                return;
            }
            __syncthreads();                          // the flags lie in the tile: every wavefront has read them
        }
    }
    if (full_tile && !vbc_tile) {
#pragma unroll
        for (int k = 0; k < F_ROWS * F_COLS / 2 / F_THREADS; k++) {
            const int slot = threadIdx.x + F_THREADS * k;
            const int r = slot / (F_COLS / 2), c = 2 * (slot % (F_COLS / 2));
            const long g = (long)(y0 + r) * a.pitch + (x0 + c);
#pragma unroll
            for (int m = 0; m < MEQN; m++) {
                double2 v = *reinterpret_cast<const double2 *>(&a.qin[m * a.plane + g]);
                if (fswz(r) & 1) { const double t = v.x; v.x = v.y; v.y = t; }       // the swizzle swaps the pair in odd rows
                *reinterpret_cast<double2 *>(&tile[(m * F_ROWS + r) * F_COLS + ((c ^ fswz(r)) & ~1)]) = v;
            }
            if constexpr (NX > 0) {
#pragma unroll
                for (int e = 0; e < NX; e++) {
                    double2 v = *reinterpret_cast<const double2 *>(&a.aux[xplane(e) + g]);
                    if (fswz(r) & 1) { const double t = v.x; v.x = v.y; v.y = t; }
                    *reinterpret_cast<double2 *>(&tile[((MEQN + e) * F_ROWS + r) * F_COLS + ((c ^ fswz(r)) & ~1)]) = v;
                }
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < F_ROWS * F_COLS / F_THREADS; k++) {
            // the rows this thread's WAVEFRONT sweeps (wave_row below): the same rows the 16-byte path gives it
            const int r = wave_row(threadIdx.x / WAVE, k) + (threadIdx.x & (WAVE - 1)) / F_COLS, c = threadIdx.x & (F_COLS - 1);
            int gx = x0 + c, gy = y0 + r;
            gx = gx < a.I ? gx : a.I - 1;            // past the edge: repeat the last cell (never feeds a stored value)
            gy = gy < a.J ? gy : a.J - 1;
            double v[MEQN];
            load_mapped_cell(vbc_tile, gx, gy, v);
#pragma unroll
            for (int m = 0; m < MEQN; m++) tile[ftile_at(m, r, c)] = v[m];
            if constexpr (NX > 0) {          // the cell's own aux, on the frame too (ghost cells of aux are real memory)
                const long ga = (long)gy * a.pitch + gx;
#pragma unroll
                for (int e = 0; e < NX; e++) tile[ftile_at(MEQN + e, r, c)] = a.aux[xplane(e) + ga];
            }
        }
    }
    // no workgroup barrier here: a wavefront sweeps exactly the four rows it loaded (the LDS operations of one
    // wavefront stay in order; the fence keeps the compiler from moving the reads of other lanes' writes up)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    double cflx = 0.0, cfly = 0.0;
    bool quiet = true;                                // wave-uniform: every sweep of this wavefront took the shortcut

    // ---- x sweeps of the tile's rows (step2ds.f:83-146) --------------------------------------------------------
    {
        const int cl = lane & (F_COLS - 1);           // (F_RX rows per wavefront where the tile is narrower than it)
        const int ca = x0 + cl;
        const bool owned = (ca >= a.mbc) && (ca < a.mbc + a.mx) && cl >= HALO && cl < F_COLS - HALO;
        const bool cfl_ok = (ca >= a.mbc) && (ca <= a.mbc + a.mx) && cl >= 1;
        // Row reuse: lane_core of an x sweep is a function of the row's q, a.dtd, the column masks owned /
        // cfl_ok and a -- with F_RX == 1 nothing in it depends on the row -- so a row that holds, in all 64 columns of the
        // window and all components, the same BITS as the row this wavefront swept before it (64-bit integer compares: -0
        // is not +0, equal NaN bits are equal) gets the same bits back.  Bit k of `same`: sweep k repeats sweep k - 1
        // (wave-uniform; the chain runs through reused rows too).  Taken here, in front of the first sweep, while every row
        // still holds its input; the rows the loop skips trail in the order and take no bit.  The wavefront leaves the
        // number of sweeps it reuses right away (one byte; wavefront 0 the launch's number), so nothing outlives the pass.
        unsigned same = 0;
        if constexpr (NX == 0) {
            static_assert(F_RX == 1, "row reuse: one row per sweep, the column masks are the same for every row");
            if (rowreuse) {                           // kernel argument: uniform
                long long p[MEQN];
#pragma unroll
                for (int m = 0; m < MEQN; m++) p[m] = __double_as_longlong(tile[ftile_at(m, wave_row(wv, 0), cl)]);
#pragma unroll
                for (int k = 1; k < F_NS; k++) {
                    bool eq = true;
#pragma unroll
                    for (int m = 0; m < MEQN; m++) {
                        const long long v = __double_as_longlong(tile[ftile_at(m, wave_row(wv, k), cl)]);
                        eq = eq & (v == p[m]);
                        p[m] = v;
                    }
                    if (__all(eq) && y0 + wave_row(wv, k) < a.J) same |= 1u << k;
                }
                if (tq_reuse && lane == 0) {
                    reinterpret_cast<unsigned char *>(tq_reuse + 2 * tile_id + 1)[wv] = (unsigned char)__popc(same);
                    if (wv == 0) tq_reuse[2 * tile_id] = ring_seq;
                }
            }
        }
        NoJumpMemo<MEQN> memo;
        bool nojump = false;                          // of the sweep before (wave-uniform)
#pragma unroll 1
        for (int k = 0; k < F_NS; k++) {
            const int r0 = wave_row(wv, k), r = r0 + lane / F_COLS;
            if (y0 + r0 >= a.J) continue;             // wave-uniform
            if (NX == 0 && ((same >> k) & 1u)) {
                // the row before again: its shortcut, or its result from its LDS row (this lane wrote that cell itself;
                // halo columns keep their input, as behind a computed sweep).  cflx holds these speeds already.
                quiet = quiet && nojump;
                if (owned && !nojump) {
                    const int rp = wave_row(wv, k - 1);
#pragma unroll
                    for (int m = 0; m < MEQN; m++) tile[ftile_at(m, r, cl)] = tile[ftile_at(m, rp, cl)];
                }
                continue;
            }
            double q[MEQN], qn[MEQN];
#pragma unroll
            for (int m = 0; m < MEQN; m++) q[m] = tile[ftile_at(m, r, cl)];
            // nojump (wave-uniform): the cells go back as they came, nothing to put back
            if constexpr (NX > 0) {
                // dtdx1d(i) = dtdx / aux(mcapa,i,j) (step2ds.f:95-99) and the solver's aux values, as sweep_kernel's x pass
                double capa = 1.0, dtdx_c = a.dtd, auxv[NAUX > 0 ? NAUX : 1];
                if constexpr (CAPA) {
                    capa = tile[ftile_at(MEQN, r, cl)];
                    dtdx_c = a.dtd / capa;
                }
#pragma unroll
                for (int m = 0; m < NAUX; m++) auxv[m] = tile[ftile_at(PAUX + m, r, cl)];
                nojump = lane_core<RP, 1, CAPA, FWAVE, false>(q, dtdx_c, capa, cfl_ok && (F_RX == 1 || y0 + r < a.J), a, qn, cflx,
                                                              nullptr, nullptr, nullptr, NAUX > 0 ? auxv : nullptr);
            } else
                nojump = lane_core<RP, 1, false, FWAVE, false>(q, a.dtd, 1.0, cfl_ok && (F_RX == 1 || y0 + r < a.J), a, qn,
                                                               cflx, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                               nullptr, &memo);
            quiet = quiet && nojump;
            if (owned && !nojump) {
#pragma unroll
                for (int m = 0; m < MEQN; m++) tile[ftile_at(m, r, cl)] = qn[m];
            }
        }
    }
    __syncthreads();

    // ---- y sweeps of the tile's columns (step2ds.f:150-159), two columns per wavefront --------------------------
    {
        SweepArgs ay = a;
        ay.dtd = a.dtd_t;
        const int rl = lane & (F_ROWS - 1), h = lane / F_ROWS;
        const int gy = y0 + rl;
        const bool row_owned = (gy >= a.mbc) && (gy < a.mbc + a.my) && rl >= HALO && rl < F_ROWS - HALO;
        const bool row_cfl = (gy >= a.mbc) && (gy <= a.mbc + a.my) && rl >= 1;
        NoJumpMemo<MEQN> memo;
#pragma unroll 1
        for (int p = wv; p < F_COLS / F_CY; p += F_WAVES) {
            const int c = F_CY * p + h, gx = x0 + c;
            // columns that hold q*: the tile's own interior columns and every ghost column (copied through by the x
            // sweeps; step2ds sweeps them too and their wave speeds count for the Courant number)
            auto has_qstar = [&](int cc) {
                const int g = x0 + cc;
                return g < a.I && ((cc >= HALO && cc < F_COLS - HALO) || g < a.mbc || g >= a.mbc + a.mx);
            };
            bool any = false;
#pragma unroll
            for (int j = 0; j < F_CY; j++) any = any || has_qstar(F_CY * p + j);
            if (!any) continue;                                            // wave-uniform
            const bool col_ok = has_qstar(c);
            const bool col_int = c >= HALO && c < F_COLS - HALO && gx >= a.mbc && gx < a.mbc + a.mx;
            double q[MEQN], qn[MEQN];
#pragma unroll
            for (int m = 0; m < MEQN; m++) q[m] = tile[ftile_at(m, rl, c)];
            bool nojump, colcut = false;
            if constexpr (NX > 0) {
                // dtdy1d(j) = dtdy / aux(mcapa,i,j) (step2ds.f:179-183), as sweep_kernel's y pass
                double capa = 1.0, dtdy_c = ay.dtd, auxv[NAUX > 0 ? NAUX : 1];
                if constexpr (CAPA) {
                    capa = tile[ftile_at(MEQN, rl, c)];
                    dtdy_c = ay.dtd / capa;
                }
#pragma unroll
                for (int m = 0; m < NAUX; m++) auxv[m] = tile[ftile_at(PAUX + m, rl, c)];
                nojump = lane_core<RP, 2, CAPA, FWAVE, false>(q, dtdy_c, capa, row_cfl && col_ok, ay, qn, cfly, nullptr, nullptr,
                                                              nullptr, NAUX > 0 ? auxv : nullptr);
            } else {
                // Column shortcut: the four columns differ from each other and each is constant
                // over its 16 rows -- the inflow strip, a front planar in x.  Only the interfaces at rl == 0 carry a jump, and
                // those reach rows 15 and 0 alone, which are never stored: every stored cell keeps its bits, so each lane
                // takes the speeds of its own cell and nothing goes back.  Not a no-jump sweep for `quiet`: TQ_ALL means one
                // state in the whole window.
                nojump = lane_core<RP, 2, false, FWAVE, false, false, false, F_ROWS>(q, ay.dtd, 1.0, row_cfl && col_ok, ay, qn, cfly,
                                                                                     nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                                     nullptr, nullptr, &memo, ycol != 0,
                                                                                     row_owned && col_int, &colcut);
                memo.valid += colcut ? 2 : 0;         // the wavefront's count, above the memo's valid bit (classic.hpp)
            }
            quiet = quiet && nojump;
            if (row_owned && col_int && !nojump && !colcut) {
#pragma unroll
                for (int m = 0; m < MEQN; m++) tile[ftile_at(m, rl, c)] = qn[m];
            }
        }
        // the wavefront leaves its count (one byte; wavefront 0 the launch's number), as the row reuse does
        if (NX == 0 && tq_ycol && lane == 0) {
            reinterpret_cast<unsigned char *>(tq_ycol + 2 * tile_id + 1)[wv] = (unsigned char)(memo.valid >> 1);
            if (wv == 0) tq_ycol[2 * tile_id] = ring_seq;
        }
    }
    // A class-Q tile quiet again needs no store: the launch before left it quiet, so its owned cells in
    // qout (that launch's input) equal qin (that launch's output), and quiet now they are also this launch's result.
    // Not under the fused source, whose fixed-point test needs the stored cells.  Each wavefront leaves its quiet flag
    // in halo row 0 of column F_CY * wv: only this wavefront's y sweep reads that cell, and the store does not.
    if (!SRC && class_q && lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        tile[ftile_at(0, 0, F_CY * wv)] = quiet ? 1.0 : 0.0;
    }
    __syncthreads();
    bool keep_store = true;
    if (!SRC && class_q) {
        keep_store = false;
#pragma unroll
        for (int w = 0; w < F_WAVES; w++) keep_store = keep_store || tile[ftile_at(0, 0, F_CY * w)] == 0.0;
    }

    // ---- store: the tile's own interior cells --------------------------------------------------------------------
    const bool all_interior = full_tile && x0 + HALO >= a.mbc && x0 + HALO + F_OWN_C <= a.mbc + a.mx && y0 + HALO >= a.mbc &&
                              y0 + HALO + F_OWN_R <= a.mbc + a.my;
    bool src_fixed = true;                            // every cell this lane stored is a fixed point of the source
    if (!keep_store) {
        // qout holds this launch's result already
    } else if (all_interior) {
        constexpr int PAIRS = F_OWN_C / 2, SLOTS = PAIRS * F_OWN_R;
#pragma unroll
        for (int k = 0; k < (SLOTS + F_THREADS - 1) / F_THREADS; k++) {
            const int slot = threadIdx.x + F_THREADS * k;
            if (slot < SLOTS) {
                const int r = HALO + slot / PAIRS, c = HALO + 2 * (slot % PAIRS);
                const long g = (long)(y0 + r) * a.pitch + (x0 + c);
                double2 v[MEQN];
#pragma unroll
                for (int m = 0; m < MEQN; m++) {
                    v[m] = *reinterpret_cast<const double2 *>(&tile[(m * F_ROWS + r) * F_COLS + ((c ^ fswz(r)) & ~1)]);
                    if (fswz(r) & 1) { const double t = v[m].x; v[m].x = v[m].y; v[m].y = t; }
                }
                if constexpr (SRC) {
                    const double2 rad = *reinterpret_cast<const double2 *>(&a.aux[g]);
                    src_fixed = src_fixed && euler_radial_source_fixed(v[0].x, v[1].x, v[2].x, v[3].x, rad.x) &&
                                euler_radial_source_fixed(v[0].y, v[1].y, v[2].y, v[3].y, rad.y);
                    euler_radial_source(v[0].x, v[1].x, v[2].x, v[3].x, rad.x, a.dt, a.src_p[0], a.src_p[1]);
                    euler_radial_source(v[0].y, v[1].y, v[2].y, v[3].y, rad.y, a.dt, a.src_p[0], a.src_p[1]);
                }
#pragma unroll
                for (int m = 0; m < MEQN; m++) st_stream2(&a.qout[m * a.plane + g], v[m]);
            }
        }
    } else {
#pragma unroll 1
        for (int slot = threadIdx.x; slot < F_OWN_R * F_OWN_C; slot += F_THREADS) {
            const int r = HALO + slot / F_OWN_C, c = HALO + slot % F_OWN_C;
            const int gx = x0 + c, gy = y0 + r;
            if (gx >= a.mbc && gx < a.mbc + a.mx && gy >= a.mbc && gy < a.mbc + a.my) {
                const long g = (long)gy * a.pitch + gx;
                double v[MEQN];
#pragma unroll
                for (int m = 0; m < MEQN; m++) v[m] = tile[ftile_at(m, r, c)];
                if constexpr (SRC) {
                    src_fixed = src_fixed && euler_radial_source_fixed(v[0], v[1], v[2], v[3], a.aux[g]);
                    euler_radial_source(v[0], v[1], v[2], v[3], a.aux[g], a.dt, a.src_p[0], a.src_p[1]);
                }
#pragma unroll
                for (int m = 0; m < MEQN; m++) a.qout[m * a.plane + g] = v[m];
            }
        }
    }
    if (tq_out) {
        // this wavefront's quiet byte and, where it is quiet, its two Courant maxima before dt/d (read back by the
        // tile's skipped launches)
        if constexpr (SRC) quiet = quiet && __all(src_fixed);
        if (quiet) {
            double cx = cflx, cy = cfly;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                cx = dmax(cx, __shfl_xor(cx, off, WAVE));
                cy = dmax(cy, __shfl_xor(cy, off, WAVE));
            }
            if (lane == 0) tq_cfl[tile_id * F_WAVES + wv] = make_double2(cx, cy);
        }
        if (lane == 0) reinterpret_cast<unsigned char *>(tq_out + tile_id)[wv] = quiet ? TQ_QUIET : 0u;
    }
    // the two passes have their own dt/d: the larger Courant number of the two is the step's (step2ds.f:136,181)
    cfl_publish(a.cfl, dmax(cfl_value<CAPA>(cflx, a.dtd), cfl_value<CAPA>(cfly, a.dtd_t)));
}

}  // namespace PCL_NS
}  // namespace pcl
