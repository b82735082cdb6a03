// classic3.hpp -- the UNSPLIT 3-D classic algorithm (step3.f + the transverse part of flux3.f) as gfx950 kernels.
//
// Reference path restated (operation order preserved; oracle: oracle/classic_oracle.c flux3_full / orc_step3):
//   flux3.f:168-258   normal solve, Godunov increment, CFL, limiter, cqxx / fadd        (as the dim-split sweep)
//   flux3.f:260-593   rpt3 x4 (+4 for the correction waves), rptt3 x8, gadd / hadd accumulation
//   step3.f:114-592   x, y, z sweeps over slices 0..m+1; every slice updates the 3 x 3 cells around it
//
// One kernel per direction (march3p_kernel, below).  Each lane computes the pieces one slice leaves for the 3 x 3 cells
// around it -- qadd, fadd(i+1)-fadd(i), gadd(2,-1:1), hadd(2,-1:1) -- in registers, and every interior cell receives the
// nine slices around it IN THE ORDER the Fortran's loop nest visits them (x and z sweeps: z-like index outer, y-like
// inner; y sweep: y-like outer), with the reference's association.  All three directions read the same qold, and the
// x, y, z contributions are added in that order, exactly like step3.f.  The kernel exists for the solvers whose
// transverse splits are driven by one component (RP::T3_PRESSURE, the variable-coefficient acoustics); the launcher
// refuses every other solver.
//
// Direction roles (step3.f:176,303,470): sweep DIR, y-like = DIR+1, z-like = DIR+2 (cyclic).  aux block of a cell:
// blk[oe+1][of+1][k] = aux component k of the neighbour at y-like offset oe, z-like offset of.
#pragma once
#include "classic.hpp"

namespace pcl {
namespace PCL_NS {

struct Slices3Args {
    long s_e, s_f;       // strides (doubles) of the y-like and z-like directions
    int n_e, n_f;        // extents with ghost cells
    int lo_e, hi_e, lo_f, hi_f;   // swept slices: 0..m+1 in both transverse directions (ghost-offset indices)
    int m3, m4;          // method(3) = 10*m3 + m4
    double dty, dtz;     // dt / d(y-like), dt / d(z-like)
};

template <class RP, int DIR>
__device__ __forceinline__ void load_blk(const SweepArgs &a, const Slices3Args &t, long g, int ce, int cf,
                                         double (&blk)[3][3][RP::NAUX]) {
#pragma unroll
    for (int oe = -1; oe <= 1; oe++)
#pragma unroll
        for (int of = -1; of <= 1; of++) {
            // clamp: the outermost slices' far neighbours do not exist; their results are never used (step3.f sweeps
            // 0..m+1 with mbc = 2, so every USED block lies inside the array)
            const int de = (ce + oe < 0) ? 0 : (ce + oe >= t.n_e ? 0 : oe);
            const int df = (cf + of < 0) ? 0 : (cf + of >= t.n_f ? 0 : of);
#pragma unroll
            for (int k = 0; k < RP::NAUX; k++)
                blk[oe + 1][of + 1][k] = a.aux[aux_idx<RP, DIR>(k) * a.plane + g + de * t.s_e + df * t.s_f];
        }
}

// ---- the pieces of one slice (flux3.f:168-593) for solvers whose transverse splits are driven by ONE component -------
// (RP::T3_PRESSURE: acoustics.)  rpt3 / rptt3_vc_acoustics read asdq(1) and asdq(iuvw+1) (oracle/classic_oracle.c), and
// what they are handed never has the second one: the normal fluctuations carry (p, sweep velocity), a y-like split
// returns (p, y-like velocity), a z-like split (p, z-like velocity).  So all 16 solves per interface reduce to
//     a1 = -t0 / (Zm + Z),  a2 = t0 / (Z + Zp)      outputs  (cm a1 Zm, -cm a1)  and  (cp a2 Zp, cp a2),
// the G terms live in components (p, y-like velocity), the H terms in (p, z-like velocity), qadd / fadd in
// (p, sweep velocity).  This form keeps only those: 24 doubles of gadd / hadd instead of 48, half the work after the
// normal solve, half the exchange.  Every operation that remains is the general form's (every component of every
// split, as flux3.f and oracle/classic_oracle.c compute them), in its order; the ones dropped
// have a structural zero as operand, so the values agree except, possibly, in the SIGN of a zero (v + 0.0 for
// v = -0.0; -t0 + 0.0*Z for t0 = 0) -- the difference DESIGN section 4.1 already accepts for dmax1/dmin1.
struct P2 { double p, v; };
// M34: method(3) = 10*m3 + m4 as a compile-time constant (22: the solver default, every term present, no run-time
// selects), or -1 = read at run time
template <class RP, int DIR, int M34 = -1>
__device__ __forceinline__ void slice3_pieces_p(const double (&q)[RP::MEQN], const double (&auxv)[RP::NAUX],
                                                const double (&blkR)[3][3][RP::NAUX], const SweepArgs &a, const Slices3Args &t,
                                                bool cfl_ok, double &cflmax, P2 &qadd, P2 &df, P2 (&G)[2][3], P2 (&H)[2][3]) {
    constexpr int MEQN = RP::MEQN, MWAVES = RP::MWAVES, NAUX = RP::NAUX;
    using Cell = typename RP::Cell;
    const int m3 = M34 >= 0 ? M34 / 10 : t.m3, m4 = M34 >= 0 ? M34 % 10 : t.m4;
    static_assert(NAUX == 2, "aux = (impedance, sound speed)");
    const double d = a.dtd;
    const Cell cR = RP::template precell<DIR>(q, a.par, auxv);
    const Cell cL = struct_from_left(cR);
    double wave[MWAVES][MEQN], s[MWAVES], amdq[MEQN], apdq[MEQN];
    RP::template solve<DIR>(cL, cR, a.par, wave, s, amdq, apdq);
    cfl_accumulate<false, MWAVES>(s, d, d, cfl_ok, cflmax);
    double cq[MEQN];
#pragma unroll
    for (int m = 0; m < MEQN; m++) cq[m] = 0.0;
    if (a.order != 1) {
#pragma unroll
        for (int mw = 0; mw < MWAVES; mw++) {
            const int lim = a.mthlim[mw];
            if (lim == 0) continue;
            double wn = 0.0, dl = 0.0;
            bool first = true;
#pragma unroll
            for (int m = 0; m < MEQN; m++) {
                if (!RP::template nz<DIR>(mw, m)) continue;
                const double w = wave[mw][m], wl = from_left(w);
                wn = first ? w * w : wn + w * w;
                dl = first ? wl * w : dl + wl * w;
                first = false;
            }
            const double dr = from_right(dl);
            if (wn != 0.0) {
                const double phi = philim(wn, s[mw] > 0.0 ? dl : dr, lim);
#pragma unroll
                for (int m = 0; m < MEQN; m++)
                    if (RP::template nz<DIR>(mw, m)) wave[mw][m] = phi * wave[mw][m];
            }
        }
        const double dtdxave = 0.5 * (d + d);
#pragma unroll
        for (int m = 0; m < MEQN; m++) {
            if (!(m == 0 || m == DIR)) continue;
            double c = 0.0;
            bool first = true;
#pragma unroll
            for (int mw = 0; mw < MWAVES; mw++)
                if (RP::template nz<DIR>(mw, m)) {
                    const double sa = fabs(s[mw]);
                    const double term = 0.5 * sa * (1.0 - sa * dtdxave) * wave[mw][m];
                    c = first ? term : c + term;
                    first = false;
                }
            cq[m] = c;
        }
    }
    qadd.p = -(d * apdq[0]) - d * from_right(amdq[0]);
    qadd.v = -(d * apdq[DIR]) - d * from_right(amdq[DIR]);
    df.p = from_right(cq[0]) - cq[0];
    df.v = from_right(cq[DIR]) - cq[DIR];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) { G[k][j].p = 0.0; G[k][j].v = 0.0; H[k][j].p = 0.0; H[k][j].v = 0.0; }
    if (m3 <= 0) return;

    // Every split below uses THIS cell's block: A^+ dq and the correction flux of interface l belong to cell l, and
    // A^- dq / the correction flux of interface l+1 -- which the general form splits in lane l+1 with the left
    // neighbour's block and then shifts back -- are fetched from the right-hand lane first and split here.  Same
    // operands, same operations, one lane to the left: the left neighbour's block, its reciprocals and 32 shifts of
    // results disappear, and the twelve impedance sums of the block are inverted once.
    const double aP = apdq[0], aM = from_right(amdq[0]);
    const double kP = cq[0], kM = from_right(cq[0]);
    Recip ry[3][2], rz[3][2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ry[r][0] = Recip(blkR[0][r][0] + blkR[1][r][0]); ry[r][1] = Recip(blkR[1][r][0] + blkR[2][r][0]);
        rz[r][0] = Recip(blkR[r][0][0] + blkR[r][1][0]); rz[r][1] = Recip(blkR[r][1][0] + blkR[r][2][0]);
    }
    // one split: the line (Zm, Z, Zp; cm, cp) of the block along the y-like (yl) or z-like direction at the other
    // direction's offset r-1, driven by the pressure part t0: minus-going and plus-going result
    auto split = [&](bool yl, int r, double t0, P2 &om, P2 &op) {
        double zm = 0.0, zp = 0.0, cm = 0.0, cp = 0.0;
        Recip by_m, by_p;
#pragma unroll
        for (int x = 0; x < 3; x++) {       // static indices only (r is a constant after inlining)
            if (x == r) {
                zm = yl ? blkR[0][x][0] : blkR[x][0][0]; zp = yl ? blkR[2][x][0] : blkR[x][2][0];
                cm = yl ? blkR[0][x][1] : blkR[x][0][1]; cp = yl ? blkR[2][x][1] : blkR[x][2][1];
                by_m = yl ? ry[x][0] : rz[x][0]; by_p = yl ? ry[x][1] : rz[x][1];
            }
        }
        const double a1 = by_m.div(-t0);
        const double a2 = by_p.div(t0);
        om.p = cm * a1 * zm; om.v = -cm * a1;
        op.p = cp * a2 * zp; op.v = cp * a2;
    };
    const P2 zero{0.0, 0.0};
    // names as in flux3.f; the ...amdq / ...cqxxm ones are those of interface l+1 (the general form's r_ values)
    P2 bmamdq, bpamdq, bmapdq, bpapdq, cmamdq, cpamdq, cmapdq, cpapdq;
    split(true, 1, aM, bmamdq, bpamdq);
    split(true, 1, aP, bmapdq, bpapdq);
    split(false, 1, aM, cmamdq, cpamdq);
    split(false, 1, aP, cmapdq, cpapdq);
    P2 bmcqxxm = zero, bpcqxxm = zero, bmcqxxp = zero, bpcqxxp = zero, cmcqxxm = zero, cpcqxxm = zero, cmcqxxp = zero, cpcqxxp = zero;
    if (m3 == 2) {
        split(true, 1, kM, bmcqxxm, bpcqxxm);
        split(true, 1, kP, bmcqxxp, bpcqxxp);
        split(false, 1, kM, cmcqxxm, cpcqxxm);
        split(false, 1, kP, cmcqxxp, cpcqxxp);
    }
    const double k6z = (1.0 / 6.0) * d * t.dtz, k6y = (1.0 / 6.0) * d * t.dty;
    // one component of the six G (or H) values of this cell: the general form's statements in their order.
    // b?a?dq: first-level split in the flux's own direction; x???: second-level results; q???: correction-wave splits
    auto six = [&](double k6, double bmap, double bpap, double bmam, double bpam, double xmcpap, double xpcpap, double xmcmap,
                   double xpcmap, double xmcpam, double xpcpam, double xmcmam, double xpcmam, double qmp, double qpp, double qmm,
                   double qpm, double &o10, double &o20, double &o21, double &o11, double &o2m, double &o1m) {
        double g10 = 0.0, g20 = 0.0, g21 = 0.0, g11 = 0.0, g2m = 0.0, g1m = 0.0;
        g10 = g10 - 0.5 * d * bmap;
        g20 = g20 - 0.5 * d * bpap;
        if (m4 > 0) {
            g20 = g20 + k6 * (xpcpap - xpcmap);
            g10 = g10 + k6 * (xmcpap - xmcmap);
            g21 = g21 - k6 * xpcpap;
            g11 = g11 - k6 * xmcpap;
            g2m = g2m + k6 * xpcmap;
            g1m = g1m + k6 * xmcmap;
        }
        if (m3 >= 2) {
            g20 = g20 + d * qpp;
            g10 = g10 + d * qmp;
        }
        g10 = g10 - 0.5 * d * bmam;                 // interface l+1
        g20 = g20 - 0.5 * d * bpam;
        if (m4 > 0) {
            g20 = g20 + k6 * (xpcpam - xpcmam);
            g10 = g10 + k6 * (xmcpam - xmcmam);
            g21 = g21 - k6 * xpcpam;
            g11 = g11 - k6 * xmcpam;
            g2m = g2m + k6 * xpcmam;
            g1m = g1m + k6 * xmcmam;
        }
        if (m3 >= 2) {
            g20 = g20 - d * qpm;
            g10 = g10 - d * qmm;
        }
        o10 = g10; o20 = g20; o21 = g21; o11 = g11; o2m = g2m; o1m = g1m;
    };
    {   // ---- G fluxes (y-like), flux3.f:347-452: the z-like splits (corrected by the correction waves' for m4 = 2)
        // split again in the y-like direction, inside the z-like row they went to
        P2 bmcpapdq = zero, bpcpapdq = zero, bmcpamdq = zero, bpcpamdq = zero, bmcmapdq = zero, bpcmapdq = zero, bmcmamdq = zero, bpcmamdq = zero;
        if (m4 > 0) {
            const double cpapdq2 = m4 == 2 ? cpapdq.p - 3.0 * cpcqxxp.p : cpapdq.p;
            const double cpamdq2 = m4 == 2 ? cpamdq.p + 3.0 * cpcqxxm.p : cpamdq.p;
            const double cmapdq2 = m4 == 2 ? cmapdq.p - 3.0 * cmcqxxp.p : cmapdq.p;
            const double cmamdq2 = m4 == 2 ? cmamdq.p + 3.0 * cmcqxxm.p : cmamdq.p;
            split(true, 2, cpapdq2, bmcpapdq, bpcpapdq);
            split(true, 2, cpamdq2, bmcpamdq, bpcpamdq);
            split(true, 0, cmapdq2, bmcmapdq, bpcmapdq);
            split(true, 0, cmamdq2, bmcmamdq, bpcmamdq);
        }
        six(k6z, bmapdq.p, bpapdq.p, bmamdq.p, bpamdq.p, bmcpapdq.p, bpcpapdq.p, bmcmapdq.p, bpcmapdq.p, bmcpamdq.p, bpcpamdq.p,
            bmcmamdq.p, bpcmamdq.p, bmcqxxp.p, bpcqxxp.p, bmcqxxm.p, bpcqxxm.p,
            G[0][1].p, G[1][1].p, G[1][2].p, G[0][2].p, G[1][0].p, G[0][0].p);
        six(k6z, bmapdq.v, bpapdq.v, bmamdq.v, bpamdq.v, bmcpapdq.v, bpcpapdq.v, bmcmapdq.v, bpcmapdq.v, bmcpamdq.v, bpcpamdq.v,
            bmcmamdq.v, bpcmamdq.v, bmcqxxp.v, bpcqxxp.v, bmcqxxm.v, bpcqxxm.v,
            G[0][1].v, G[1][1].v, G[1][2].v, G[0][2].v, G[1][0].v, G[0][0].v);
    }
    {   // ---- H fluxes (z-like), flux3.f:462-590: the y-like splits (corrected for m4 = 2) split again in the z-like direction
        P2 ymcpapdq = zero, ypcpapdq = zero, ymcpamdq = zero, ypcpamdq = zero, ymcmapdq = zero, ypcmapdq = zero, ymcmamdq = zero, ypcmamdq = zero;
        if (m4 > 0) {
            const double bpapdq2 = m4 == 2 ? bpapdq.p - 3.0 * bpcqxxp.p : bpapdq.p;
            const double bpamdq2 = m4 == 2 ? bpamdq.p + 3.0 * bpcqxxm.p : bpamdq.p;
            const double bmapdq2 = m4 == 2 ? bmapdq.p - 3.0 * bmcqxxp.p : bmapdq.p;
            const double bmamdq2 = m4 == 2 ? bmamdq.p + 3.0 * bmcqxxm.p : bmamdq.p;
            split(false, 2, bpapdq2, ymcpapdq, ypcpapdq);
            split(false, 2, bpamdq2, ymcpamdq, ypcpamdq);
            split(false, 0, bmapdq2, ymcmapdq, ypcmapdq);
            split(false, 0, bmamdq2, ymcmamdq, ypcmamdq);
        }
        six(k6y, cmapdq.p, cpapdq.p, cmamdq.p, cpamdq.p, ymcpapdq.p, ypcpapdq.p, ymcmapdq.p, ypcmapdq.p, ymcpamdq.p, ypcpamdq.p,
            ymcmamdq.p, ypcmamdq.p, cmcqxxp.p, cpcqxxp.p, cmcqxxm.p, cpcqxxm.p,
            H[0][1].p, H[1][1].p, H[1][2].p, H[0][2].p, H[1][0].p, H[0][0].p);
        six(k6y, cmapdq.v, cpapdq.v, cmamdq.v, cpamdq.v, ymcpapdq.v, ypcpapdq.v, ymcmapdq.v, ypcmapdq.v, ymcpamdq.v, ypcpamdq.v,
            ymcmamdq.v, ypcmamdq.v, cmcqxxp.v, cpcqxxp.v, cmcqxxm.v, cpcqxxm.v,
            H[0][1].v, H[1][1].v, H[1][2].v, H[0][2].v, H[1][0].v, H[0][0].v);
    }
}

// ---- the marching kernel ------------------------------------------------------------------------------------------
// step3.f visits the slices of a direction in a loop nest -- x and z sweeps: z-like index outside, y-like inside; y sweep:
// y-like outside (step3.f:176,303,470) -- and every slice adds to the 3 x 3 cells around it, so a cell receives its nine
// contributions ordered by the OUTER index of the source slice first, the inner one second.  march3p_kernel walks the
// outer index ("march axis" M): a workgroup of NW wavefronts holds NW consecutive slices of the inner index ("wave
// axis" W) of one 64-cell strip, and at march step m every wavefront computes the pieces of its slice (w, m)
// (slice3_pieces_p).  A target cell (w, tm) then gets, in the reference's order,
//     from plane m = tm-1:  slices w-1, w, w+1      (first: the accumulator starts from the cell's old value)
//     from plane m = tm  :  slices w-1, w, w+1
//     from plane m = tm+1:  slices w-1, w, w+1      (last: the cell is complete and is stored)
// i.e. three accumulators per wavefront live in registers across march steps (planes m+1, m, m-1) and only the
// contributions to the neighbouring slices w-1 / w+1 cross wavefronts, through LDS (every update is q = (q + A) + B
// with A the y-like and B the z-like flux term, products and signs applied by the SOURCE lane -- the operations of
// step3.f's update, so the bits are the same).  Tiles overlap by two slices along W (NW/(NW-2)
// recompute) and the march range is cut into segments (one extra source plane at each end) so that a 256^3 grid
// still gives every CU a workgroup.
//     DIR 1: M = z-like (k), W = y-like (j)     DIR 2: M = y-like (k), W = z-like (i)     DIR 3: M = z-like (j), W = y-like (i)
// For the y and z sweeps the wave axis is i: the 8 wavefronts of a workgroup touch 8 neighbouring doubles of every
// line and workgroups that are neighbours along i run on the same XCD (xcd_logical_block).
struct March3Args {
    const double *qsrc;   // what a cell's accumulator starts from: qold (x direction), the state accumulated so far (y, z)
    double *qacc;
    long s_w, s_m;        // strides (doubles) of the wave axis / march axis
    int n_w, n_m, m_w, m_m;   // extents with ghost cells / interior extents
    int seg;              // target planes per workgroup along the march axis
    int ntiles_al, ntiles_w;
};

// the ordered pair of addends slice S gives the cell at (y-like offset oe, z-like offset of) from itself (step3.f's
// update formulas; G_(k,j) = G[k-1][j+1], H_(k,j) = H[k-1][j+1]): q := (q + A) + B, A from G (components p, y-like
// velocity), B from H (components p, z-like velocity).  The centre cell (0,0) has two more addends in front (qadd,
// -dtd*df), applied by the caller.
__device__ __forceinline__ void pair3p(int oe, int of, double dty, double dtz, const P2 (&G)[2][3], const P2 (&H)[2][3],
                                       P2 &A, P2 &B) {
#define G_(k, j, c) G[(k)-1][(j) + 1].c
#define H_(k, j, c) H[(k)-1][(j) + 1].c
#define PAIR_(EA, EB) { A.p = EA(p); A.v = EA(v); B.p = EB(p); B.v = EB(v); }
#define A00(c) -(dty * (G_(2, 0, c) - G_(1, 0, c)))
#define B00(c) -(dtz * (H_(2, 0, c) - H_(1, 0, c)))
#define AM0(c) -(dty * G_(1, 0, c))
#define BM0(c) -(dtz * (H_(2, -1, c) - H_(1, -1, c)))
#define AMM(c) -(dty * G_(1, -1, c))
#define BMM(c) -(dtz * H_(1, -1, c))
#define A0M(c) -(dty * (G_(2, -1, c) - G_(1, -1, c)))
#define B0M(c) -(dtz * H_(1, 0, c))
#define APM(c) (dty * G_(2, -1, c))
#define BPM(c) -(dtz * H_(1, 1, c))
#define AP0(c) (dty * G_(2, 0, c))
#define BP0(c) -(dtz * (H_(2, 1, c) - H_(1, 1, c)))
#define APP(c) (dty * G_(2, 1, c))
#define BPP(c) (dtz * H_(2, 1, c))
#define A0P(c) -(dty * (G_(2, 1, c) - G_(1, 1, c)))
#define B0P(c) (dtz * H_(2, 0, c))
#define AMP(c) -(dty * G_(1, 1, c))
#define BMP(c) (dtz * H_(2, -1, c))
    if (oe == 0 && of == 0) PAIR_(A00, B00)
    else if (oe == -1 && of == 0) PAIR_(AM0, BM0)
    else if (oe == -1 && of == -1) PAIR_(AMM, BMM)
    else if (oe == 0 && of == -1) PAIR_(A0M, B0M)
    else if (oe == 1 && of == -1) PAIR_(APM, BPM)
    else if (oe == 1 && of == 0) PAIR_(AP0, BP0)
    else if (oe == 1 && of == 1) PAIR_(APP, BPP)
    else if (oe == 0 && of == 1) PAIR_(A0P, B0P)
    else PAIR_(AMP, BMP)
#undef G_
#undef H_
#undef PAIR_
#undef A00
#undef B00
#undef AM0
#undef BM0
#undef AMM
#undef BMM
#undef A0M
#undef B0M
#undef APM
#undef BPM
#undef AP0
#undef BP0
#undef APP
#undef BPP
#undef A0P
#undef B0P
#undef AMP
#undef BMP
}

// The marching kernel (above) for the pressure-driven pieces: component 0 receives both addends of every contribution,
// the y-like velocity only A, the z-like velocity only B, the sweep velocity only the slice's own qadd / fadd -- 24
// doubles per lane cross wavefronts instead of 48, in ONE exchange phase (two barriers per march step).
template <class RP, int DIR, int NW, int M34 = -1>
__global__ __launch_bounds__(NW *WAVE) void march3p_kernel(SweepArgs a, Slices3Args t, March3Args g) {
    constexpr int MEQN = RP::MEQN, NAUX = RP::NAUX;
    static_assert(MEQN == 4 && RP::T3_PRESSURE, "q = (p, u, v, w)");
    constexpr bool E_OUTER = DIR == 2;
    constexpr int IE = DIR % 3 + 1, IF = (DIR + 1) % 3 + 1;      // components of the y-like / z-like velocity
    // xbuf[w][side][o][A.p | B.p | A.v | B.v][lane]: side 0 = for the slice w+1, 1 = for the slice w-1; o = M offset + 1
    __shared__ double xbuf[NW][2][3][4][WAVE];
    // y and z sweeps: the lanes of a wavefront are `pitch` doubles apart in memory, 64 lines per load / store
    // instruction, and with ~18 of them per step the texture addresser -- not the VALU -- set the pace (x direction
    // 1.14 ms, y / z 1.49 ms at 256^3).  Their wave axis is i, the contiguous one: the workgroup loads and stores
    // 64-row x NW-column tiles cooperatively (8 doubles = 64 B per row segment, 8 segments per instruction instead of
    // 64 lines) and transposes them through LDS.  STAGED tiles: the next plane's cell values (tq1), the accumulated
    // state two planes ahead (tq2: what that plane's accumulator starts from), the aux face two planes ahead (ta,
    // NW + 2 columns), and -- in xbuf's memory, free between two exchanges -- the finished plane on its way out.
    constexpr bool STAGED = DIR != 1;
    constexpr int TP = NW + 1, TAP = NW + 3;
    __shared__ double tq1[STAGED ? MEQN : 1][STAGED ? WAVE : 1][STAGED ? TP : 1];
    __shared__ double tq2[STAGED ? MEQN : 1][STAGED ? WAVE : 1][STAGED ? TP : 1];
    __shared__ double tau[STAGED ? NAUX : 1][STAGED ? WAVE : 1][STAGED ? TAP : 1];
    static_assert(!STAGED || MEQN * WAVE * TP <= NW * 2 * 3 * 4 * WAVE, "the outgoing tile lives in xbuf");
    double(*tout)[WAVE][TP] = reinterpret_cast<double(*)[WAVE][TP]>(&xbuf[0][0][0][0][0]);
    constexpr int NT = NW * WAVE;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int bid = DIR == 1 ? (int)blockIdx.x : xcd_logical_block();
    const int tw = bid % g.ntiles_w, ta = (bid / g.ntiles_w) % g.ntiles_al, ts = bid / (g.ntiles_w * g.ntiles_al);
    const int a0 = a.mbc - HALO + ta * STRIP;
    const int ca = a0 + lane;
    const int cc = ca < a.n_al ? ca : a.n_al - 1;
    const int cw0 = a.mbc - 1 + tw * (NW - 2);
    const int cw = cw0 + w;
    const bool w_live = cw <= a.mbc + g.m_w;                           // wave-uniform
    const int cwc = cw < g.n_w ? cw : g.n_w - 1;
    const bool target_w = w >= 1 && w <= NW - 2 && cw >= a.mbc && cw < a.mbc + g.m_w;
    const bool owned = (ca >= a.mbc) && (ca < a.mbc + a.m_al) && lane >= HALO && lane < WAVE - HALO && target_w;
    const bool cfl_ok = (ca >= a.mbc) && (ca <= a.mbc + a.m_al) && lane >= 1;
    const int tm0 = a.mbc + ts * g.seg;
    const int tm1 = tm0 + g.seg < a.mbc + g.m_m ? tm0 + g.seg : a.mbc + g.m_m;
    const long base = (long)cc * a.s_al + (long)cwc * g.s_w;
    const int wl = w > 0 ? w - 1 : w, wr = w < NW - 1 ? w + 1 : w;
    // this thread's cell of the cooperative tiles: row tr along the sweep, column tc along the wave axis
    const int tc = threadIdx.x % NW, tr = threadIdx.x / NW;
    const int trow = a0 + tr < a.n_al ? a0 + tr : a.n_al - 1;
    const int tcol = cw0 + tc < g.n_w ? cw0 + tc : g.n_w - 1;
    const long tbase = (long)trow * a.s_al + (long)tcol * g.s_w;
    const bool t_owned = (a0 + tr >= a.mbc) && (a0 + tr < a.mbc + a.m_al) && tr >= HALO && tr < WAVE - HALO && tc >= 1 &&
                         tc <= NW - 2 && cw0 + tc >= a.mbc && cw0 + tc < a.mbc + g.m_w;
    double cflmax = 0.0;
    double accP[MEQN], acc0[MEQN], accM[MEQN], accN[MEQN];
#pragma unroll
    for (int m = 0; m < MEQN; m++) { accP[m] = 0.0; acc0[m] = 0.0; accM[m] = 0.0; accN[m] = 0.0; }

    // The 3 x 3 aux block and the cell itself travel with the march: per step only the face ahead (three cells of the
    // wave axis at plane pm+2) and the next cell are needed -- 6 + 4 values instead of 18 + 2 + 4.
    double blkR[3][3][NAUX], qc[MEQN];
    {
        const long g0 = base + (long)(tm0 - 1) * g.s_m;
        load_blk<RP, DIR>(a, t, g0, E_OUTER ? tm0 - 1 : cwc, E_OUTER ? cwc : tm0 - 1, blkR);
#pragma unroll
        for (int m = 0; m < MEQN; m++) qc[m] = a.qin[m * a.plane + g0];
        if (STAGED && target_w) {      // the first target plane's starting value (later ones come through tq2)
#pragma unroll
            for (int m = 0; m < MEQN; m++) accN[m] = g.qsrc[m * a.plane + g0 + g.s_m];
        }
    }
    const long sw_lo = cwc > 0 ? -g.s_w : 0, sw_hi = cwc + 1 < g.n_w ? g.s_w : 0;      // wave-axis neighbours, clamped like load_blk
    for (int pm = tm0 - 1; pm <= tm1; pm++) {
        const long gc = base + (long)pm * g.s_m;
        // ---- loads for the NEXT step, in flight through this step's arithmetic
        double qn[MEQN], face[3][NAUX];
        double gq[MEQN], gs[MEQN], ga[2][NAUX];
        if constexpr (STAGED) {
            const long tg = tbase + (long)pm * g.s_m;
#pragma unroll
            for (int m = 0; m < MEQN; m++) gq[m] = a.qin[m * a.plane + tg + g.s_m];
            if (pm < tm1) {      // uniform
#pragma unroll
                for (int m = 0; m < MEQN; m++) gs[m] = g.qsrc[m * a.plane + tg + 2 * g.s_m];
#pragma unroll
                for (int k2 = 0; k2 < 2; k2++) {
                    const int id = threadIdx.x + k2 * NT;
                    const int ac_ = id % (NW + 2), ar_ = id / (NW + 2);
                    int col = cw0 - 1 + ac_;
                    col = col < 0 ? 0 : (col < g.n_w ? col : g.n_w - 1);
                    const int row = a0 + ar_ < a.n_al ? a0 + ar_ : a.n_al - 1;
#pragma unroll
                    for (int k = 0; k < NAUX; k++)
                        ga[k2][k] = ar_ < WAVE ? a.aux[aux_idx<RP, DIR>(k) * a.plane + (long)row * a.s_al + (long)col * g.s_w + (long)(pm + 2) * g.s_m] : 0.0;
                }
            } else {
#pragma unroll
                for (int m = 0; m < MEQN; m++) gs[m] = 0.0;
#pragma unroll
                for (int k2 = 0; k2 < 2; k2++)
#pragma unroll
                    for (int k = 0; k < NAUX; k++) ga[k2][k] = 0.0;
            }
            if (target_w) {
#pragma unroll
                for (int m = 0; m < MEQN; m++) accP[m] = accN[m];      // plane pm+1 starts from the accumulated state
            }
        } else {
#pragma unroll
            for (int m = 0; m < MEQN; m++) qn[m] = a.qin[m * a.plane + gc + g.s_m];
            if (pm < tm1) {      // uniform
#pragma unroll
                for (int k = 0; k < NAUX; k++) {
                    const long at = aux_idx<RP, DIR>(k) * a.plane + gc + 2 * g.s_m;
                    face[0][k] = a.aux[at + sw_lo]; face[1][k] = a.aux[at]; face[2][k] = a.aux[at + sw_hi];
                }
            } else {
#pragma unroll
                for (int k = 0; k < NAUX; k++) { face[0][k] = blkR[1][1][k]; face[1][k] = blkR[1][1][k]; face[2][k] = blkR[1][1][k]; }
            }
            if (target_w) {      // wave-uniform; x direction: the accumulator starts from qold = the next cell itself
#pragma unroll
                for (int m = 0; m < MEQN; m++) accP[m] = qn[m];
            }
        }
        P2 qadd{0.0, 0.0}, df{0.0, 0.0}, G[2][3], H[2][3];
        if (w_live) {
            double auxv[NAUX];
#pragma unroll
            for (int k = 0; k < NAUX; k++) auxv[k] = blkR[1][1][k];
            slice3_pieces_p<RP, DIR, M34>(qc, auxv, blkR, a, t, cfl_ok, cflmax, qadd, df, G, H);
        } else {
#pragma unroll
            for (int k = 0; k < 2; k++)
#pragma unroll
                for (int j = 0; j < 3; j++) { G[k][j].p = 0.0; G[k][j].v = 0.0; H[k][j].p = 0.0; H[k][j].v = 0.0; }
        }
#pragma unroll
        for (int side = 0; side < 2; side++)
#pragma unroll
            for (int o = -1; o <= 1; o++) {
                const int in = side == 0 ? 1 : -1;
                P2 A, B;
                pair3p(E_OUTER ? o : in, E_OUTER ? in : o, t.dty, t.dtz, G, H, A, B);
                xbuf[w][side][o + 1][0][lane] = A.p;
                xbuf[w][side][o + 1][1][lane] = B.p;
                xbuf[w][side][o + 1][2][lane] = A.v;
                xbuf[w][side][o + 1][3][lane] = B.v;
            }
        __syncthreads();
#pragma unroll
        for (int o = 1; o >= -1; o--) {
            double *acc = o == 1 ? accP : (o == 0 ? acc0 : accM);
            P2 A, B;
            pair3p(E_OUTER ? o : 0, E_OUTER ? 0 : o, t.dty, t.dtz, G, H, A, B);
            double vp = acc[0], ve = acc[IE], vf = acc[IF];
            vp = vp + xbuf[wl][0][o + 1][0][lane];                      // from the slice w-1
            vp = vp + xbuf[wl][0][o + 1][1][lane];
            ve = ve + xbuf[wl][0][o + 1][2][lane];
            vf = vf + xbuf[wl][0][o + 1][3][lane];
            if (o == 0) {
                vp = vp + qadd.p; vp = vp - a.dtd * df.p;
                acc[DIR] = (acc[DIR] + qadd.v) - a.dtd * df.v;
            }
            vp = vp + A.p; vp = vp + B.p;                               // this slice's own
            ve = ve + A.v;
            vf = vf + B.v;
            vp = vp + xbuf[wr][1][o + 1][0][lane];                      // from the slice w+1
            vp = vp + xbuf[wr][1][o + 1][1][lane];
            ve = ve + xbuf[wr][1][o + 1][2][lane];
            vf = vf + xbuf[wr][1][o + 1][3][lane];
            acc[0] = vp; acc[IE] = ve; acc[IF] = vf;
        }
        __syncthreads();
        const bool plane_out = pm - 1 >= tm0 && pm - 1 < tm1;           // the plane behind is complete (uniform)
        if constexpr (STAGED) {
            // transpose: the loaded tiles in, the finished plane out (tout shares xbuf's memory: every wavefront is past
            // the exchange)
#pragma unroll
            for (int m = 0; m < MEQN; m++) {
                tq1[m][tr][tc] = gq[m];
                tq2[m][tr][tc] = gs[m];
                tout[m][lane][w] = accM[m];
            }
#pragma unroll
            for (int k2 = 0; k2 < 2; k2++) {
                const int id = threadIdx.x + k2 * NT;
                const int ac_ = id % (NW + 2), ar_ = id / (NW + 2);
                if (ar_ < WAVE) {
#pragma unroll
                    for (int k = 0; k < NAUX; k++) tau[k][ar_][ac_] = ga[k2][k];
                }
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < MEQN; m++) { qn[m] = tq1[m][lane][w]; accN[m] = tq2[m][lane][w]; }
#pragma unroll
            for (int k = 0; k < NAUX; k++) {
                if (pm < tm1) { face[0][k] = tau[k][lane][w]; face[1][k] = tau[k][lane][w + 1]; face[2][k] = tau[k][lane][w + 2]; }
                else { face[0][k] = blkR[1][1][k]; face[1][k] = blkR[1][1][k]; face[2][k] = blkR[1][1][k]; }
            }
            if (plane_out && t_owned) {
                const long tg = tbase + (long)(pm - 1) * g.s_m;
#pragma unroll
                for (int m = 0; m < MEQN; m++) g.qacc[m * a.plane + tg] = tout[m][tr][tc];
            }
            __syncthreads();
        } else {
            if (owned && plane_out) {
#pragma unroll
                for (int m = 0; m < MEQN; m++) g.qacc[m * a.plane + gc - g.s_m] = accM[m];
            }
        }
#pragma unroll
        for (int m = 0; m < MEQN; m++) { accM[m] = acc0[m]; acc0[m] = accP[m]; qc[m] = qn[m]; }
        // the block moves one plane along the march axis (y sweep: the y-like index, else the z-like one)
#pragma unroll
        for (int x = 0; x < 3; x++)
#pragma unroll
            for (int k = 0; k < NAUX; k++) {
                if (E_OUTER) { blkR[0][x][k] = blkR[1][x][k]; blkR[1][x][k] = blkR[2][x][k]; blkR[2][x][k] = face[x][k]; }
                else { blkR[x][0][k] = blkR[x][1][k]; blkR[x][1][k] = blkR[x][2][k]; blkR[x][2][k] = face[x][k]; }
            }
    }
    cfl_publish(a.cfl, cfl_value<false>(cflmax, a.dtd));
}

// ---- the general form: any meqn, every component of every split, rpt3 / rptt3 given by the solver --------------------
// For a solver RP with transverse3<DIR, ICOOR>(...) and, where RP::TRANS3 == 2, dtransverse3<DIR, ICOOR>(...) (a user-written
// solver with rpt3 / rptt3 bodies, cellrp.hpp).  Two kernels per direction instead of the march: with 16 user solves per
// interface the pieces of a slice do not stay in registers across a march for general meqn.
//   pieces3_kernel   one wavefront per strip of one slice (e, f), one lane per cell of the sweep line, neighbours by the
//                    lane shifts slice3_pieces_p uses (60 owned cells per wavefront).  Every statement of flux3.f in its
//                    order and association (oracle/classic_oracle.c, flux3_full); as in slice3_pieces_p the splits of
//                    A-dq and of the correction flux of interface l+1 are made in lane l, whose cell they belong to
//                    (imp = 1), after fetching the input from the right-hand lane.  The 14 * meqn values of a cell --
//                    qadd, fadd(i+1) - fadd(i), gadd(1:2, -1:1), hadd(1:2, -1:1) -- go to scratch planes as each is final.
//   gather3_kernel   one thread per interior cell: the nine slices around it in the order of step3.f's loop nest, each
//                    as q = (q + A) + B with pair3p's formulas (26 * meqn reads), the centre's qadd and -dtd * dfadd in front.
// The scratch is dense (no row pitch): cell (i, j, k) with ghost cells at i + n0 * (j + n1 * k), value v of component m
// in plane v * meqn + m (sweep_args.hpp: unsplit3_scratch_bytes).
constexpr int P3_QADD = 0, P3_DF = 1, P3_G = 2, P3_H = 8;      // value index: G / H + 3 * (k - 1) + (j + 1)
static_assert(P3_H + 6 == UNSPLIT3_VALUES, "14 values per cell and component");
struct Pieces3Args {
    double *scr;
    long s_al, s_e, s_f;   // scratch strides (doubles) of the sweep, y-like and z-like directions
    long cells;            // doubles per scratch plane
    int g0, g1, g2;        // the grid of workgroups (g0 fastest); the launch is g0 * g1 * g2 blocks in one dimension
};

// one rpt3: the fluctuation `in` of the interface whose side imp says (1: it belongs to the cell left of the interface,
// 2: right of it); this lane's cell q0 is that cell either way, qm / qp are its left / right neighbours
template <class RP, int DIR, int ICOOR>
__device__ __forceinline__ void rpt3_lane(int imp, const double (&qm)[RP::MEQN], const double (&q0)[RP::MEQN],
                                          const double (&qp)[RP::MEQN], const double (&blk)[3][3][RP::NAUX > 0 ? RP::NAUX : 1],
                                          const RpParams &par, const double (&in)[RP::MEQN], double (&om)[RP::MEQN],
                                          double (&op)[RP::MEQN]) {
    if constexpr (RP::NAUX > 0) RP::template transverse3<DIR, ICOOR>(imp, q0, blk, par, in, om, op);
    else RP::template transverse3<DIR, ICOOR>(imp == 1 ? q0 : qm, imp == 1 ? qp : q0, par, in, om, op);
}
template <class RP, int DIR, int ICOOR>
__device__ __forceinline__ void rptt3_lane(int imp, int impt, const double (&qm)[RP::MEQN], const double (&q0)[RP::MEQN],
                                           const double (&qp)[RP::MEQN], const double (&blk)[3][3][RP::NAUX > 0 ? RP::NAUX : 1],
                                           const RpParams &par, const double (&in)[RP::MEQN], double (&om)[RP::MEQN],
                                           double (&op)[RP::MEQN]) {
    if constexpr (RP::NAUX > 0) RP::template dtransverse3<DIR, ICOOR>(imp, impt, q0, blk, par, in, om, op);
    else RP::template dtransverse3<DIR, ICOOR>(impt, imp == 1 ? q0 : qm, imp == 1 ? qp : q0, par, in, om, op);
}

// A workgroup is P3_NW wavefronts on neighbouring slices of one transverse direction: the one whose index is i, the
// contiguous one, where there is one (y sweep: z-like, z sweep: y-like), so that the wavefronts of a workgroup touch
// neighbouring doubles of every line a lane reads or writes, as march3p_kernel's do; in the x sweep the y-like one.
constexpr int P3_NW = 8;
template <int DIR> constexpr bool p3_waves_on_f() { return DIR == 2; }
template <class RP, int DIR>
__global__ __launch_bounds__(WAVE *P3_NW) void pieces3_kernel(SweepArgs a, Slices3Args t, Pieces3Args g) {
    constexpr int MEQN = RP::MEQN, MWAVES = RP::MWAVES, NAUX = RP::NAUX, NB = NAUX > 0 ? NAUX : 1;
    using Cell = typename RP::Cell;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    // block indices of the strip along the sweep and of the y-like / z-like slices.  The fastest one, b0, runs along i in
    // every direction, and workgroups that are neighbours along i run on the same XCD close in time (xcd_logical_block):
    // the 60-cell strips and the P3_NW-column tiles are not line-aligned, so neighbours share lines of q and aux and write
    // the two parts of scratch lines, which merge in that XCD's L2 before they go to HBM
    const int bid = xcd_logical_block();
    const int b0 = bid % g.g0, b1 = (bid / g.g0) % g.g1, b2 = bid / (g.g0 * g.g1);
    const int bs = DIR == 1 ? b0 : b2;
    const int be = DIR == 3 ? b0 : b1;
    const int bf = DIR == 1 ? b2 : DIR == 2 ? b0 : b1;
    const int ca = a.mbc - HALO + bs * STRIP + lane;
    const int cc = ca < a.n_al ? ca : a.n_al - 1;
    // y and z sweeps: the lanes of a wavefront are a row / a plane of the array apart, 64 lines per load / store
    // instruction.  Their wave axis is i: the workgroup moves q in and the 14 * meqn results out as 64-row x P3_NW-column
    // tiles, 64 B per row segment, transposed through LDS (STAGED; as march3p_kernel's tiles).  A wavefront past the last
    // swept slice then stays for the barriers: it computes that last slice again and stores nothing.
    constexpr bool STAGED = DIR != 1;
    constexpr int SV = 8;       // values the stage holds at once: MEQN <= 8 components of q, or a group of results
    static_assert(MEQN <= SV && SV >= 6, "the stage holds q of one cell and the six G or H values of one component");
    __shared__ double stg[STAGED ? SV : 1][STAGED ? WAVE : 1][STAGED ? P3_NW + 1 : 1];
    const int we = t.lo_e + (p3_waves_on_f<DIR>() ? be : be * P3_NW + w);
    const int wf = t.lo_f + (p3_waves_on_f<DIR>() ? bf * P3_NW + w : bf);
    if (!STAGED && (we > t.hi_e || wf > t.hi_f)) return;     // (wave-uniform, and no barrier on this path)
    const int ce = we > t.hi_e ? t.hi_e : we, cf = wf > t.hi_f ? t.hi_f : wf;
    const bool owned = (ca >= a.mbc) && (ca < a.mbc + a.m_al) && lane >= HALO && lane < WAVE - HALO;
    const bool cfl_ok = (ca >= a.mbc) && (ca <= a.mbc + a.m_al) && lane >= 1;
    const long gq = (long)cc * a.s_al + (long)ce * t.s_e + (long)cf * t.s_f;
    // this thread's cell of the cooperative tiles: row tr along the sweep, column tc along the wave axis
    const int tc = threadIdx.x % P3_NW, tr = threadIdx.x / P3_NW;
    const int ta = a.mbc - HALO + bs * STRIP + tr;
    const int te_w = t.lo_e + (p3_waves_on_f<DIR>() ? be : be * P3_NW + tc);
    const int tf_w = t.lo_f + (p3_waves_on_f<DIR>() ? bf * P3_NW + tc : bf);
    const bool t_owned = (ta >= a.mbc) && (ta < a.mbc + a.m_al) && tr >= HALO && tr < WAVE - HALO && te_w <= t.hi_e && tf_w <= t.hi_f;
    const int te = te_w > t.hi_e ? t.hi_e : te_w, tf = tf_w > t.hi_f ? t.hi_f : tf_w;
    const long tgs = (long)ta * g.s_al + (long)te * g.s_e + (long)tf * g.s_f;      // (used where t_owned: inside the scratch)
    double q[MEQN], blk[3][3][NB];
    // the aux block's offsets are clamped like load_blk's: every USED block lies inside the array (slices 0..m+1, mbc = 2)
    if constexpr (STAGED) {
        const long tgq = (long)(ta < a.n_al ? ta : a.n_al - 1) * a.s_al + (long)te * t.s_e + (long)tf * t.s_f;
#pragma unroll
        for (int m = 0; m < MEQN; m++) stg[m][tr][tc] = a.qin[m * a.plane + tgq];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MEQN; m++) q[m] = stg[m][lane][w];
        __syncthreads();
        // the 9 * NAUX values of the block, SV tiles at a time: value x = ((oe + 1) * 3 + (of + 1)) * NAUX + k
        constexpr int NX = NAUX > 0 ? 9 * NAUX : 0;
#pragma unroll
        for (int x0 = 0; x0 < NX; x0 += SV) {
#pragma unroll
            for (int j = 0; j < SV; j++) {
                const int x = x0 + j;
                if (x < NX) {
                    const int oe = x / (3 * NB) - 1, of = (x / NB) % 3 - 1, k = x % NB;
                    const int de = (te + oe < 0) ? 0 : (te + oe >= t.n_e ? 0 : oe);
                    const int df_ = (tf + of < 0) ? 0 : (tf + of >= t.n_f ? 0 : of);
                    stg[j][tr][tc] = a.aux[aux_idx<RP, DIR>(k) * a.plane + tgq + de * t.s_e + df_ * t.s_f];
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SV; j++) {
                const int x = x0 + j;
                if (x < NX) blk[x / (3 * NB)][(x / NB) % 3][x % NB] = stg[j][lane][w];
            }
            __syncthreads();
        }
        if constexpr (NAUX == 0) {
#pragma unroll
            for (int x = 0; x < 9; x++) blk[x / 3][x % 3][0] = 0.0;
        }
    } else {
#pragma unroll
        for (int m = 0; m < MEQN; m++) q[m] = a.qin[m * a.plane + gq];
#pragma unroll
        for (int oe = -1; oe <= 1; oe++)
#pragma unroll
            for (int of = -1; of <= 1; of++) {
                const int de = (ce + oe < 0) ? 0 : (ce + oe >= t.n_e ? 0 : oe);
                const int df_ = (cf + of < 0) ? 0 : (cf + of >= t.n_f ? 0 : of);
#pragma unroll
                for (int k = 0; k < NB; k++)
                    blk[oe + 1][of + 1][k] = NAUX > 0 ? a.aux[aux_idx<RP, DIR>(k) * a.plane + gq + de * t.s_e + df_ * t.s_f] : 0.0;
            }
    }
    const double d = a.dtd;
    Cell cR;
    if constexpr (NAUX > 0) {
        double auxv[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) auxv[k] = blk[1][1][k];
        cR = RP::template precell<DIR>(q, a.par, auxv);
    } else cR = RP::template precell<DIR>(q, a.par);
    const Cell cL = struct_from_left(cR);
    double wave[MWAVES][MEQN], s[MWAVES], amdq[MEQN], apdq[MEQN];
    RP::template solve<DIR>(cL, cR, a.par, wave, s, amdq, apdq);
    double cflmax = 0.0;
    cfl_accumulate<false, MWAVES>(s, d, d, cfl_ok, cflmax);
    cfl_publish(a.cfl, cfl_value<false>(cflmax, a.dtd));
    double cq[MEQN];
#pragma unroll
    for (int m = 0; m < MEQN; m++) cq[m] = 0.0;
    if (a.order != 1) {
#pragma unroll
        for (int mw = 0; mw < MWAVES; mw++) {
            const int lim = a.mthlim[mw];
            if (lim == 0) continue;
            double wn = 0.0, dl = 0.0;
#pragma unroll
            for (int m = 0; m < MEQN; m++) {
                const double w = wave[mw][m], wl = from_left(w);
                wn = m == 0 ? w * w : wn + w * w;
                dl = m == 0 ? wl * w : dl + wl * w;
            }
            const double dr = from_right(dl);
            if (wn != 0.0) {
                const double phi = philim(wn, s[mw] > 0.0 ? dl : dr, lim);
#pragma unroll
                for (int m = 0; m < MEQN; m++) wave[mw][m] = phi * wave[mw][m];
            }
        }
        const double dtdxave = 0.5 * (d + d);
#pragma unroll
        for (int m = 0; m < MEQN; m++) {
            double c = 0.0;
#pragma unroll
            for (int mw = 0; mw < MWAVES; mw++) {
                const double sa = fabs(s[mw]);
                const double term = 0.5 * sa * (1.0 - sa * dtdxave) * wave[mw][m];
                c = mw == 0 ? term : c + term;
            }
            cq[m] = c;
        }
    }
    const long gs = (long)cc * g.s_al + (long)ce * g.s_e + (long)cf * g.s_f;
    // STAGED: put(slot, ...) leaves a value in the stage and flush(n, plane of slot k) moves the first n slots out; else put
    // stores at once and flush does nothing
    auto put = [&](int slot, int v, int m, double x) {
        if constexpr (STAGED) stg[slot][lane][w] = x;
        else if (owned) g.scr[(long)(v * MEQN + m) * g.cells + gs] = x;
    };
    auto flush = [&](int n, auto plane_of) {
        if constexpr (STAGED) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < SV; k++)
                if (k < n && t_owned) g.scr[(long)plane_of(k) * g.cells + tgs] = stg[k][tr][tc];
            __syncthreads();
        }
    };
    // the fluctuations and correction fluxes of this cell: A+dq and cqxx of interface l (imp = 2), A-dq and cqxx of
    // interface l+1 (imp = 1)
    double aP[MEQN], aM[MEQN], kP[MEQN], kM[MEQN], qm[MEQN], qp[MEQN];
#pragma unroll
    for (int m = 0; m < MEQN; m++) {
        aP[m] = apdq[m]; aM[m] = from_right(amdq[m]);
        kP[m] = cq[m]; kM[m] = from_right(cq[m]);
        qm[m] = NAUX > 0 ? 0.0 : from_left(q[m]);
        qp[m] = NAUX > 0 ? 0.0 : from_right(q[m]);
    }
#pragma unroll
    for (int m = 0; m < MEQN; m++) {
        put(0, P3_QADD, m, -(d * aP[m]) - d * aM[m]);
        put(1, P3_DF, m, kM[m] - kP[m]);
        flush(2, [&](int k) { return k * MEQN + m; });
    }
    const int m3 = t.m3, m4 = t.m4;
    if (m3 <= 0) {      // flux3.f:260: no transverse propagation (the same for every wavefront)
#pragma unroll
        for (int m = 0; m < MEQN; m++) {
#pragma unroll
            for (int k = 0; k < 6; k++) put(k, P3_G + k, m, 0.0);
            flush(6, [&](int k) { return (P3_G + k) * MEQN + m; });
#pragma unroll
            for (int k = 0; k < 6; k++) put(k, P3_H + k, m, 0.0);
            flush(6, [&](int k) { return (P3_H + k) * MEQN + m; });
        }
        return;
    }
#define PCL_T3(ICOOR, imp, in, om, op) rpt3_lane<RP, DIR, ICOOR>(imp, qm, q, qp, blk, a.par, in, om, op)
#define PCL_TT3(ICOOR, imp, impt, in, om, op) rptt3_lane<RP, DIR, ICOOR>(imp, impt, qm, q, qp, blk, a.par, in, om, op)
    // names as in flux3.f; the ...amdq / ...cqxxm ones are those of interface l+1
    double bmamdq[MEQN], bpamdq[MEQN], bmapdq[MEQN], bpapdq[MEQN], cmamdq[MEQN], cpamdq[MEQN], cmapdq[MEQN], cpapdq[MEQN];
    PCL_T3(2, 1, aM, bmamdq, bpamdq);
    PCL_T3(2, 2, aP, bmapdq, bpapdq);
    PCL_T3(3, 1, aM, cmamdq, cpamdq);
    PCL_T3(3, 2, aP, cmapdq, cpapdq);
    double bmcqxxm[MEQN], bpcqxxm[MEQN], bmcqxxp[MEQN], bpcqxxp[MEQN], cmcqxxm[MEQN], cpcqxxm[MEQN], cmcqxxp[MEQN], cpcqxxp[MEQN];
#pragma unroll
    for (int m = 0; m < MEQN; m++) {
        bmcqxxm[m] = 0.0; bpcqxxm[m] = 0.0; bmcqxxp[m] = 0.0; bpcqxxp[m] = 0.0;
        cmcqxxm[m] = 0.0; cpcqxxm[m] = 0.0; cmcqxxp[m] = 0.0; cpcqxxp[m] = 0.0;
    }
    if (m3 == 2) {      // flux3.f:299-337: with aux one split per side; without, the same values from the side's own pair
        PCL_T3(2, 1, kM, bmcqxxm, bpcqxxm);
        PCL_T3(2, 2, kP, bmcqxxp, bpcqxxp);
        PCL_T3(3, 1, kM, cmcqxxm, cpcqxxm);
        PCL_T3(3, 2, kP, cmcqxxp, cpcqxxp);
    }
    // one component of the six G (or H) values of this cell: flux3.f's statements in their order (slice3_pieces_p: six)
    auto six = [&](int vbase, int m, double k6, double bmap, double bpap, double bmam, double bpam, double xmcpap, double xpcpap,
                   double xmcmap, double xpcmap, double xmcpam, double xpcpam, double xmcmam, double xpcmam, double qmp, double qpp,
                   double qmm, double qpm) {
        double g10 = 0.0, g20 = 0.0, g21 = 0.0, g11 = 0.0, g2m = 0.0, g1m = 0.0;
        g10 = g10 - 0.5 * d * bmap;
        g20 = g20 - 0.5 * d * bpap;
        if (m4 > 0) {
            g20 = g20 + k6 * (xpcpap - xpcmap);
            g10 = g10 + k6 * (xmcpap - xmcmap);
            g21 = g21 - k6 * xpcpap;
            g11 = g11 - k6 * xmcpap;
            g2m = g2m + k6 * xpcmap;
            g1m = g1m + k6 * xmcmap;
        }
        if (m3 >= 2) {
            g20 = g20 + d * qpp;
            g10 = g10 + d * qmp;
        }
        g10 = g10 - 0.5 * d * bmam;                 // interface l+1
        g20 = g20 - 0.5 * d * bpam;
        if (m4 > 0) {
            g20 = g20 + k6 * (xpcpam - xpcmam);
            g10 = g10 + k6 * (xmcpam - xmcmam);
            g21 = g21 - k6 * xpcpam;
            g11 = g11 - k6 * xmcpam;
            g2m = g2m + k6 * xpcmam;
            g1m = g1m + k6 * xmcmam;
        }
        if (m3 >= 2) {
            g20 = g20 - d * qpm;
            g10 = g10 - d * qmm;
        }
        // value index vbase + 3 * (k - 1) + (j + 1)
        put(0, vbase + 0, m, g1m); put(1, vbase + 1, m, g10); put(2, vbase + 2, m, g11);
        put(3, vbase + 3, m, g2m); put(4, vbase + 4, m, g20); put(5, vbase + 5, m, g21);
        flush(6, [&](int k) { return (vbase + k) * MEQN + m; });
    };
    const double k6z = (1.0 / 6.0) * d * t.dtz, k6y = (1.0 / 6.0) * d * t.dty;
    double xmcpap[MEQN], xpcpap[MEQN], xmcpam[MEQN], xpcpam[MEQN], xmcmap[MEQN], xpcmap[MEQN], xmcmam[MEQN], xpcmam[MEQN];
    auto zero8 = [&]() {
#pragma unroll
        for (int m = 0; m < MEQN; m++) {
            xmcpap[m] = 0.0; xpcpap[m] = 0.0; xmcpam[m] = 0.0; xpcpam[m] = 0.0;
            xmcmap[m] = 0.0; xpcmap[m] = 0.0; xmcmam[m] = 0.0; xpcmam[m] = 0.0;
        }
    };
    {   // ---- G fluxes (y-like), flux3.f:347-452: the z-like splits (corrected by the correction waves' for m4 = 2)
        // split again in the y-like direction, inside the z-like row they went to
        zero8();
        if constexpr (RP::TRANS3 >= 2) {
            if (m4 > 0) {
                double pp[MEQN], pm[MEQN], mp[MEQN], mm[MEQN];
#pragma unroll
                for (int m = 0; m < MEQN; m++) {
                    pp[m] = m4 == 2 ? cpapdq[m] - 3.0 * cpcqxxp[m] : cpapdq[m];
                    pm[m] = m4 == 2 ? cpamdq[m] + 3.0 * cpcqxxm[m] : cpamdq[m];
                    mp[m] = m4 == 2 ? cmapdq[m] - 3.0 * cmcqxxp[m] : cmapdq[m];
                    mm[m] = m4 == 2 ? cmamdq[m] + 3.0 * cmcqxxm[m] : cmamdq[m];
                }
                PCL_TT3(2, 2, 2, pp, xmcpap, xpcpap);
                PCL_TT3(2, 1, 2, pm, xmcpam, xpcpam);
                PCL_TT3(2, 2, 1, mp, xmcmap, xpcmap);
                PCL_TT3(2, 1, 1, mm, xmcmam, xpcmam);
            }
        }
#pragma unroll
        for (int m = 0; m < MEQN; m++)
            six(P3_G, m, k6z, bmapdq[m], bpapdq[m], bmamdq[m], bpamdq[m], xmcpap[m], xpcpap[m], xmcmap[m], xpcmap[m], xmcpam[m],
                xpcpam[m], xmcmam[m], xpcmam[m], bmcqxxp[m], bpcqxxp[m], bmcqxxm[m], bpcqxxm[m]);
    }
    {   // ---- H fluxes (z-like), flux3.f:462-590: the y-like splits (corrected for m4 = 2) split again in the z-like direction
        zero8();
        if constexpr (RP::TRANS3 >= 2) {
            if (m4 > 0) {
                double pp[MEQN], pm[MEQN], mp[MEQN], mm[MEQN];
#pragma unroll
                for (int m = 0; m < MEQN; m++) {
                    pp[m] = m4 == 2 ? bpapdq[m] - 3.0 * bpcqxxp[m] : bpapdq[m];
                    pm[m] = m4 == 2 ? bpamdq[m] + 3.0 * bpcqxxm[m] : bpamdq[m];
                    mp[m] = m4 == 2 ? bmapdq[m] - 3.0 * bmcqxxp[m] : bmapdq[m];
                    mm[m] = m4 == 2 ? bmamdq[m] + 3.0 * bmcqxxm[m] : bmamdq[m];
                }
                PCL_TT3(3, 2, 2, pp, xmcpap, xpcpap);
                PCL_TT3(3, 1, 2, pm, xmcpam, xpcpam);
                PCL_TT3(3, 2, 1, mp, xmcmap, xpcmap);
                PCL_TT3(3, 1, 1, mm, xmcmam, xpcmam);
            }
        }
#pragma unroll
        for (int m = 0; m < MEQN; m++)
            six(P3_H, m, k6y, cmapdq[m], cpapdq[m], cmamdq[m], cpamdq[m], xmcpap[m], xpcpap[m], xmcmap[m], xpcmap[m], xmcpam[m],
                xpcpam[m], xmcmam[m], xpcmam[m], cmcqxxp[m], cpcqxxp[m], cmcqxxm[m], cpcqxxm[m]);
    }
#undef PCL_T3
#undef PCL_TT3
}

// what a gather launch needs: the scratch, where a cell's accumulator starts from (qold in the x direction, the state
// accumulated so far in y and z) and the result; threads run over (i, j, k) with i, the contiguous index, fastest in
// every direction, and the direction only names the strides of the y-like and z-like neighbours
struct Gather3Args {
    const double *scr, *qsrc;
    double *qacc;
    long plane;                 // doubles between components of q
    long s[3];                  // strides of q (doubles) along x, y, z
    long c[3], cells;           // the same of the scratch, and doubles per scratch plane
    long c_e, c_f;              // scratch strides of the y-like / z-like direction
    int mbc, m[3], meqn;
    double dtd, dty, dtz;
};

// E_OUTER: the y-like index is the outer one of step3.f's loop nest (the y sweep), else the z-like one
template <bool E_OUTER>
__global__ __launch_bounds__(256) void gather3_kernel(Gather3Args g) {
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 >= g.m[0] || (int)blockIdx.y >= g.m[1] || (int)blockIdx.z >= g.m[2]) return;
    const int c0 = g.mbc + i0, c1 = g.mbc + (int)blockIdx.y, c2 = g.mbc + (int)blockIdx.z;
    const long gq = (long)c0 * g.s[0] + (long)c1 * g.s[1] + (long)c2 * g.s[2];
    const long gs = (long)c0 * g.c[0] + (long)c1 * g.c[1] + (long)c2 * g.c[2];
    const double dty = g.dty, dtz = g.dtz;
    for (int m = 0; m < g.meqn; m++) {
        double v = g.qsrc[m * g.plane + gq];
#pragma unroll
        for (int so = -1; so <= 1; so++)
#pragma unroll
            for (int si = -1; si <= 1; si++) {
                // the source slice at (se, sf) from here; this cell lies at (oe, of) = (-se, -sf) from it
                const int se = E_OUTER ? so : si, sf = E_OUTER ? si : so;
                const int oe = -se, of = -sf;
                const long src = gs + se * g.c_e + sf * g.c_f;
                auto val = [&](int vi) { return g.scr[(long)(vi * g.meqn + m) * g.cells + src]; };
                auto G_ = [&](int k, int j) { return val(P3_G + 3 * (k - 1) + (j + 1)); };
                auto H_ = [&](int k, int j) { return val(P3_H + 3 * (k - 1) + (j + 1)); };
                double A, B;      // step3.f's update formulas, as pair3p
                if (oe == 0 && of == 0) {
                    v = v + val(P3_QADD);
                    v = v - g.dtd * val(P3_DF);
                    A = -(dty * (G_(2, 0) - G_(1, 0))); B = -(dtz * (H_(2, 0) - H_(1, 0)));
                } else if (oe == -1 && of == 0) { A = -(dty * G_(1, 0)); B = -(dtz * (H_(2, -1) - H_(1, -1))); }
                else if (oe == -1 && of == -1) { A = -(dty * G_(1, -1)); B = -(dtz * H_(1, -1)); }
                else if (oe == 0 && of == -1) { A = -(dty * (G_(2, -1) - G_(1, -1))); B = -(dtz * H_(1, 0)); }
                else if (oe == 1 && of == -1) { A = dty * G_(2, -1); B = -(dtz * H_(1, 1)); }
                else if (oe == 1 && of == 0) { A = dty * G_(2, 0); B = -(dtz * (H_(2, 1) - H_(1, 1))); }
                else if (oe == 1 && of == 1) { A = dty * G_(2, 1); B = dtz * H_(2, 1); }
                else if (oe == 0 && of == 1) { A = -(dty * (G_(2, 1) - G_(1, 1))); B = dtz * H_(2, 0); }
                else { A = -(dty * G_(1, 1)); B = dtz * H_(2, -1); }
                v = (v + A) + B;
            }
        g.qacc[m * g.plane + gq] = v;
    }
}

// ghost frame of the accumulated state := the old state's (the first direction writes interior cells only)
__global__ __launch_bounds__(256) void ghost3_copy_kernel(const double *src, double *dst, int meqn, long plane, int I, int J, int K,
                                                           long pitch, int mbc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
    if (i >= I) return;
    if (i >= mbc && i < I - mbc && j >= mbc && j < J - mbc && k >= mbc && k < K - mbc) return;
    const long c = ((long)k * J + j) * pitch + i;
    for (int m = 0; m < meqn; m++) dst[m * plane + c] = src[m * plane + c];
}

}  // namespace PCL_NS
}  // namespace pcl
