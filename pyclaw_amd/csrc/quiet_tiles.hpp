// quiet_tiles.hpp -- host state of the quiet tiles of the one-kernel dim-split step (host only, included by pclaw.hip;
// the kernels: classic_fused.hpp, the proofs: DESIGN.md 4.1a).
//
// Device memory: three word arrays W[0..2] (one 32-bit word per tile), the per-wavefront Courant maxima C, the tile
// list L, the ring marks R (one 32-bit word per tile), the row-reuse counts U and the column-shortcut counts Y (each two
// words per tile: the launch's number and one byte per wavefront) and three TileNext blocks N[0..2].  Two counters rotate them: c
// (words) advances with every booked launch, x (blocks) with every hand-over that built a list; r numbers the booked
// launches.  With c and x taken in front of launch n (indices modulo 3):
//
//                                  reads                       writes                            then
//   launch n        plan()         L, N[x+2] if it skips       W[c+1], C (computed tiles),       c += 1, r += 1
//                                                              R := r (tiles its ring check
//                                                              settled, classic_fused.hpp),
//                                                              U, Y (computed tiles: r and the counts)
//   hand-over n     handover()     W[c+1], C, N[x+2] if        W[c+2] (tiles n + 1 skips), L,    x += 1
//                                  launch n ran over a list    N[x] filled, N[x+1] zeroed,
//                                  (its na + nq)               host word [2] (tiles launch n ran)
//   launch n + 1    plan()         L, N[x] if it skips         W[c+2], C (computed tiles), R
//   a hook between                 W[c]   (words_read)         nothing
//                                  N[x+2] (ran_over)
//                                  R      (ring_marks: the words equal to r)
//                                  U      (reuse_counts: the tiles whose first word equals r)
//                                  Y      (ycol_counts: the same)
//
// Host word [2] (next to the Courant number [0] and the sequence number [1]) is read by the form-trial gate of
// step_hyperbolic (pclaw.hip) while list_count_current() holds: no read-back, no wait.
// N[x] is filled with atomics, so it must be zero: the hand-over before zeroed it.  A launch with skipping switched off,
// or one whose step fails before its hand-over, advances c and not x; one counter for both would then have the next
// hand-over fill a block that nobody zeroed, so there are two.  A hand-over launch that fails zeroes all three blocks
// and restarts x at 0.
//
// Flags, and the only events that change them:
//   valid    the last launch was a booked one, last_in -> last_out with last_key, and since then only the buffer swap of
//            the step and read-only calls have happened.  Set by launched(); cleared by invalidate() (the first statement
//            of every C entry point that is neither a step nor read-only: tests/test_quiet_tiles_cpu.py), by take_valid()
//            (the step entry points; the value travels down to plan() as `carry`) and by plan().  adopted() gives the
//            taken value back when the step asked for is the launch it was set for (a step enqueued ahead).
//   hand     a hand-over with a list is due behind the last launch.  Set by launched() while skipping is enabled;
//            cleared by handover() and plan().
//   listed   L and N[x-1] hold the list of the next launch.  Set by handed_over(true); cleared by handover() (every
//            Courant read-back: a later step of another form drops the list) and plan().
//   last     what the last launch was (NONE / ALL / LIST), for the hooks.  Set by launched(); cleared by plan().
// drop() clears all four: a step that was enqueued ahead of the caller and not adopted (pclaw.hip: step ahead).
#pragma once
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>

#include "sweep_args.hpp"

namespace pcl {

class QuietTiles {
public:
    // the settings two launches must share for the words of one to decide the other (compared bytewise)
    struct Key {
        int rp, fwave, math, src;
        long module;        // the id of the attached module of a user-written solver (cellrp.hpp), 0 for a built-in one:
                            // two bodies share rp = PCL_RP_CELL, and a skipped tile's cached Courant maxima are the body's speeds
        double src_p[2];
        RpParams par;
        Key(int rp_, long module_, int fwave_, int math_, const SweepArgs &a) {
            memset(this, 0, sizeof(Key));
            rp = rp_; module = module_; fwave = fwave_; math = math_; src = a.src_id;
            src_p[0] = a.src_p[0]; src_p[1] = a.src_p[1];
            par = a.par;
        }
        Key() { memset(this, 0, sizeof(Key)); }
        bool operator==(const Key &o) const { return memcmp(this, &o, sizeof(Key)) == 0; }
    };
    enum Last { NONE = 0, ALL = 1, LIST = 2 };   // no booked launch / it computed every tile / it ran over the list

    int ntx = 0, nty = 0;

    // mx x my interior cells; the blocks are zeroed on `stream`
    hipError_t create(int mx, int my, hipStream_t stream) {
        ntx = (mx + TILE_OWN_C - 1) / TILE_OWN_C;
        nty = (my + TILE_OWN_R - 1) / TILE_OWN_R;
        const size_t nt = (size_t)ntx * nty;
        hipError_t e = hipSuccess;
        for (auto &w : words)
            if (e == hipSuccess) e = hipMalloc((void **)&w, nt * sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc((void **)&cfl, nt * 4 * sizeof(double2));
        if (e == hipSuccess) e = hipMalloc((void **)&list, nt * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void **)&ring, nt * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(ring, 0, nt * sizeof(unsigned), stream);
        if (e == hipSuccess) e = hipMalloc((void **)&reuse, 2 * nt * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(reuse, 0, 2 * nt * sizeof(unsigned), stream);
        if (e == hipSuccess) e = hipMalloc((void **)&ycol, 2 * nt * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(ycol, 0, 2 * nt * sizeof(unsigned), stream);
        if (e == hipSuccess) e = hipMalloc((void **)&next, 3 * sizeof(TileNext));
        if (e == hipSuccess) e = hipMemsetAsync(next, 0, 3 * sizeof(TileNext), stream);
        return e;
    }
    void destroy() {
        for (unsigned *w : words)
            if (w) hipFree(w);
        if (cfl) hipFree(cfl);
        if (list) hipFree(list);
        if (ring) hipFree(ring);
        if (reuse) hipFree(reuse);
        if (ycol) hipFree(ycol);
        if (next) hipFree(next);
    }

    void invalidate() { valid = false; }
    bool take_valid() { const bool v = valid; valid = false; return v; }
    // A step enqueued ahead (pclaw.hip: step ahead) that nobody asked for: its launch and its hand-over ran, its result is
    // not the state.  Every flag down, as plan() leaves them: the next launch computes every tile and lists afresh.  c, x
    // and r have moved on with the launch and its hand-over, which is what keeps the words and the blocks consistent.
    void drop() {
        valid = hand = listed = false;
        last = NONE;
    }
    // The step entry point took the flag (true: nothing but read-only calls since the launch) and found that the launch
    // it was set for is the very step it is asked for (pclaw.hip: ahead_adopt): nothing is launched, so launched() does
    // not set it again -- the flag goes back as it was taken.
    void adopted(bool taken) { valid = taken; }
    // the last launch was a booked one with the next launch's list behind it, and nothing has happened since
    bool list_behind_last() const { return valid && listed; }
    void set_enabled(bool on) { enabled = on; }
    void set_ring(bool on) { ring_on = on; }
    void set_rowreuse(bool on) { reuse_on = on; }
    void set_ycol(bool on) { ycol_on = on; }

    // In front of a one-kernel launch qin -> qout: fills l.tq_* and returns true if the launch is booked (`whole`: the
    // whole undecomposed block).  Every flag is cleared; launched() sets them again.  The row-reuse and column-shortcut
    // switches go to every launch, booked or not (tile subsets of a decomposed block: the same kernel); their counts only
    // to a booked one.
    bool plan(SweepLaunch &l, const double *qin, const double *qout, const Key &key, double dt, bool whole, bool carry) {
        const bool book = whole && words[0];
        l.rowreuse = reuse_on ? 1 : 0;
        l.ycol = ycol_on ? 1 : 0;
        if (book) {
            l.tq_reuse = reuse;
            l.tq_ycol = ycol;
            l.tq_out = written_next();
            l.tq_cfl = cfl;
            if (++ring_seq == 0) ring_seq = 1;          // 0 is what create() left in R
            l.ring_seq = ring_seq;
            if (may_skip(qin, qout, key, dt, carry)) {
                l.tq_list = list;
                l.tq_next = block(2);
                if (ring_on) l.tq_ring = ring;
            }
        }
        valid = hand = listed = false;
        last = NONE;
        return book;
    }
    // the booked launch was enqueued
    void launched(const SweepLaunch &l, const double *qin, const double *qout, const Key &key) {
        c = (c + 1) % 3;
        valid = true;
        last_in = qin;
        last_out = qout;
        last_key = key;
        last = l.tq_list ? LIST : ALL;
        stat = block(2);
        hand = enabled;
    }

    // In front of the Courant hand-over: true if it takes the next launch's list with it, h's tile fields filled.
    bool handover(TileHandover &h) {
        const bool due = hand;
        hand = listed = false;
        if (due) {
            h.ntx = ntx;
            h.nty = nty;
            h.tq_in = written();
            h.tq_out = written_next();
            h.tq_cfl = cfl;
            h.tq_list = list;
            h.next = block(0);
            h.other = block(1);
            h.ran = last == LIST ? stat : nullptr;
        }
        return due;
    }
    // ok: that hand-over was enqueued; not ok: nothing ran, the list state back to its start (every block zero)
    void handed_over(bool ok, hipStream_t stream) {
        if (ok) {
            listed = true;
            x = (x + 1) % 3;
        } else {
            (void)hipMemsetAsync(next, 0, 3 * sizeof(TileNext), stream);
            x = 0;
        }
    }

    // for the hooks, behind the last launch
    Last last_launch() const { return last; }
    const unsigned *words_read() const { return words[(c + 2) % 3]; }   // the words its list was built from
    const TileNext *ran_over() const { return stat; }                   // the block of that list (last_launch() == LIST)
    const unsigned *ring_marks() const { return ring; }                 // a tile its ring check settled holds ring_number()
    unsigned ring_number() const { return ring_seq; }
    const unsigned *reuse_counts() const { return reuse; }              // per tile: the number of the launch that computed it
                                                                        // last, then its x sweeps reused, a byte per wavefront
    const unsigned *ycol_counts() const { return ycol; }                // the same layout: its y-sweep calls that took the
                                                                        // column shortcut
    // The last launch ran over a list and the launch to come would run over the next one (carry: QuietTiles::take_valid
    // at the step's entry point): the count its hand-over left in host memory describes the state as it is now.
    bool list_count_current(bool carry) const { return carry && last == LIST && listed; }

private:
    unsigned *words[3] = {nullptr, nullptr, nullptr};
    double2 *cfl = nullptr;
    int *list = nullptr;
    TileNext *next = nullptr;
    int c = 0, x = 0;
    const TileNext *stat = nullptr;
    bool enabled = true;                // pcl_tile_skip
    unsigned *ring = nullptr;
    unsigned ring_seq = 0;              // the number of the last booked launch
    bool ring_on = true;                // pcl_tile_ring
    unsigned *reuse = nullptr;
    bool reuse_on = true;               // pcl_tile_rowreuse
    unsigned *ycol = nullptr;
    bool ycol_on = true;                // pcl_tile_ycol
    bool valid = false, hand = false, listed = false;
    Last last = NONE;
    const double *last_in = nullptr, *last_out = nullptr;
    Key last_key;

    unsigned *written() const { return words[c]; }                  // by the last launch
    unsigned *written_next() const { return words[(c + 1) % 3]; }   // by the next launch and, for the tiles it skips, the list kernel
    TileNext *block(int k) const { return next + (x + k) % 3; }     // 0: the next hand-over fills it, 1: zeroes it, 2: the last one filled it

    // The next launch may run over the list: skipping is on, the previous launch ran on the swapped pair with the same
    // settings, the list behind it was built and nothing has happened since (carry); under the fused source its
    // fixed-point test (euler_radial_source_fixed) holds for these dt, gamma1 and ndim - 1; dt is positive and finite
    // (the skipped tiles' Courant number: DESIGN.md 4.1a).
    bool may_skip(const double *qin, const double *qout, const Key &key, double dt, bool carry) const {
        const bool src_ok = key.src == 0 || (dt <= SRC_FIXED_BOUND && fabs(key.src_p[0]) <= SRC_FIXED_BOUND &&
                                             fabs(key.src_p[1]) <= SRC_FIXED_BOUND);
        return enabled && carry && listed && last_in == qout && last_out == qin && last_key == key && src_ok && dt > 0.0 &&
               dt < HUGE_VAL;
    }
};

}  // namespace pcl
