// step_form.hpp -- which form of the dimension-split 2-D step runs (host only, no device, no clock, no environment:
// included by pclaw.hip, which passes in what it read; the rule: DESIGN.md 4.1a; the tests: tests/test_step_form_cpu.py
// through pcl_step_form_trace).
//
// The two forms give identical results: 1 = one kernel, 0 = two passes.  PCL_TUNE_FUSED_STEP = 0 pins the two passes,
// 1 the one kernel, 2 (default) takes the faster of the two: 64 steps into every window of WINDOW tuned steps either
// the tile count of the last launch settles it (a list launch dispatched for a quarter of the tiles or fewer: one
// kernel for the whole window, nothing timed) or a few steps of each form are timed on the host (a step ends with the
// Courant number's read-back) and the rest of the window runs the faster one.  The one-kernel step halves the HBM
// traffic and wins wherever most wavefronts take the no-jump shortcut; where every cell is active its halo rows
// (32 / 28 of the arithmetic) make the two passes faster.
//
// A step is TUNED where the one-kernel form is possible, the mode is 2 and the block is whole or steps behind its
// exchange (pclaw.hip: step_hyperbolic); every other step takes `can ? 1 : 0` and leaves the window alone.  With
// k = step mod WINDOW - T0 (phase()), the ranges of k, each named once below:
//   gate step       k = 0                 the best times reset; the window is gated iff listed >= 0 and
//                                         4 listed <= ntiles, and a gated window's form is one kernel
//   trial step      k = 0 .. 2 (TRIAL+1) - 1   of an ungated window: the first TRIAL + 1 run one kernel, the others the
//                                         two passes; the first of each form is untimed, the best time of the others is kept
//   verdict step    k = 2 (TRIAL+1)       of an ungated window: two passes iff t[0] < 0.98 t[1]
//   every other k                         the window's form
//
// Fields, and the only events that change them:
//   now      the window's form.  Set by begin() at a gated window's gate step (1) and at an ungated one's verdict step.
//   step     tuned steps so far.  Advanced by end() behind a tuned step and by adopted() in mode 2 (a step enqueued
//            ahead is a plain one-kernel step of its window: next_is_plain_onek()).
//   t[2]     best wall time of a timed trial step of each form in this window.  Reset by begin() at the gate step,
//            lowered by end() behind a timed step.
//   gated    this window has no trials.  Set or cleared by begin() at the gate step.
//   was      the form of the last dim-split 2-D step, -1: none since forget_last().  Set by begin() and adopted(),
//            cleared by forget_last() (pcl_bc_step, in front of its plans).
//   n[2]     steps run in each form (pcl_step_form_stats).  Bumped by end(), ran() and adopted(); zeroed by
//            reset_counts() (pcl_kernel_timing).
#pragma once

namespace pcl {

class StepForm {
public:
    // form: 1 = one kernel, 0 = two passes; tuned: the step belongs to the window, end() advances it; timed: end() wants
    // the step's wall time (launch to Courant read-back), in seconds
    struct Pick { int form; bool tuned, timed; };

    // In front of a dim-split 2-D step.  can: the one-kernel form is possible; tune: see above; listed: the tile count
    // the last launch's hand-over left where it describes the launch to come (QuietTiles::list_count_current), else -1;
    // ntiles: tiles of the grid.
    Pick begin(bool can, bool tune, long listed, long ntiles) {
        Pick p = {can ? 1 : 0, tune, false};
        if (tune) {
            const long k = phase();
            if (is_gate(k)) {
                t[0] = t[1] = 1e30;
                // The gate: where the last launch ran over a list of L tiles, the next one runs over the list behind
                // it, and 4 L <= ntiles, this window has no trials and stays with one kernel.  A one-kernel step with
                // every tile active costs 1.00 ms at 4096^2 and the two passes never less than 0.48 ms there
                // (DESIGN.md 4.1a), so a listed fraction under 0.48 cannot lose; 1/4 leaves a factor of two.  L is a
                // function of the state, not of timing: the same run takes the same forms every time.  Everything
                // else -- a full launch in front, the two passes being the current form, skipping switched off, the
                // aux-carrying instantiations and decomposed blocks (no list), L above the bound -- runs the trials.
                gated = listed >= 0 && 4 * listed <= ntiles;
                if (gated) now = 1;
            }
            if (!gated && is_trial(k)) {
                p.form = trial_form(k);
                p.timed = !is_first_trial(k);
            } else {
                if (!gated && is_verdict(k)) now = t[0] < 0.98 * t[1] ? 0 : 1;
                p.form = now;
            }
        }
        was = p.form;
        return p;
    }
    // behind the step's Courant read-back; seconds is read only where p.timed
    void end(const Pick &p, double seconds) {
        n[p.form]++;
        if (p.timed && seconds < t[p.form]) t[p.form] = seconds;
        if (p.tuned) step++;
    }
    // The step to come takes the one-kernel form as a plain step of its window: not the step at which the window's form
    // is decided (the gate step, the verdict step), not a trial step.  (A step run ahead is never a decomposed block's.)
    bool next_is_plain_onek(bool can, int mode) const {
        if (!can) return false;
        if (mode != 2) return true;
        const long k = phase();
        if (is_gate(k) || (!gated && (is_trial(k) || is_verdict(k)))) return false;
        return now == 1;
    }
    // a step enqueued ahead became the step asked for: what begin() and end() do around a plain one-kernel step
    void adopted(int mode) { n[1]++; was = 1; if (mode == 2) step++; }
    void ran(int form) { n[form]++; }               // a step of the overlapped plans: counted, no part of the window
    void forget_last() { was = -1; }
    int last() const { return was; }
    void reset_counts() { n[0] = n[1] = 0; }
    const long *counts() const { return n; }        // [0] two passes, [1] one kernel

private:
    static constexpr long WINDOW = 256;
    static constexpr int TRIAL = 3;         // timed steps per form at the start of a window (the first one untimed)
    static constexpr long T0 = 64;          // the trials start 64 steps into a window: a short run never meets them

    int now = 1, was = -1;
    long step = 0, n[2] = {0, 0};
    double t[2] = {0, 0};
    bool gated = false;

    long phase() const { return step % WINDOW - T0; }
    static bool is_gate(long k) { return k == 0; }
    static bool is_trial(long k) { return k >= 0 && k < 2 * (TRIAL + 1); }      // of an ungated window
    static int trial_form(long k) { return k < TRIAL + 1 ? 1 : 0; }
    static bool is_first_trial(long k) { return k % (TRIAL + 1) == 0; }
    static bool is_verdict(long k) { return k == 2 * (TRIAL + 1); }
};

}  // namespace pcl
