// step_ahead.hpp -- step ahead (pcl_step_ahead): the decisions and the counters (host only, no device, no clock, no
// environment: included by pclaw.hip; the scheme: DESIGN.md 4.1a; the tests: tests/test_step_ahead_cpu.py through
// pcl_step_ahead_trace).  Also BcSpec, the boundary spec of one pcl_bc_step call as the host keeps it.
//
// Armed, pcl_bc_step enqueues the step after the one it was asked for before it returns, with the dt the caller's rule
// gives (next_dt) and the boundary spec of this call: q -> t2 and its hand-over, q and t2 NOT swapped, no counter
// advanced.  The next pcl_bc_step adopts it if it asks for exactly that step (matches: the same dt bits, the same spec,
// nothing but read-only calls in between) -- then it only waits for it -- and drops it otherwise: a finished kernel
// whose output nobody uses.  Everything that touches the device or other solver state (the launch, the hand-over and
// its poll, commit_step, undo_slot, QuietTiles::drop / adopted) is pclaw.hip's: ahead_enqueue, ahead_adopt, ahead_drop.
//
// Fields, and the only events that change them:
//   armed, rule, cfl_desired, cfl_max, dt_max   the caller's rule.  Set by arm() (pcl_step_ahead, behind the drop).
//   pending       a step is enqueued ahead.  Set by enqueued(); cleared by adopted() and dropped().
//   dt, seq, spec of the pending step: its dt, the sequence number of its hand-over, its boundary spec.  Set by enqueued().
//   miss, pause   a pending step that was not the one asked for, although nothing came in between, cost a launch for
//                 nothing: the next `pause` steps are not run ahead of, twice as many after every such miss in a row
//                 (1, 2, 4 .. 64).  miss: raised by missed(), zeroed by adopted() and arm().  pause: set by missed(),
//                 zeroed by arm(), counted down by wants() -- only by a call that every earlier check let pass.
//   asked_ran     tiles the last step the caller asked for was dispatched for (host word [2] of its hand-over, read
//                 before the pending hand-over overwrites it).  Set by enqueued().
//   report        the same once the pending step is dropped, for pcl_tile_skip_stats (the dropped launch took the
//                 device's record of it along); -1: nothing to report.  Set by dropped(); cleared by forget_report()
//                 (the step entry points).
//   n_enqueued, n_adopted, n_dropped   pcl_step_ahead_stats.  Bumped by the events of those names.
#pragma once
#include <cstring>

#include "../../include/pyclaw_amd.h"

namespace pcl {

// Boundary types of up to four sides and the constant states of the PCL_BC_CUSTOM ones, as pcl_bc_step takes them.
// One builder; sides at or beyond nsides get -1, constants are zero except on custom sides, so two specs are the same
// request iff they are the same bytes (-0.0 differs from 0.0, a NaN equals itself).
struct BcSpec {
    int t[4];
    double c[4][PCL_MAX_RP_PARAMS];
    BcSpec() : BcSpec(nullptr, nullptr, 0) {}
    BcSpec(const int *bc, const double *cstate, int nsides) {
        for (int k = 0; k < 4; k++) {
            t[k] = k < nsides ? bc[k] : -1;
            for (int m = 0; m < PCL_MAX_RP_PARAMS; m++)
                c[k][m] = (t[k] == PCL_BC_CUSTOM) ? cstate[k * PCL_MAX_RP_PARAMS + m] : 0.0;
        }
    }
    bool operator==(const BcSpec &o) const { return memcmp(this, &o, sizeof(BcSpec)) == 0; }
};
static_assert(sizeof(BcSpec) == 4 * sizeof(int) + 4 * PCL_MAX_RP_PARAMS * sizeof(double), "BcSpec has padding: compared bytewise");

class StepAhead {
public:
    // on = 0 off, 1 the rule of pcl_step_ahead_dt (a pure host function of the library), 2 the same dt again
    void arm(int on, double cfl_desired_, double cfl_max_, double dt_max_) {
        armed = on != 0;
        rule = on == 2 ? 2 : 1;
        miss = pause = 0;
        cfl_desired = cfl_desired_, cfl_max = cfl_max_, dt_max = dt_max_;
    }
    // Behind a step that read the Courant number c and ran over `ran` of the grid's `ntiles` tiles: run ahead of the
    // next one?  (The checks on solver state come first, in pclaw.hip: ahead_enqueue.)
    bool wants(double c, long ran, long ntiles, bool next_plain_onek) {
        // (a NaN fails both comparisons; an infinite c is not below cfl_max)
        if (!armed || !(c > 0.0 && c < cfl_max) || !next_plain_onek) return false;
        if (pause > 0) { pause--; return false; }
        // Short launches only: the step ahead saves one host turn-round (about 10 us) per step and costs one launch for
        // nothing whenever the caller turns out to want something else, the last step of a run included.  The launch to
        // come runs over about as many tiles as the one just run: at most a quarter of the grid (the bound of the form
        // gate, step_form.hpp) or 4096 tiles, four rounds of the 1024 workgroups the chip holds at a time.
        return !(ran > 4096 && 4 * ran > ntiles);
    }
    double next_dt(double dt_, double c) const { return rule == 2 ? dt_ : pcl_step_ahead_dt(dt_, c, cfl_desired, dt_max); }
    // that step and its hand-over (sequence number seq_) are enqueued
    void enqueued(double dt_, unsigned long long seq_, const BcSpec &spec_, long ran) {
        dt = dt_, seq = seq_, spec = spec_, asked_ran = ran;
        pending = true;
        n_enqueued++;
    }
    // the caller asks for exactly the pending step: the same dt bits, the same boundary spec, nothing in between
    bool matches(const BcSpec &spec_, double dt_, bool carry) const {
        return armed && carry && memcmp(&dt_, &dt, sizeof(double)) == 0 && spec_ == spec;
    }
    // it did not, although nothing came in between: the caller's rule is not the one it armed with
    void missed() {
        if (!armed) return;
        miss = miss < 7 ? miss + 1 : 7;
        pause = 1 << (miss - 1);
    }
    void adopted() { pending = false; miss = 0; n_adopted++; }
    // true: a step was pending and is no more (the caller has QuietTiles forget it)
    bool dropped() {
        if (!pending) return false;
        pending = false;
        report = asked_ran;
        n_dropped++;
        return true;
    }
    void forget_report() { report = -1; }

    bool is_pending() const { return pending; }
    unsigned long long pending_seq() const { return seq; }
    long reported() const { return report; }
    void stats(long *enq, long *ado, long *dro) const { *enq = n_enqueued; *ado = n_adopted; *dro = n_dropped; }

private:
    bool armed = false, pending = false;
    int rule = 1, miss = 0, pause = 0;
    double cfl_desired = 0.0, cfl_max = 0.0, dt_max = 0.0, dt = 0.0;
    unsigned long long seq = 0;
    BcSpec spec;
    long n_enqueued = 0, n_adopted = 0, n_dropped = 0;
    long asked_ran = -1, report = -1;
};

}  // namespace pcl
