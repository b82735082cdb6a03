// gauge_log.hpp -- the device gauge log (pcl_gauge_log): the bookkeeping of its records (host only, no device, no clock,
// no environment: included by pclaw.hip; the scheme: DESIGN.md 4.4c; the tests: tests/test_gauge_log_cpu.py through
// pcl_gauge_log_trace).
//
// Armed, every step entry point (pcl_bc_step, pcl_step_hyperbolic) enqueues one more small kernel behind the step: it
// copies the gauge cells of the NEW state into record `slot` of a device-resident log, log[(slot * ncell + c) * per + m].
// Nothing waits for it; the host reads all records held in one copy (pcl_gauge_log_read).  Everything that touches the
// device (the two allocations, the index upload, the launch, the read-back) is pclaw.hip's; here is which slot a step
// writes, which record a rejected step takes back with it, and when the log refuses.
//
// Fields, and the only events that change them:
//   armed, ncell, per, capacity   set by arm() (pcl_gauge_log), zeroed by disarm().  per = meqn + (maux if aux was
//                 uploaded when the log was armed, else 0): the stride of a cell in a record, fixed for the log's life.
//   count         records held, 0 .. capacity.  Raised by slot_for_step(), lowered by pop(), zeroed by taken(), arm()
//                 and disarm().
//   last_recorded the last step call wrote record count - 1 and nothing has popped it.  Set by slot_for_step(); cleared
//                 by pop(), taken(), arm() and disarm().
//   n_recorded, n_popped, n_reads   totals since arm(), for pcl_gauge_log_stats.
// Invariant: a slot handed out is < capacity -- the log never writes past its end.  A full log refuses (slot_for_step()
// returns -1 and changes nothing); the step entry point asks full() before it launches anything and fails with PCL_ESTATE.
#pragma once

namespace pcl {

class GaugeLog {
public:
    void arm(int ncell_, int per_, int capacity_) {
        disarm();
        armed = true;
        ncell = ncell_, per = per_, capacity = capacity_;
    }
    void disarm() {
        armed = false, last_recorded = false;
        ncell = per = capacity = count = 0;
        n_recorded = n_popped = n_reads = 0;
    }
    bool is_armed() const { return armed; }
    bool full() const { return armed && count == capacity; }
    // the slot the step just taken writes: `count`, then one record more is held; -1 (nothing changes) when the log is
    // full or not armed
    int slot_for_step() {
        if (!armed || count == capacity) return -1;
        last_recorded = true;
        n_recorded++;
        return count++;
    }
    // pcl_undo_step / pcl_restore: a rejected step's record goes with the step.  Once per step: a second undo, or a
    // restore that follows no step, takes nothing.  true: a record was taken back
    bool pop() {
        if (!armed || !last_recorded) return false;
        count--;
        last_recorded = false;
        n_popped++;
        return true;
    }
    // behind a read of all `count` records
    void taken() {
        if (!armed) return;
        count = 0;
        last_recorded = false;
        n_reads++;
    }

    int cells() const { return ncell; }
    int stride() const { return per; }
    int room() const { return capacity; }
    int held() const { return count; }
    bool last_is_recorded() const { return last_recorded; }
    void stats(long *rec, long *pop_, long *rd) const { *rec = n_recorded; *pop_ = n_popped; *rd = n_reads; }

private:
    bool armed = false, last_recorded = false;
    int ncell = 0, per = 0, capacity = 0, count = 0;
    long n_recorded = 0, n_popped = 0, n_reads = 0;
};

// pcl_gauge_log_trace: a fresh GaugeLog driven through n events.  ev[i]: 0 arm(ncell 1, per 1, capacity a[i]); 1 a step:
// out = slot_for_step() (-1: refused); 2 undo and 3 restore: out = pop(); 4 read: out = the records held, then taken();
// 5 disarm.  out[4 i ..] = that value, count, last_recorded, armed behind the event.  Returns nullptr, or what was wrong.
inline const char *gauge_log_trace(long n, const int *ev, const int *a, int *out) {
    GaugeLog g;
    for (long i = 0; i < n; i++) {
        int v = 0;
        if (ev[i] == 0) {
            if (a[i] <= 0) return "bad capacity";
            g.arm(1, 1, a[i]);
        } else if (ev[i] == 1) v = g.slot_for_step();
        else if (ev[i] == 2 || ev[i] == 3) v = g.pop();
        else if (ev[i] == 4) { v = g.held(); g.taken(); }
        else if (ev[i] == 5) g.disarm();
        else return "bad event";
        out[4 * i] = v;
        out[4 * i + 1] = g.held();
        out[4 * i + 2] = g.last_is_recorded();
        out[4 * i + 3] = g.is_armed();
    }
    return nullptr;
}

}  // namespace pcl
