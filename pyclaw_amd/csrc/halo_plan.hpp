// halo_plan.hpp -- how a decomposed block steps beside its halo exchange: the overlap mode, the step's plan and launch
// order, and which buffers hold a filled ghost frame (host only, no device, no clock, no environment: included by
// pclaw.hip; the scheme and its measurements: DESIGN.md 5 and 7; the tests: tests/test_halo_plan_cpu.py through
// pcl_halo_plan_trace).  Everything that touches the device -- the halo stream and its events, the launches, the
// exchange itself -- is pclaw.hip's: step_overlapped runs the order chosen here, framed_x_pass the unsplit step's and
// the SharpClaw stage's.
//
// Fields, and the only events that change them:
//   ov, dflt   the mode: PCL_HALO_OVERLAP (0 the exchange in front of the step, 1 overlapped, 2 the test order: the
//              overlapped step's launches on one stream, interior tiles strictly before the exchange), and whether the
//              variable was NOT set -- then the library picks per kernel family (twopass_ok).  Set by configure()
//              (comm_ready, which reads the environment).
//   ea         exchange-ahead (pcl_halo_exchange_ahead): the halo exchange of the NEW state is enqueued on the halo
//              stream right behind the launch that produced it, so it runs through the hand-over of the Courant number,
//              the host's accept / retake decision and the first tiles of the next step instead of in front of that
//              step's rim tiles.  0 off; 1 in the two-pass step's order on the communicator (all-reduce, then the new
//              state's exchange); 2 in the one-kernel step's (the exchange behind the rim tiles, then the all-reduce).
//              Every rank of a run holds the same value.  Set by set_exchange_ahead(), which drops all marks.
//   mark[2]    the buffers whose ghost frame an exchange has filled and nothing has touched since, the newest first: the
//              state itself and, for a retaken step, the pre-step state (pcl_undo_step).  At most two are held; a null
//              buffer is never filled.  A buffer is added by exchanged() (a held one: no-op; the older of two is
//              forgotten); one is dropped by written() (a launch writes it); all are dropped by touched() (every
//              entry point that changes a state buffer or its frame from outside the overlapped step), failed() (a
//              step that returns an error), set_exchange_ahead(), and by plan() whenever its answer is not an
//              overlapped step (exchange-ahead lives in the overlapped dimension-split step only).
#pragma once

namespace pcl {

class OverlapPlan {
public:
    // What pclaw.hip knows about the block when it asks (block_facts).  active: a communicator is set up.  split2: the
    // classic dimension-split 2-D step with at most 8 equations.  sel0: the calls act on the state register.  onek_ok:
    // the block may take the one-kernel step (fused_step_ok).  onek_family: an aux-free solver of the one-kernel step,
    // no capacity function (see twopass_ok).  onek_box / x_box: the one-kernel step's / the x pass' tiles leave an
    // interior box, tiles that read no ghost cell.
    struct Facts { bool active, split2, sel0, onek_ok, onek_family, onek_box, x_box; };

    // The launch orders of an overlapped step, each spelt out where it is run (pclaw.hip: step_overlapped).
    enum Order { NOT_OVERLAPPED = 0, RIM_FIRST, EXCHANGE_IN_FRONT, TEST_ORDER, INTERIOR_FIRST };
    // onek: the one-kernel step (else x pass + y pass).  have: the state's ghost frame is already filled by an exchange
    // sent ahead -- the step neither forks the halo stream nor exchanges.  send_ahead: behind the step the new state's
    // exchange is sent ahead (the tail of TEST_ORDER and INTERIOR_FIRST; RIM_FIRST sends it inside its order).
    struct Step { Order order; bool onek, have, send_ahead; };

    void configure(int overlap, bool set) { ov = overlap; dflt = !set; }
    void set_exchange_ahead(int on) { ea = on == 2 ? 2 : on ? 1 : 0; touched(); }

    // pcl_halo_can_overlap: 0 this block cannot send its exchange ahead, 1 in the two-pass step only, 2 in the
    // one-kernel step too.  Asked before ea is set (pcl_halo_exchange_ahead, ClawSolver._decide_exchange_ahead), so it
    // is form() with nothing agreed yet; only mode 1 sends an exchange ahead (plan: send_ahead), and the register the
    // calls act on at the moment is no property of the block.
    int offers(const Facts &f) const { return f.active && f.split2 && ov == 1 ? form(f, true, false) : 0; }

    // pcl_bc_step: the plan of this step, q the state buffer.  Under ea == 1 the ranks have agreed on the two-pass
    // order because some block is too thin for one-kernel tiles: this rank keeps that order too, and keeps the
    // overlap where the default alone would put the exchange in front (every rank issues the same sequence on the
    // communicator).  The test order (ov == 2) plans like mode 1 and sends nothing ahead.
    Step plan(const Facts &f, const double *q) {
        const int k = f.active && f.split2 && ov != 0 && f.sel0 ? form(f, ea != 1, ea == 1) : 0;
        if (!k) {
            touched();
            return Step{NOT_OVERLAPPED, false, false, false};
        }
        const bool onek = k == 2, have = ea != 0 && filled(q);
        const Order o = onek && ov == 1 && have          ? RIM_FIRST
                        : onek && ov == 1 && ea == 0     ? EXCHANGE_IN_FRONT
                        : ov == 2                        ? TEST_ORDER
                                                         : INTERIOR_FIRST;
        return Step{o, onek, have, ea != 0 && ov == 1};
    }

    // the unsplit 2-D step builds its ghost frame beside the interior tiles of its x phase: only where the mode is set
    // explicitly (by default the exchange in front measures faster)
    bool unsplit_overlaps(bool active) const { return active && ov != 0 && !dflt; }
    // a SharpClaw stage does the same for its x pass: in every mode but 0, 2-D only
    bool sharp_overlaps(bool active, int ndim) const { return active && ov != 0 && ndim == 2; }
    // framed_x_pass: frame and tiles on the solver stream, in order -- nothing overlaps, or the test order
    bool frame_sequential(bool overlapping) const { return !overlapping || ov == 2; }

    bool filled(const double *buf) const { return buf && (mark[0] == buf || mark[1] == buf); }
    void exchanged(const double *buf) { if (!filled(buf)) { mark[1] = mark[0]; mark[0] = buf; } }
    void written(const double *buf) { for (auto &m : mark) if (m == buf) m = nullptr; }
    void touched() { mark[0] = mark[1] = nullptr; }
    void failed() { touched(); }

private:
    // The one statement of "may this block overlap, and in which form": 2 the one-kernel step over interior / rim tile
    // subsets, 1 the two passes with the interior x tiles beside the exchange, 0 neither.  onek: the one-kernel form
    // is open to this step; agreed2: the run has agreed on the two-pass order (ea == 1).
    int form(const Facts &f, bool onek, bool agreed2) const {
        if (onek && f.onek_ok && f.onek_box) return 2;
        return (twopass_ok(f) || agreed2) && f.x_box ? 1 : 0;
    }
    // The two-pass step with its interior x tiles BESIDE the exchange.  For the solver family of the one-kernel step
    // (aux-free, no capacity function: an x pass register-allocated for four workgroups per CU) the interior launch
    // starves the halo stream's pack / Send-Recv kernels (44 / 77 us instead of 6 / 34) and the step is slower than
    // with the exchange in front (4096 x 2048 Euler block: 0.489 against 0.320 ms), so those blocks -- too thin for
    // one-kernel tiles, mbc > 2, PCL_TUNE_FUSED_STEP=0 -- take the exchange in front unless PCL_HALO_OVERLAP=1 is set
    // explicitly (tests, A/B).  Solvers with aux arrays or a capacity function keep the overlap (their decomposed
    // blocks never take the one-kernel step: fused_step_ok).
    bool twopass_ok(const Facts &f) const { return !(f.onek_family && dflt); }

    int ov = 1, ea = 0;
    bool dflt = true;
    const double *mark[2] = {nullptr, nullptr};
};

// One OverlapPlan driven through n scripted events (pcl_halo_plan_trace, include/pyclaw_amd.h: the events and the
// encoding of out[]).  Returns null, or what is wrong with the script.
inline const char *overlap_plan_trace(long n, const int *event, const int *a, const int *b, int *out) {
    static const double bufs[8] = {};       // buffer id 1..7: a distinct address, 0: the null buffer
    OverlapPlan p;
    for (long i = 0; i < n; i++) {
        const int e = event[i], x = a[i], y = b[i];
        const bool has_buf = e >= 3 && e <= 6;      // a plan's state buffer is b[i], a mark event's a[i]
        const int id = e == 3 ? y : x;
        if (has_buf && (id < 0 || id > 7)) return "bad buffer id";
        const double *buf = has_buf && id > 0 ? bufs + id : nullptr;
        const OverlapPlan::Facts f{(x & 1) != 0, (x & 2) != 0, (x & 4) != 0, (x & 8) != 0, (x & 16) != 0, (x & 32) != 0, (x & 64) != 0};
        out[i] = 0;
        if (e == 0) p.configure(x, y != 0);
        else if (e == 1) p.set_exchange_ahead(x);
        else if (e == 2) out[i] = p.offers(f);
        else if (e == 3) {
            const OverlapPlan::Step st = p.plan(f, buf);
            out[i] = (int)st.order | (st.onek ? 8 : 0) | (st.have ? 16 : 0) | (st.send_ahead ? 32 : 0);
        } else if (e == 4) out[i] = p.filled(buf);
        else if (e == 5) p.exchanged(buf);
        else if (e == 6) p.written(buf);
        else if (e == 7) p.touched();
        else if (e == 8) p.failed();
        else if (e == 9) out[i] = p.unsplit_overlaps(x != 0);
        else if (e == 10) out[i] = p.sharp_overlaps(x != 0, y);
        else if (e == 11) out[i] = p.frame_sequential(x != 0);
        else return "bad event";
    }
    return nullptr;
}

}  // namespace pcl
