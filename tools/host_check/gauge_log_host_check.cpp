// gauge_log_host_check.cpp -- the host side of the device gauge log, end to end, on a machine without a GPU: the real
// pclaw.hip (built with the sanitizer on its host code) linked against hip_shim.cpp.  Drives the C ABI the way
// pyclaw_amd/solver.py does -- arm at the entry of evolve_to_time, one record per step, undo for a rejected step, a flush
// into a buffer of exactly the size _gauge_log_flush allocates (min(capacity, accepted + 1) records), re-arm on another key,
// disarm, and both ends a handle can take: disarm then pcl_destroy (Solver._release behind a disarm) and pcl_destroy of an
// armed handle.  Kernels do not run (see hip_shim.cpp), so values are not checked here, only counts, return codes and --
// through the sanitizer -- every host access.  Exit status 0 and no sanitizer report: passed.  tools/host_check/run.sh
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/pyclaw_amd.h"

#define CHECK(call)                                                                                     \
    do {                                                                                                \
        const int rc_ = (call);                                                                         \
        if (rc_ != PCL_OK) {                                                                            \
            fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, pcl_last_error()); \
            exit(1);                                                                                    \
        }                                                                                               \
    } while (0)
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "%s:%d: expected %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

// Solver._gauge_log_flush: a heap buffer of exactly nmax records
static int flush(pcl_solver *s, int accepted, int capacity, int ncell, int per) {
    const int nmax = capacity < accepted + 1 ? capacity : accepted + 1;
    double *out = (double *)malloc(sizeof(double) * nmax * ncell * per);
    int nrec = -1;
    CHECK(pcl_gauge_log_read(s, nmax, out, &nrec));
    free(out);
    return nrec;
}

static void stats(pcl_solver *s, long want_rec, long want_pop, long want_reads) {
    long rec, pop, reads;
    CHECK(pcl_gauge_log_stats(s, &rec, &pop, &reads));
    EXPECT(rec == want_rec && pop == want_pop && reads == want_reads);
}

static void drive(const pcl_config &cfg, const std::vector<int> &ij, bool destroy_armed) {
    const int st = cfg.ndim > 2 ? 3 : 2, ncell = (int)ij.size() / st, per = cfg.meqn + cfg.maux;
    pcl_solver *s = nullptr;
    CHECK(pcl_create(&cfg, &s));
    long cells = 1, ghosted = 1;
    for (int k = 0; k < cfg.ndim; k++) cells *= cfg.n[k], ghosted *= cfg.n[k] + 2 * cfg.mbc;
    std::vector<double> q(cells * cfg.meqn, 1.0), aux(ghosted * (cfg.maux > 0 ? cfg.maux : 1), 1.0);
    CHECK(pcl_put_q(s, q.data(), 0));
    if (cfg.maux > 0) CHECK(pcl_put_aux(s, aux.data()));
    double cfl = -1.0;
    // refusals leave nothing behind
    std::vector<int> bad(ij);
    bad[0] = cfg.n[0];
    EXPECT(pcl_gauge_log(s, ncell, bad.data(), 3) == PCL_EINVAL);
    EXPECT(pcl_gauge_log(s, ncell, ij.data(), 0) == PCL_EINVAL);
    int n = -1;
    EXPECT(pcl_gauge_log_read(s, 1, q.data(), &n) == PCL_ESTATE);
    // evolve_to_time(tend) with capacity 3: ten accepted steps, one of them behind a rejected one
    const int cap = 3;
    CHECK(pcl_gauge_log(s, ncell, ij.data(), cap));
    int accepted = 0, reads = 0;
    for (int k = 0; k < 10; k++) {
        CHECK(pcl_step_hyperbolic(s, 1e-3, &cfl));
        if (k == 4) {                          // rejected: undo, retake
            CHECK(pcl_undo_step(s));
            EXPECT(pcl_undo_step(s) == PCL_ESTATE);
            CHECK(pcl_step_hyperbolic(s, 5e-4, &cfl));
        }
        if (++accepted == cap) {
            EXPECT(flush(s, accepted, cap, ncell, per) == accepted);
            accepted = 0, reads++;
        }
    }
    EXPECT(flush(s, accepted, cap, ncell, per) == accepted);
    reads++;
    stats(s, 11, 1, reads);
    // the copied backup of a run with a start_step: restore takes the record back, once
    CHECK(pcl_backup(s));
    CHECK(pcl_step_hyperbolic(s, 1e-3, &cfl));
    CHECK(pcl_restore(s));
    CHECK(pcl_restore(s));
    EXPECT(flush(s, 0, cap, ncell, per) == 0);
    // a full log refuses the step; a read that is too small reads nothing
    for (int k = 0; k < cap; k++) CHECK(pcl_step_hyperbolic(s, 1e-3, &cfl));
    EXPECT(pcl_step_hyperbolic(s, 1e-3, &cfl) == PCL_ESTATE);
    EXPECT(pcl_gauge_log_read(s, cap - 1, q.data(), &n) == PCL_EINVAL);
    EXPECT(flush(s, cap, cap, ncell, per) == cap);
    // another key: one cell, capacity 1
    CHECK(pcl_gauge_log(s, 1, ij.data(), 1));
    stats(s, 0, 0, 0);
    CHECK(pcl_step_hyperbolic(s, 1e-3, &cfl));
    EXPECT(flush(s, 1, 1, 1, per) == 1);
    // the direct path next to it
    std::vector<double> qv(ncell * cfg.meqn), av(ncell * (cfg.maux > 0 ? cfg.maux : 1));
    CHECK(pcl_get_cells(s, ncell, ij.data(), qv.data(), cfg.maux > 0 ? av.data() : nullptr));
    // disarmed: steps record nothing; disarming twice is fine
    CHECK(pcl_gauge_log(s, 0, nullptr, 0));
    CHECK(pcl_gauge_log(s, 0, nullptr, 0));
    CHECK(pcl_step_hyperbolic(s, 1e-3, &cfl));
    stats(s, 0, 0, 0);
    // armed again with a record held, then the two ends
    CHECK(pcl_gauge_log(s, ncell, ij.data(), 1024));
    CHECK(pcl_step_hyperbolic(s, 1e-3, &cfl));
    if (!destroy_armed) CHECK(pcl_gauge_log(s, 0, nullptr, 0));
    pcl_destroy(s);
}

int main() {
    pcl_config c1 = {};
    c1.ndim = 1, c1.n[0] = 50, c1.mbc = 2, c1.meqn = 1, c1.mwaves = 1, c1.maux = 0;
    c1.method[1] = 2, c1.mthlim[0] = 4, c1.rp = PCL_RP_ADVECTION_1D, c1.rp_params[0] = 1.0, c1.d[0] = 0.02;
    pcl_config c3 = {};
    c3.ndim = 3, c3.n[0] = 12, c3.n[1] = 10, c3.n[2] = 8, c3.mbc = 2, c3.meqn = 4, c3.mwaves = 2, c3.maux = 2;
    c3.method[1] = 2, c3.method[2] = -1, c3.method[6] = 2, c3.mthlim[0] = c3.mthlim[1] = 4, c3.rp = PCL_RP_VC_ACOUSTICS_3D;
    c3.d[0] = c3.d[1] = c3.d[2] = 0.1;
    for (int armed = 0; armed < 2; armed++) {
        drive(c1, {0, 0, 49, 0, 7, 0}, armed != 0);
        drive(c3, {0, 0, 0, 11, 9, 7, 5, 2, 6}, armed != 0);
    }
    // the bookkeeping alone (pcl_gauge_log_trace): arm 2, three steps, undo, step, read, disarm
    const int ev[] = {0, 1, 1, 1, 2, 1, 4, 5}, a[] = {2, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int> out(4 * 8);
    CHECK(pcl_gauge_log_trace(8, ev, a, out.data()));
    EXPECT(out[4 * 3] == -1 && out[4 * 5] == 1 && out[4 * 6] == 2);
    pcl_layer1_release();
    printf("gauge_log_host_check: ok\n");
    return 0;
}
