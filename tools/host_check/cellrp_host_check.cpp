// cellrp_host_check.cpp -- the host side of the user-written Riemann solvers (csrc/cellrp.hpp, pcl_cellrp_*) on a machine
// without a GPU: the real pclaw.hip (built with the sanitizer on its host code) linked against hip_shim.cpp.  The compile
// is real (libhiprtc needs no device): program text, named headers, name expressions, lowered names and the shared cache
// all run under the sanitizer.  The shim loads no module, so pcl_cellrp_attach ends in PCL_EHIP behind its host-only
// checks and a PCL_RP_CELL handle stays without a solver: every step is refused, which is the path checked here.
// The second half does the same for solvers that read aux (pcl_cellrp_compile_aux, pcl_cellrp_aux): the list in the
// cache key, every refusal of a list, and attach against a solver whose maux does not reach it.
// The third half is the form (pcl_cellrp_compile_form, pcl_cellrp_form): a compile per form, hit and miss on the form, form 0
// as pcl_cellrp_compile_t's entry, the refusals with the compile count unmoved, pcl_create_cellrp against every pair of
// handle and configuration, and attach of a handle of another form.
// The last part is the one-kernel step (pcl_cellrp_compile_onek, pcl_cellrp_onek): its refusals, its own cache entry, five
// kernels in one program, and attach as far as the module load.
// Exit status 0 and no sanitizer report: passed.  tools/host_check/run.sh
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
#define EXPECT(cond)                                                                                   \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            fprintf(stderr, "%s:%d: expected %s (%s)\n", __FILE__, __LINE__, #cond, pcl_last_error()); \
            exit(1);                                                                                   \
        }                                                                                              \
    } while (0)

static const char *kBurgers =
    "wave[0][0] = qr[0] - ql[0];\n"
    "s[0] = 0.5 * (ql[0] + qr[0]);\n"
    "const bool transonic = qr[0] > 0.0 && ql[0] < 0.0;\n"
    "amdq[0] = transonic ? -0.5 * (ql[0] * ql[0]) : dmin(s[0], 0.0) * wave[0][0];\n"
    "apdq[0] = transonic ? 0.5 * (qr[0] * qr[0]) : dmax(s[0], 0.0) * wave[0][0];\n";

int main() {
    long n0 = 0, h0 = 0, n = 0, h = 0, size = 0;
    CHECK(pcl_cellfn_stats(&n0, &h0));
    pcl_cellrp *a = nullptr, *b = nullptr, *c = nullptr, *bad = nullptr;
    // refusals in front of the compile
    EXPECT(pcl_cellrp_compile(kBurgers, "", 0, 1, 2, PCL_MATH_EXACT, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(pcl_cellrp_compile(kBurgers, "", 1, 9, 2, PCL_MATH_EXACT, &bad, nullptr) == PCL_EINVAL);
    EXPECT(pcl_cellrp_compile(kBurgers, "", 1, 1, 3, PCL_MATH_EXACT, &bad, nullptr) == PCL_EINVAL);
    EXPECT(pcl_cellrp_compile(nullptr, "", 1, 1, 2, PCL_MATH_EXACT, &bad, nullptr) == PCL_EINVAL);
    // two passes in 2-D, one kernel in 1-D; a null preamble; the cache
    CHECK(pcl_cellrp_compile(kBurgers, nullptr, 1, 1, 2, PCL_MATH_EXACT, &a, &size));
    EXPECT(a && size > 0);
    CHECK(pcl_cellrp_compile(kBurgers, "", 1, 1, 2, PCL_MATH_EXACT, &b, nullptr));
    EXPECT(b == a);
    CHECK(pcl_cellrp_compile(kBurgers, "__device__ inline double twice(double v) { return 2.0 * v; }\n", 1, 1, 1, PCL_MATH_FAST, &c, nullptr));
    EXPECT(c && c != a);
    CHECK(pcl_cellfn_stats(&n, &h));
    EXPECT(n == n0 + 2 && h == h0 + 1);
    // a body that does not compile: the log names the line, nothing is cached
    EXPECT(pcl_cellrp_compile("s[0] = 1.0;\ns[0] = nothing;\n", "", 1, 1, 1, PCL_MATH_EXACT, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "riemann:2") != nullptr);
    CHECK(pcl_cellfn_stats(&n, &h));
    EXPECT(n == n0 + 2 && h == h0 + 1);
    // the handle's constants
    CHECK(pcl_cellrp_check(a, 1, 1, 2, PCL_MATH_EXACT));
    EXPECT(pcl_cellrp_check(a, 2, 1, 2, PCL_MATH_EXACT) == PCL_EINVAL);
    EXPECT(pcl_cellrp_check(a, 1, 1, 2, PCL_MATH_FAST) == PCL_EINVAL);
    EXPECT(pcl_cellrp_check(nullptr, 1, 1, 2, PCL_MATH_EXACT) == PCL_EINVAL);

    // a PCL_RP_CELL solver handle
    pcl_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.ndim = 2; cfg.n[0] = 70; cfg.n[1] = 9; cfg.mbc = 3; cfg.meqn = 1; cfg.mwaves = 1;
    cfg.method[0] = 1; cfg.method[1] = 2; cfg.method[2] = -1;
    cfg.mthlim[0] = 4; cfg.rp = PCL_RP_CELL; cfg.d[0] = cfg.d[1] = 0.1; cfg.math = PCL_MATH_EXACT;
    pcl_solver *s = nullptr;
    pcl_config wrong = cfg;
    wrong.fwave = 1;
    EXPECT(pcl_create(&wrong, &s) == PCL_EINVAL && !s);
    wrong = cfg;
    wrong.method[2] = 1;
    EXPECT(pcl_create(&wrong, &s) == PCL_EINVAL && !s);
    CHECK(pcl_create(&cfg, &s));
    int info[10];
    EXPECT(pcl_rp_info(PCL_RP_CELL, info) == PCL_EINVAL);
    std::vector<double> q((size_t)cfg.n[0] * cfg.n[1], 1.0);
    CHECK(pcl_put_q(s, q.data(), 0));
    double cfl = -1.0;
    EXPECT(pcl_step_hyperbolic(s, 0.01, &cfl) == PCL_ESTATE);
    EXPECT(pcl_sweep(s, 2, 0.01, &cfl) == PCL_ESTATE);
    EXPECT(pcl_cellrp_attach(s, c) == PCL_EINVAL);          // compiled for 1-D, fast
    EXPECT(pcl_cellrp_attach(s, nullptr) == PCL_EINVAL);
    EXPECT(pcl_cellrp_attach(s, a) == PCL_EHIP);            // host checks passed; the shim loads no module
    EXPECT(pcl_step_hyperbolic(s, 0.01, &cfl) == PCL_ESTATE);
    const double p9[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    EXPECT(pcl_cellrp_params(s, p9, 9) == PCL_EINVAL);
    CHECK(pcl_cellrp_params(s, p9, 8));
    CHECK(pcl_cellrp_params(s, nullptr, 0));
    const int nbr[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    char uid[128] = {0};
    EXPECT(pcl_comm_init(s, 1, 0, uid, nbr) == PCL_EINVAL);
    pcl_destroy(s);

    // references: two for a (compiled twice), one for c
    CHECK(pcl_cellrp_release(a));
    CHECK(pcl_cellrp_release(b));
    EXPECT(pcl_cellrp_release(a) == PCL_EINVAL);
    CHECK(pcl_cellrp_release(c));
    CHECK(pcl_cellrp_release(nullptr));
    CHECK(pcl_cellrp_compile(kBurgers, "", 1, 1, 2, PCL_MATH_EXACT, &b, nullptr));      // released, not forgotten
    EXPECT(b == a);

    // ---- solvers that read aux: pcl_cellrp_compile_aux, pcl_cellrp_aux ----
    static const char *kVcAdvection =
        "const double vel = ixy == 1 ? auxr[0] : auxr[1];\n"
        "wave[0][0] = qr[0] - ql[0];\n"
        "s[0] = vel;\n"
        "amdq[0] = dmin(vel, 0.0) * wave[0][0];\n"
        "apdq[0] = dmax(vel, 0.0) * wave[0][0];\n";
    pcl_cellrp *x01 = nullptr, *x01b = nullptr, *x10 = nullptr, *x31 = nullptr, *plain = nullptr;
    const int l01[2] = {0, 1}, l10[2] = {1, 0}, l31[2] = {3, 1}, neg[2] = {0, -1}, twice[3] = {2, 0, 2};
    const int many[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    CHECK(pcl_cellfn_stats(&n0, &h0));
    // every new refusal, in front of the compiler
    EXPECT(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, l01, -1, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, nullptr, 2, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, neg, 2, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "negative") != nullptr);
    EXPECT(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, twice, 3, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "twice") != nullptr);
    EXPECT(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, many, 8, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "meqn + naux = 9") != nullptr && strstr(pcl_last_error(), "at most 8 planes") != nullptr);
    EXPECT(pcl_cellrp_compile_aux(kVcAdvection, "", 3, 1, 2, PCL_MATH_EXACT, many, 6, &bad, nullptr) == PCL_EINVAL && !bad);
    CHECK(pcl_cellfn_stats(&n, &h));
    EXPECT(n == n0 && h == h0);
    // compile with a list; hit and miss on the list and on its order; the list comes back
    CHECK(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, l01, 2, &x01, &size));
    EXPECT(x01 && size > 0);
    CHECK(pcl_cellrp_compile_aux(kVcAdvection, nullptr, 1, 1, 2, PCL_MATH_EXACT, l01, 2, &x01b, nullptr));
    EXPECT(x01b == x01);
    CHECK(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, l10, 2, &x10, nullptr));
    CHECK(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_STRICT, l31, 2, &x31, nullptr));
    EXPECT(x10 && x31 && x10 != x01 && x31 != x01 && x31 != x10);
    CHECK(pcl_cellfn_stats(&n, &h));
    EXPECT(n == n0 + 3 && h == h0 + 1);
    int naux = -1, list[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    CHECK(pcl_cellrp_aux(x31, &naux, list));
    EXPECT(naux == 2 && list[0] == 3 && list[1] == 1 && list[2] == -1);
    CHECK(pcl_cellrp_aux(x10, &naux, nullptr));
    EXPECT(naux == 2);
    EXPECT(pcl_cellrp_aux(nullptr, &naux, list) == PCL_EINVAL);
    EXPECT(pcl_cellrp_aux(x01, nullptr, list) == PCL_EINVAL);
    // an empty list is pcl_cellrp_compile: the handle of the plain compile of this text
    CHECK(pcl_cellrp_compile_aux(kBurgers, "", 1, 1, 2, PCL_MATH_EXACT, nullptr, 0, &plain, nullptr));
    EXPECT(plain == a);
    CHECK(pcl_cellrp_aux(plain, &naux, list));
    EXPECT(naux == 0 && list[0] == 3);
    // a body that names auxl without a list does not compile
    EXPECT(pcl_cellrp_compile("s[0] = 1.0;\ns[0] = auxl[0];\n", "", 1, 1, 1, PCL_MATH_EXACT, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "riemann:2") != nullptr);
    CHECK(pcl_cellrp_check(x01, 1, 1, 2, PCL_MATH_EXACT));
    EXPECT(pcl_cellrp_check(x31, 1, 1, 2, PCL_MATH_EXACT) == PCL_EINVAL);

    // a PCL_RP_CELL handle with two aux components
    cfg.maux = 2;
    cfg.method[6] = 2;
    pcl_config capa = cfg;
    capa.method[5] = 1;
    EXPECT(pcl_create(&capa, &s) == PCL_EINVAL);            // a capacity function is still refused
    s = nullptr;
    CHECK(pcl_create(&cfg, &s));
    CHECK(pcl_put_q(s, q.data(), 0));
    const size_t ncell = (size_t)(cfg.n[0] + 2 * cfg.mbc) * (cfg.n[1] + 2 * cfg.mbc);
    std::vector<double> aux(2 * ncell, 0.5);
    EXPECT(pcl_cellrp_attach(s, x31) == PCL_EINVAL);        // math strict, and component 3 of 2
    pcl_cellrp *y31 = nullptr;
    CHECK(pcl_cellrp_compile_aux(kVcAdvection, "", 1, 1, 2, PCL_MATH_EXACT, l31, 2, &y31, nullptr));
    EXPECT(pcl_cellrp_attach(s, y31) == PCL_EINVAL);        // maux too small: refused before the module load
    EXPECT(strstr(pcl_last_error(), "aux component 3") != nullptr && strstr(pcl_last_error(), "maux = 2") != nullptr);
    EXPECT(pcl_step_hyperbolic(s, 0.01, &cfl) == PCL_ESTATE);
    CHECK(pcl_put_aux(s, aux.data()));
    EXPECT(pcl_cellrp_attach(s, x10) == PCL_EHIP);          // host checks passed; the shim loads no module
    EXPECT(pcl_step_hyperbolic(s, 0.01, &cfl) == PCL_ESTATE);
    EXPECT(pcl_sweep(s, 1, 0.01, &cfl) == PCL_ESTATE);
    EXPECT(pcl_comm_init(s, 1, 0, uid, nbr) == PCL_EINVAL);
    pcl_destroy(s);
    CHECK(pcl_cellrp_release(x01));
    CHECK(pcl_cellrp_release(x01b));
    EXPECT(pcl_cellrp_release(x01) == PCL_EINVAL);
    CHECK(pcl_cellrp_release(x10));
    CHECK(pcl_cellrp_release(x31));
    CHECK(pcl_cellrp_release(y31));
    CHECK(pcl_cellrp_release(plain));

    // ---- the form of a solver: pcl_cellrp_compile_form, pcl_cellrp_form ----
    // (a body that assigns neither wave nor fwave compiles in every form)
    static const char *kSpeeds = "s[0] = -p[2]; s[1] = p[2];\n";
    static const char *kNoTrans = "";
    const int FW = PCL_CELLRP_FORM_FWAVE, CA = PCL_CELLRP_FORM_CAPA;
    pcl_cellrp *f[4] = {nullptr, nullptr, nullptr, nullptr}, *again = nullptr, *viat = nullptr;
    CHECK(pcl_cellfn_stats(&n0, &h0));
    // the refusals, in front of the compiler: an unknown bit, and one plane too many with the capacity function's
    EXPECT(pcl_cellrp_compile_form(kSpeeds, kNoTrans, "", 3, 2, 2, PCL_MATH_EXACT, nullptr, 0, 4, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "form = 4") != nullptr);
    EXPECT(pcl_cellrp_compile_form(kSpeeds, kNoTrans, "", 3, 2, 2, PCL_MATH_EXACT, nullptr, 0, -1, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(pcl_cellrp_compile_form(kSpeeds, nullptr, "", 3, 2, 2, PCL_MATH_EXACT, many, 5, CA, &bad, nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "meqn + 1 + naux = 9") != nullptr && strstr(pcl_last_error(), "at most 8 planes") != nullptr);
    CHECK(pcl_cellfn_stats(&n, &h));
    EXPECT(n == n0 && h == h0);
    // form 0 is pcl_cellrp_compile_t: one entry, whichever door
    CHECK(pcl_cellrp_compile_t(kSpeeds, kNoTrans, "", 3, 2, 2, PCL_MATH_EXACT, nullptr, 0, &viat, &size));
    long size0 = 0;
    CHECK(pcl_cellrp_compile_form(kSpeeds, kNoTrans, nullptr, 3, 2, 2, PCL_MATH_EXACT, nullptr, 0, 0, &f[0], &size0));
    EXPECT(f[0] == viat && size0 == size);
    CHECK(pcl_cellfn_stats(&n, &h));
    EXPECT(n == n0 + 1 && h == h0 + 1);
    // every other form is a program of its own; hit and miss on the form; the form comes back
    for (int form = 1; form < 4; form++) {
        CHECK(pcl_cellrp_compile_form(kSpeeds, kNoTrans, "", 3, 2, 2, PCL_MATH_EXACT, nullptr, 0, form, &f[form], &size));
        EXPECT(f[form] && size > 0);
        for (int k = 0; k < form; k++) EXPECT(f[form] != f[k]);
    }
    CHECK(pcl_cellrp_compile_form(kSpeeds, kNoTrans, "", 3, 2, 2, PCL_MATH_EXACT, nullptr, 0, FW | CA, &again, nullptr));
    EXPECT(again == f[FW | CA]);
    CHECK(pcl_cellfn_stats(&n, &h));
    EXPECT(n == n0 + 4 && h == h0 + 2);
    for (int form = 0; form < 4; form++) {
        int got = -1;
        CHECK(pcl_cellrp_form(f[form], &got));
        EXPECT(got == form);
    }
    int got = -1;
    EXPECT(pcl_cellrp_form(nullptr, &got) == PCL_EINVAL);
    EXPECT(pcl_cellrp_form(f[0], nullptr) == PCL_EINVAL);
    // an f-wave body assigns fwave; one that assigns wave does not compile, and its line is named
    EXPECT(pcl_cellrp_compile_form("s[0] = 1.0;\nwave[0][0] = qr[0] - ql[0];\n", nullptr, "", 1, 1, 1, PCL_MATH_EXACT, nullptr, 0, FW, &bad,
                                   nullptr) == PCL_EINVAL && !bad);
    EXPECT(strstr(pcl_last_error(), "riemann:2") != nullptr);
    pcl_cellrp *fw1 = nullptr;
    CHECK(pcl_cellrp_compile_form("s[0] = 1.0;\nfwave[0][0] = qr[0] - ql[0];\napdq[0] = fwave[0][0];\n", nullptr, "", 1, 1, 1, PCL_MATH_EXACT,
                                  nullptr, 0, FW, &fw1, nullptr));

    // pcl_create_cellrp against matching and mismatching handles, dimension-split and unsplit: a match passes every host
    // check and reaches the shim's module load (PCL_EHIP), every mismatch is PCL_EINVAL in front of the device
    pcl_config fc;
    memset(&fc, 0, sizeof fc);
    fc.ndim = 2; fc.n[0] = 9; fc.n[1] = 7; fc.mbc = 2; fc.meqn = 3; fc.mwaves = 2; fc.maux = 2;
    fc.method[0] = 1; fc.method[1] = 2; fc.method[6] = 2;
    fc.mthlim[0] = fc.mthlim[1] = 4; fc.rp = PCL_RP_CELL; fc.d[0] = fc.d[1] = 0.1; fc.math = PCL_MATH_EXACT;
    for (int unsplit = 0; unsplit < 2; unsplit++)
        for (int want = 0; want < 4; want++)
            for (int have = 0; have < 4; have++) {
                pcl_config k = fc;
                k.method[2] = unsplit ? 2 : -1;
                k.fwave = (want & FW) ? 1 : 0;
                k.method[5] = (want & CA) ? 2 : 0;
                s = nullptr;
                const int rc = pcl_create_cellrp(&k, f[have], &s);
                EXPECT(!s);
                if (have == want) EXPECT(rc == PCL_EHIP);
                else {
                    EXPECT(rc == PCL_EINVAL && strstr(pcl_last_error(), "PCL_RP_CELL") != nullptr);
                    EXPECT(strstr(pcl_last_error(), ((have ^ want) & FW) ? "f-waves" : "capacity function") != nullptr);
                }
                if (want) EXPECT(pcl_create(&k, &s) == PCL_EINVAL && !s);      // pcl_create cannot know a handle
            }
    {   // mcapa stays within maux
        pcl_config k = fc;
        k.method[2] = -1; k.method[5] = 3;
        EXPECT(pcl_create_cellrp(&k, f[CA], &s) == PCL_EINVAL && !s);
    }
    // attach on a solver made by pcl_create (wave form, no capacity function): a handle of another form is refused in front
    // of the module load, one of its own form gets as far as the load; the steps stay refused; release, destroy
    fc.method[2] = -1;
    s = nullptr;
    CHECK(pcl_create(&fc, &s));
    for (int form = 1; form < 4; form++) {
        EXPECT(pcl_cellrp_attach(s, f[form]) == PCL_EINVAL);
        EXPECT(strstr(pcl_last_error(), "PCL_RP_CELL") != nullptr);
    }
    EXPECT(pcl_cellrp_attach(s, f[0]) == PCL_EHIP);
    EXPECT(pcl_step_hyperbolic(s, 0.01, &cfl) == PCL_ESTATE);
    pcl_destroy(s);
    for (int form = 0; form < 4; form++) CHECK(pcl_cellrp_release(f[form]));
    CHECK(pcl_cellrp_release(viat));
    CHECK(pcl_cellrp_release(again));
    CHECK(pcl_cellrp_release(fw1));
    EXPECT(pcl_cellrp_release(fw1) == PCL_EINVAL);

    // ---- the one-kernel step: pcl_cellrp_compile_onek, pcl_cellrp_onek ----
    {
        pcl_cellrp *plain = nullptr, *one = nullptr, *one2 = nullptr, *five = nullptr;
        long psize = 0, osize = 0;
        int has = -1;
        CHECK(pcl_cellfn_stats(&n0, &h0));
        // refused in front of the compiler: more than five equations, a form bit, a null body
        EXPECT(pcl_cellrp_compile_onek(kBurgers, nullptr, "", 6, 1, PCL_MATH_EXACT, nullptr, 0, 0, &bad, nullptr) == PCL_EINVAL && !bad);
        EXPECT(strstr(pcl_last_error(), "meqn > 5") != nullptr);
        EXPECT(pcl_cellrp_compile_onek(kBurgers, nullptr, "", 1, 1, PCL_MATH_EXACT, nullptr, 0, 4, &bad, nullptr) == PCL_EINVAL);
        EXPECT(pcl_cellrp_compile_onek(nullptr, nullptr, "", 1, 1, PCL_MATH_EXACT, nullptr, 0, 0, &bad, nullptr) == PCL_EINVAL);
        CHECK(pcl_cellfn_stats(&n, &h));
        EXPECT(n == n0 && h == h0);
        // another entry than the same text without the kernel, a larger code object; again: a hit
        CHECK(pcl_cellrp_compile(kBurgers, "// onek\n", 1, 1, 2, PCL_MATH_EXACT, &plain, &psize));
        CHECK(pcl_cellrp_compile_onek(kBurgers, nullptr, "// onek\n", 1, 1, PCL_MATH_EXACT, nullptr, 0, 0, &one, &osize));
        EXPECT(one && one != plain && osize > psize);
        CHECK(pcl_cellrp_compile_onek(kBurgers, nullptr, "// onek\n", 1, 1, PCL_MATH_EXACT, nullptr, 0, 0, &one2, nullptr));
        EXPECT(one2 == one);
        CHECK(pcl_cellfn_stats(&n, &h));
        EXPECT(n == n0 + 2 && h == h0 + 1);
        CHECK(pcl_cellrp_onek(one, &has));
        EXPECT(has == 1);
        CHECK(pcl_cellrp_onek(plain, &has));
        EXPECT(has == 0);
        EXPECT(pcl_cellrp_onek(nullptr, &has) == PCL_EINVAL && pcl_cellrp_onek(one, nullptr) == PCL_EINVAL);
        // five kernels: the sweeps, the unsplit phases and the one-kernel step, in the f-wave form with a capacity function
        CHECK(pcl_cellrp_compile_onek("s[0] = p[0];\n", "", "", 5, 2, PCL_MATH_STRICT, nullptr, 0, 3, &five, nullptr));
        CHECK(pcl_cellrp_onek(five, &has));
        EXPECT(has == 1);
        // attach: the host checks pass, the shim loads no module; the step stays refused
        pcl_config k = cfg;
        k.mbc = 2;
        s = nullptr;
        CHECK(pcl_create(&k, &s));
        EXPECT(pcl_cellrp_attach(s, one) == PCL_EHIP);
        EXPECT(pcl_step_hyperbolic(s, 0.01, &cfl) == PCL_ESTATE);
        pcl_destroy(s);
        CHECK(pcl_cellrp_release(plain));
        CHECK(pcl_cellrp_release(one));
        CHECK(pcl_cellrp_release(one2));
        CHECK(pcl_cellrp_release(five));
    }
    printf("cellrp_host_check: ok\n");
    return 0;
}
