/*
 * oracle/classic_oracle.c  --  TEST INFRASTRUCTURE ONLY (the parity oracle).
 *
 * A plain-C, scalar, CPU restatement of the reference's classic (Clawpack)
 * wave-propagation path.  It exists so that tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg can check / time the HIP product against
 * it.  Nothing under pyclaw_amd/ may import, link or call this file.
 *
 * Every function keeps the reference's floating-point operation ORDER so the
 * result is bit-identical to the flang/gfortran build of the reference
 * Fortran (compile with -O2 -ffp-contract=off; checked against oracle/_ref
 * by tests/test_oracle_vs_ref.py and against the reference's golden files
 * test/sb_density, test/acoustics2D_solution by tests/test_oracle_golden.py).
 *
 * Reference sources followed (paths relative to /root/reference):
 *   philim      src/fortran/1d/classic/philim.f:1-58
 *   limiter     src/fortran/1d/classic/limiter.f:4-60
 *   step1       src/fortran/1d/classic/step1.f:4-142
 *   flux2       src/fortran/2d/classic/flux2.f:5-193   (+ flux2fw.f:151-152)
 *   step2ds     src/fortran/2d/classic/step2ds.f:2-248
 *   step2       src/fortran/2d/classic/step2.f:2-241
 *   rpn2 Euler  development/rp_approaches/rpn2_euler_5wave.f:5-302
 *   rpt2 Euler  development/rp_approaches/rpt2_euler_5wave_rec_loc.f:4-121
 *   flux3       src/fortran/3d/classic/flux3.f:168-258   (normal solve, CFL, correction: the part the
 *                                                          dimension-split algorithm uses, method(3)<0)
 *   step3ds     src/fortran/3d/classic/step3ds.f:108-374
 * Riemann solvers whose source is NOT in the reference tree (third-party
 * clawpack/riemann, unpinned; named in the app Makefiles only) are restated
 * from their published algorithm: rp1_advection, rp1_acoustics,
 * rpn2/rpt2_shallow_roe_with_efix (apps/shallow/2d/Makefile), rp1_euler_with_efix, rp1_shallow_roe_with_efix (apps/euler/1d, apps/shallow/1d Makefiles; restated like the
 * vendored 2-D Euler solver they share their structure with), rp1_burgers, rpn2_advection, rpt2_advection (named by apps/burgers/1d/Makefile, apps/advection/2d/Makefile;
 * no golden in the reference: parity unpinned at the Riemann-solver boundary),
 * rpn2_acoustics, rpt2_acoustics, rpn3_vc_acoustics (the reference's test/acoustics/3d/Makefile names
 * $(RIEMANN)/src/rpn3_vc_acoustics.f; pinned only through the scalar result 0.00286 +- 1e-4 of
 * test_3D_acoustics_homogeneous, test/test_examples.py:481-488).  rpn2_acoustics is pinned through the
 * reference golden test/acoustics2D_solution; the others are "parity
 * unpinned" at the Riemann-solver boundary.
 *
 * Array conventions are the Fortran ones: component index fastest,
 * q(m,i,j) at q[(m-1) + meqn*((i+mbc-1) + (mx+2mbc)*(j+mbc-1))].
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define RP_ADVECTION_1D 1
#define RP_ACOUSTICS_1D 2
#define RP_ACOUSTICS_2D 10
#define RP_EULER5_2D 11
#define RP_BURGERS_1D 3
#define RP_EULER_1D 4
#define RP_SHALLOW_1D 5
#define RP_ADVECTION_COLOR_1D 6
#define RP_ADVECTION_2D 12
#define RP_SHALLOW_2D 13
#define RP_VC_ACOUSTICS_2D 14
#define RP_VC_ADVECTION_2D 15
#define RP_ELASTICITY_FWAVE_1D 7
#define RP_SHALLOW_SPHERE_2D 16
#define RP_PSYSTEM_FWAVE_2D 17
#define RP_VC_ACOUSTICS_3D 20

static inline double dmax(double a, double b) { return a > b ? a : b; }
static inline double dmin(double a, double b) { return a < b ? a : b; }

/* ---------------------------------------------------------------- philim */
/* philim.f:19-55 */
static double philim(double a, double b, int meth)
{
    double r = b / a;
    switch (meth) {
    case 1: return dmax(0.0, dmin(1.0, r));
    case 2: return dmax(dmax(0.0, dmin(1.0, 2.0 * r)), dmin(2.0, r));
    case 3: return (r + fabs(r)) / (1.0 + fabs(r));
    case 4: {
        double c = (1.0 + r) / 2.0;
        return dmax(0.0, dmin(dmin(c, 2.0), 2.0 * r));
    }
    case 5: return r;
    }
    return 1.0;
}

/* slice-array accessors; i runs 1-mbc .. maxm+mbc like the Fortran */
#define IX(i) ((i) + mbc - 1)
#define W(m, mw, i) wave[((m)-1) + meqn * (((mw)-1) + mwaves * IX(i))]
#define S(mw, i) s[((mw)-1) + mwaves * IX(i)]
#define A2(arr, m, i) arr[((m)-1) + meqn * IX(i)]

/* --------------------------------------------------------------- limiter */
/* limiter.f:33-57 */
static void limiter(int meqn, int mwaves, int mbc, int mx, double *wave,
                    const double *s, const int *mthlim)
{
    for (int mw = 1; mw <= mwaves; mw++) {
        if (mthlim[mw - 1] == 0) continue;
        double dotr = 0.0;
        for (int i = 0; i <= mx + 1; i++) {
            double wnorm2 = 0.0;
            double dotl = dotr;
            dotr = 0.0;
            for (int m = 1; m <= meqn; m++) {
                wnorm2 = wnorm2 + W(m, mw, i) * W(m, mw, i);
                dotr = dotr + W(m, mw, i) * W(m, mw, i + 1);
            }
            if (i == 0) continue;
            if (wnorm2 == 0.0) continue;
            double wlimitr;
            if (S(mw, i) > 0.0)
                wlimitr = philim(wnorm2, dotl, mthlim[mw - 1]);
            else
                wlimitr = philim(wnorm2, dotr, mthlim[mw - 1]);
            for (int m = 1; m <= meqn; m++) W(m, mw, i) = wlimitr * W(m, mw, i);
        }
    }
}

/* ------------------------------------------------------- Riemann solvers */
/* 1-D, restated (third-party rp1_advection.f): wave = dq, s = u */
static void rp1_advection(int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                          double *wave, double *s, double *amdq, double *apdq,
                          const double *par)
{
    double u = par[0];
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        W(1, 1, i) = A2(ql, 1, i) - A2(qr, 1, i - 1);
        S(1, i) = u;
        A2(amdq, 1, i) = dmin(u, 0.0) * W(1, 1, i);
        A2(apdq, 1, i) = dmax(u, 0.0) * W(1, 1, i);
    }
}

/* 1-D acoustics, restated (third-party rp1_acoustics.f); par = rho,bulk,cc,zz */
static void rp1_acoustics(int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                          double *wave, double *s, double *amdq, double *apdq,
                          const double *par)
{
    double cc = par[2], zz = par[3];
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double d1 = A2(ql, 1, i) - A2(qr, 1, i - 1);
        double d2 = A2(ql, 2, i) - A2(qr, 2, i - 1);
        double a1 = (-d1 + zz * d2) / (2.0 * zz);
        double a2 = (d1 + zz * d2) / (2.0 * zz);
        W(1, 1, i) = -a1 * zz;
        W(2, 1, i) = a1;
        S(1, i) = -cc;
        W(1, 2, i) = a2 * zz;
        W(2, 2, i) = a2;
        S(2, i) = cc;
        for (int m = 1; m <= meqn; m++) {
            A2(amdq, m, i) = S(1, i) * W(m, 1, i);
            A2(apdq, m, i) = S(2, i) * W(m, 2, i);
        }
    }
}

/* 1-D Burgers' equation q_t + (q^2/2)_x = 0 with the transonic entropy fix, restated (third-party rp1_burgers.f90) */
static void rp1_burgers(int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                        double *wave, double *s, double *amdq, double *apdq, const double *par)
{
    (void)par;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double qL = A2(qr, 1, i - 1), qR = A2(ql, 1, i);
        W(1, 1, i) = qR - qL;
        S(1, i) = 0.5 * (qL + qR);
        A2(amdq, 1, i) = dmin(S(1, i), 0.0) * W(1, 1, i);
        A2(apdq, 1, i) = dmax(S(1, i), 0.0) * W(1, 1, i);
        if (qR > 0.0 && qL < 0.0) {          /* transonic rarefaction */
            A2(amdq, 1, i) = -0.5 * (qL * qL);
            A2(apdq, 1, i) = 0.5 * (qR * qR);
        }
    }
}

/* 1-D colour equation q_t + u(x) q_x = 0, restated (third-party rp1_advection_color.f, apps/advection/1d/variable):
 * aux(1,i) = velocity at the LEFT edge of cell i, i.e. at interface i */
extern const double *orc_aux1d;
extern int orc_maux1d;
static void rp1_advection_color(int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                                double *wave, double *s, double *amdq, double *apdq)
{
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const double u = orc_aux1d[0 + orc_maux1d * IX(i)];
        W(1, 1, i) = A2(ql, 1, i) - A2(qr, 1, i - 1);
        S(1, i) = u;
        A2(amdq, 1, i) = dmin(u, 0.0) * W(1, 1, i);
        A2(apdq, 1, i) = dmax(u, 0.0) * W(1, 1, i);
    }
}

/* 1-D Euler equations, Roe solver with the Harten-Hyman entropy fix, restated (third-party rp1_euler_with_efix.f;
 * same structure as the vendored rpn2_euler_5wave.f without the shear and tracer waves); par = gamma, gamma1 */
static void rp1_euler(int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                      double *wave, double *s, double *amdq, double *apdq, const double *par)
{
    const double gamma = par[0], gamma1 = par[1];
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const double rl = A2(qr, 1, i - 1), ml = A2(qr, 2, i - 1), el = A2(qr, 3, i - 1);
        const double rr = A2(ql, 1, i), mr = A2(ql, 2, i), er = A2(ql, 3, i);
        const double rsl = sqrt(rl), rsr = sqrt(rr);
        const double pl = gamma1 * (el - 0.5 * (ml * ml) / rl), pr = gamma1 * (er - 0.5 * (mr * mr) / rr);
        const double rhsq2 = rsl + rsr;
        const double u = (ml / rsl + mr / rsr) / rhsq2;
        const double enth = ((el + pl) / rsl + (er + pr) / rsr) / rhsq2;
        const double a2r = gamma1 * (enth - .5 * (u * u));
        const double a = sqrt(a2r);
        const double d1 = rr - rl, d2 = mr - ml, d3 = er - el;
        const double a2 = gamma1 / a2r * ((enth - u * u) * d1 + u * d2 - d3);
        const double a3 = (d2 + (a - u) * d1 - a * a2) / (2.0 * a);
        const double a1 = d1 - a2 - a3;
        W(1, 1, i) = a1; W(2, 1, i) = a1 * (u - a); W(3, 1, i) = a1 * (enth - u * a); S(1, i) = u - a;
        W(1, 2, i) = a2; W(2, 2, i) = a2 * u;       W(3, 2, i) = a2 * 0.5 * (u * u);  S(2, i) = u;
        W(1, 3, i) = a3; W(2, 3, i) = a3 * (u + a); W(3, 3, i) = a3 * (enth + u * a); S(3, i) = u + a;
        /* entropy fix */
        const double cl = sqrt(gamma * pl / rl);
        const double s0 = ml / rl - cl;
        int done = 0;
        if (s0 >= 0.0 && S(1, i) > 0.0) {
            for (int m = 1; m <= 3; m++) A2(amdq, m, i) = 0.0;
            done = 1;
        }
        if (!done) {
            const double rho1 = rl + W(1, 1, i), rhou1 = ml + W(2, 1, i), en1 = el + W(3, 1, i);
            const double p1 = gamma1 * (en1 - 0.5 * (rhou1 * rhou1) / rho1);
            const double c1 = sqrt(gamma * p1 / rho1);
            const double s1 = rhou1 / rho1 - c1;
            double sfract;
            if (s0 < 0.0 && s1 > 0.0) sfract = s0 * (s1 - S(1, i)) / (s1 - s0);
            else if (S(1, i) < 0.0) sfract = S(1, i);
            else sfract = 0.0;
            for (int m = 1; m <= 3; m++) A2(amdq, m, i) = sfract * W(m, 1, i);
            if (!(S(2, i) >= 0.0)) {
                for (int m = 1; m <= 3; m++) A2(amdq, m, i) = A2(amdq, m, i) + S(2, i) * W(m, 2, i);
                const double cr = sqrt(gamma * pr / rr);
                const double s3 = mr / rr + cr;
                const double rho2 = rr - W(1, 3, i), rhou2 = mr - W(2, 3, i), en2 = er - W(3, 3, i);
                const double p2 = gamma1 * (en2 - 0.5 * (rhou2 * rhou2) / rho2);
                const double c2 = sqrt(gamma * p2 / rho2);
                const double s2 = rhou2 / rho2 + c2;
                int add = 1;
                if (s2 < 0.0 && s3 > 0.0) sfract = s2 * (s3 - S(3, i)) / (s3 - s2);
                else if (S(3, i) < 0.0) sfract = S(3, i);
                else add = 0;
                if (add) for (int m = 1; m <= 3; m++) A2(amdq, m, i) = A2(amdq, m, i) + sfract * W(m, 3, i);
            }
        }
        for (int m = 1; m <= 3; m++) {
            double df = 0.0;
            for (int mw = 1; mw <= 3; mw++) df = df + S(mw, i) * W(m, mw, i);
            A2(apdq, m, i) = df - A2(amdq, m, i);
        }
    }
}

/* 1-D shallow water equations, Roe solver with the Harten-Hyman entropy fix, restated (third-party
 * rp1_shallow_roe_with_efix.f); q = (h, hu); par = g */
static void rp1_shallow(int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                        double *wave, double *s, double *amdq, double *apdq, const double *par)
{
    const double g = par[0];
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const double hl = A2(qr, 1, i - 1), ml = A2(qr, 2, i - 1), hr = A2(ql, 1, i), mr = A2(ql, 2, i);
        const double hsl = sqrt(hl), hsr = sqrt(hr);
        const double ubar = (ml / hsl + mr / hsr) / (hsl + hsr);
        const double cbar = sqrt(0.5 * g * (hl + hr));
        const double d1 = hr - hl, d2 = mr - ml;
        const double a1 = 0.5 * (-d2 + (ubar + cbar) * d1) / cbar;
        const double a2 = 0.5 * (d2 - (ubar - cbar) * d1) / cbar;
        W(1, 1, i) = a1; W(2, 1, i) = a1 * (ubar - cbar); S(1, i) = ubar - cbar;
        W(1, 2, i) = a2; W(2, 2, i) = a2 * (ubar + cbar); S(2, i) = ubar + cbar;
        /* entropy fix: 1-wave */
        const double s0 = ml / hl - sqrt(g * hl);
        int done = 0;
        if (s0 >= 0.0 && S(1, i) > 0.0) {
            A2(amdq, 1, i) = 0.0; A2(amdq, 2, i) = 0.0;
            done = 1;
        }
        if (!done) {
            const double h1 = hl + W(1, 1, i), hu1 = ml + W(2, 1, i);
            const double s1 = hu1 / h1 - sqrt(g * h1);
            double sfract;
            if (s0 < 0.0 && s1 > 0.0) sfract = s0 * (s1 - S(1, i)) / (s1 - s0);
            else if (S(1, i) < 0.0) sfract = S(1, i);
            else sfract = 0.0;
            for (int m = 1; m <= 2; m++) A2(amdq, m, i) = sfract * W(m, 1, i);
            /* 2-wave */
            const double s3 = mr / hr + sqrt(g * hr);
            const double h2 = hr - W(1, 2, i), hu2 = mr - W(2, 2, i);
            const double s2 = hu2 / h2 + sqrt(g * h2);
            int add = 1;
            if (s2 < 0.0 && s3 > 0.0) sfract = s2 * (s3 - S(2, i)) / (s3 - s2);
            else if (S(2, i) < 0.0) sfract = S(2, i);
            else add = 0;
            if (add) for (int m = 1; m <= 2; m++) A2(amdq, m, i) = A2(amdq, m, i) + sfract * W(m, 2, i);
        }
        for (int m = 1; m <= 2; m++) {
            double df = 0.0;
            for (int mw = 1; mw <= 2; mw++) df = df + S(mw, i) * W(m, mw, i);
            A2(apdq, m, i) = df - A2(amdq, m, i);
        }
    }
}

/* 2-D constant-coefficient advection q_t + u q_x + v q_y = 0, restated (third-party rpn2_advection.f /
 * rpt2_advection.f); par = u, v */
static void rpn2_advection(int ixy, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                           double *wave, double *s, double *amdq, double *apdq, const double *par)
{
    double vel = par[ixy - 1];
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        W(1, 1, i) = A2(ql, 1, i) - A2(qr, 1, i - 1);
        S(1, i) = vel;
        A2(amdq, 1, i) = dmin(vel, 0.0) * W(1, 1, i);
        A2(apdq, 1, i) = dmax(vel, 0.0) * W(1, 1, i);
    }
}
static void rpt2_advection(int ixy, int meqn, int mbc, int mx, const double *asdq, double *bmasdq,
                           double *bpasdq, const double *par)
{
    double stran = par[2 - ixy];             /* the OTHER velocity */
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        A2(bmasdq, 1, i) = dmin(stran, 0.0) * A2(asdq, 1, i);
        A2(bpasdq, 1, i) = dmax(stran, 0.0) * A2(asdq, 1, i);
    }
}

/* 2-D shallow water, Roe solver with the Harten-Hyman entropy fix and its transverse solver, restated
 * (third-party rpn2_shallow_roe_with_efix.f / rpt2_shallow_roe_with_efix.f); q = (h, hu, hv); par = g */
typedef struct { double h, u, v, a; } swroe_t;
static inline swroe_t sw_roe(const double *ql, const double *qr, int meqn, int mbc, int i, int mu, int mv, double g)
{
    swroe_t r;
    r.h = (A2(qr, 1, i - 1) + A2(ql, 1, i)) * 0.5;
    const double hsl = sqrt(A2(qr, 1, i - 1)), hsr = sqrt(A2(ql, 1, i)), hsq2 = hsl + hsr;
    r.u = (A2(qr, mu, i - 1) / hsl + A2(ql, mu, i) / hsr) / hsq2;
    r.v = (A2(qr, mv, i - 1) / hsl + A2(ql, mv, i) / hsr) / hsq2;
    r.a = sqrt(g * r.h);
    return r;
}
static void rpn2_shallow(int ixy, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                         double *wave, double *s, double *amdq, double *apdq, const double *par)
{
    const double g = par[0];
    const int mu = (ixy == 1) ? 2 : 3, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const swroe_t r = sw_roe(ql, qr, meqn, mbc, i, mu, mv, g);
        const double d1 = A2(ql, 1, i) - A2(qr, 1, i - 1), d2 = A2(ql, mu, i) - A2(qr, mu, i - 1);
        const double d3 = A2(ql, mv, i) - A2(qr, mv, i - 1);
        const double a1 = ((r.u + r.a) * d1 - d2) * (0.5 / r.a);
        const double a2 = -r.v * d1 + d3;
        const double a3 = (-(r.u - r.a) * d1 + d2) * (0.5 / r.a);
        W(1, 1, i) = a1; W(mu, 1, i) = a1 * (r.u - r.a); W(mv, 1, i) = a1 * r.v; S(1, i) = r.u - r.a;
        W(1, 2, i) = 0.0; W(mu, 2, i) = 0.0; W(mv, 2, i) = a2; S(2, i) = r.u;
        W(1, 3, i) = a3; W(mu, 3, i) = a3 * (r.u + r.a); W(mv, 3, i) = a3 * r.v; S(3, i) = r.u + r.a;
        const double hl = A2(qr, 1, i - 1), hr = A2(ql, 1, i);
        const double s0 = A2(qr, mu, i - 1) / hl - sqrt(g * hl);
        int done = 0;
        if (s0 >= 0.0 && S(1, i) > 0.0) {
            for (int m = 1; m <= 3; m++) A2(amdq, m, i) = 0.0;
            done = 1;
        }
        if (!done) {
            const double h1 = hl + W(1, 1, i), hu1 = A2(qr, mu, i - 1) + W(mu, 1, i);
            const double s1 = hu1 / h1 - sqrt(g * h1);
            double sfract;
            if (s0 < 0.0 && s1 > 0.0) sfract = s0 * (s1 - S(1, i)) / (s1 - s0);
            else if (S(1, i) < 0.0) sfract = S(1, i);
            else sfract = 0.0;
            for (int m = 1; m <= 3; m++) A2(amdq, m, i) = sfract * W(m, 1, i);
            if (!(S(2, i) >= 0.0)) {
                for (int m = 1; m <= 3; m++) A2(amdq, m, i) = A2(amdq, m, i) + S(2, i) * W(m, 2, i);
                const double s03 = A2(ql, mu, i) / hr + sqrt(g * hr);
                const double h3 = hr - W(1, 3, i), hu3 = A2(ql, mu, i) - W(mu, 3, i);
                const double s3 = hu3 / h3 + sqrt(g * h3);
                int add = 1;
                if (s3 < 0.0 && s03 > 0.0) sfract = s3 * (s03 - S(3, i)) / (s03 - s3);
                else if (S(3, i) < 0.0) sfract = S(3, i);
                else add = 0;
                if (add) for (int m = 1; m <= 3; m++) A2(amdq, m, i) = A2(amdq, m, i) + sfract * W(m, 3, i);
            }
        }
        for (int m = 1; m <= 3; m++) {
            double df = 0.0;
            for (int mw = 1; mw <= 3; mw++) df = df + S(mw, i) * W(m, mw, i);
            A2(apdq, m, i) = df - A2(amdq, m, i);
        }
    }
}
static void rpt2_shallow(int ixy, int meqn, int mbc, int mx, const double *q, const double *asdq,
                         double *bmasdq, double *bpasdq, const double *par)
{
    const double g = par[0];
    const int mu = (ixy == 1) ? 2 : 3, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const swroe_t r = sw_roe(q, q, meqn, mbc, i, mu, mv, g);
        const double a1 = (0.5 / r.a) * ((r.v + r.a) * A2(asdq, 1, i) - A2(asdq, mv, i));
        const double a2 = A2(asdq, mu, i) - r.u * A2(asdq, 1, i);
        const double a3 = (0.5 / r.a) * (-(r.v - r.a) * A2(asdq, 1, i) + A2(asdq, mv, i));
        double wb[4][4], sb[4];
        wb[1][1] = a1; wb[mu][1] = a1 * r.u; wb[mv][1] = a1 * (r.v - r.a); sb[1] = r.v - r.a;
        wb[1][2] = 0.0; wb[mu][2] = a2; wb[mv][2] = 0.0; sb[2] = r.v;
        wb[1][3] = a3; wb[mu][3] = a3 * r.u; wb[mv][3] = a3 * (r.v + r.a); sb[3] = r.v + r.a;
        for (int m = 1; m <= 3; m++) {
            double bm = 0.0, bp = 0.0;
            for (int mw = 1; mw <= 3; mw++) {
                bm = bm + dmin(sb[mw], 0.0) * wb[m][mw];
                bp = bp + dmax(sb[mw], 0.0) * wb[m][mw];
            }
            A2(bmasdq, m, i) = bm;
            A2(bpasdq, m, i) = bp;
        }
    }
}

/* The aux values of the slice being solved, for Riemann solvers with cell-wise coefficients: the Fortran passes
 * aux2(:,:,2) of the slice next to q1d (flux2.f:99); the slice drivers below set these before every solve. */
const double *orc_aux1d = NULL;    /* auxl: aux of the cell to the RIGHT of interface i is orc_aux1d(:, i)            */
const double *orc_auxr1d = NULL;   /* auxr: aux of the cell to the LEFT is orc_auxr1d(:, i-1); NULL = same array        */
int orc_maux1d = 0;
/* for transverse solvers with cell-wise coefficients: aux of the neighbouring slices (aux1 / aux3 of step2.f:97-101) */
const double *orc_auxb1d = NULL, *orc_auxa1d = NULL;

/* 2-D acoustics with cell-wise impedance and sound speed, restated (third-party rpn2_vc_acoustics.f; same
 * formulas as rpn3_vc_acoustics below); q = (p, u, v); aux(1) = Z, aux(2) = c */
static void rpn2_vc_acoustics(int ixy, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                              double *wave, double *s, double *amdq, double *apdq)
{
    const double *aux = orc_aux1d, *auxr = orc_auxr1d ? orc_auxr1d : orc_aux1d;
    const int maux = orc_maux1d;
#define AX(ma, i) aux[((ma)-1) + maux * IX(i)]
#define AXR(ma, i) auxr[((ma)-1) + maux * IX(i)]
    int mu = ixy + 1;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double d1 = A2(ql, 1, i) - A2(qr, 1, i - 1);
        double d2 = A2(ql, mu, i) - A2(qr, mu, i - 1);
        double zi = AX(1, i), zim = AXR(1, i - 1);
        double a1 = (-d1 + zi * d2) / (zim + zi);
        double a2 = (d1 + zim * d2) / (zim + zi);
        for (int m = 1; m <= meqn; m++) { W(m, 1, i) = 0.0; W(m, 2, i) = 0.0; }
        W(1, 1, i) = -a1 * zim;
        W(mu, 1, i) = a1;
        S(1, i) = -AXR(2, i - 1);
        W(1, 2, i) = a2 * zi;
        W(mu, 2, i) = a2;
        S(2, i) = AX(2, i);
    }
    for (int m = 1; m <= meqn; m++)
        for (int i = 2 - mbc; i <= mx + mbc; i++) {
            A2(amdq, m, i) = S(1, i) * W(m, 1, i);
            A2(apdq, m, i) = S(2, i) * W(m, 2, i);
        }
#undef AX
#undef AXR
}

/* 2-D colour equation q_t + u(x,y) q_x + v(x,y) q_y = 0 with edge velocities, restated (third-party
 * rpn2_vc_advection.f / rpt2_vc_advection.f, apps/advection/2d/annulus): aux(1) = u at the cell's left edge,
 * aux(2) = v at its bottom edge */
static void rpn2_vc_advection(int ixy, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                              double *wave, double *s, double *amdq, double *apdq)
{
    const int maux = orc_maux1d;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const double vel = orc_aux1d[(ixy - 1) + maux * IX(i)];
        W(1, 1, i) = A2(ql, 1, i) - A2(qr, 1, i - 1);
        S(1, i) = vel;
        A2(amdq, 1, i) = dmin(vel, 0.0) * W(1, 1, i);
        A2(apdq, 1, i) = dmax(vel, 0.0) * W(1, 1, i);
    }
}
static void rpt2_vc_advection(int ixy, int imp, int meqn, int mbc, int mx, const double *asdq, double *bmasdq,
                              double *bpasdq)
{
    const int maux = orc_maux1d, kv = 3 - ixy;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const int i1 = i - 2 + imp;
        A2(bmasdq, 1, i) = dmin(orc_aux1d[(kv - 1) + maux * IX(i1)], 0.0) * A2(asdq, 1, i);
        A2(bpasdq, 1, i) = dmax(orc_auxa1d[(kv - 1) + maux * IX(i1)], 0.0) * A2(asdq, 1, i);
    }
}

/* transverse solver of the variable-coefficient acoustics equations, restated (third-party rpt2_vc_acoustics.f):
 * the down-going part of asdq enters the slice below with ITS impedance and sound speed, the up-going part the
 * slice above; i1 = i-2+imp is the cell asdq belongs to (left of the interface for amdq, right for apdq) */
static void rpt2_vc_acoustics(int ixy, int imp, int meqn, int mbc, int mx, const double *asdq, double *bmasdq,
                              double *bpasdq)
{
    const int maux = orc_maux1d;
    const double *aux1 = orc_auxb1d, *aux2 = orc_aux1d, *aux3 = orc_auxa1d;
#define AXN(arr, ma, i) arr[((ma)-1) + maux * IX(i)]
    const int mu = ixy + 1, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const int i1 = i - 2 + imp;
        const double zm = AXN(aux1, 1, i1), zz = AXN(aux2, 1, i1), zp = AXN(aux3, 1, i1);
        const double cm = AXN(aux1, 2, i1), cp = AXN(aux3, 2, i1);
        const double a1 = (-A2(asdq, 1, i) + A2(asdq, mv, i) * zz) / (zm + zz);
        const double a2 = (A2(asdq, 1, i) + A2(asdq, mv, i) * zz) / (zz + zp);
        A2(bmasdq, 1, i) = cm * a1 * zm;
        A2(bmasdq, mu, i) = 0.0;
        A2(bmasdq, mv, i) = -cm * a1;
        A2(bpasdq, 1, i) = cp * a2 * zp;
        A2(bpasdq, mu, i) = 0.0;
        A2(bpasdq, mv, i) = cp * a2;
    }
#undef AXN
}


/* ------------------------------------------------------------------------------------------------------------
 * Shallow water on the sphere (Calhoun, Helzel & LeVeque, SIAM Review 50 (2008) 723-752), 3-D Cartesian momentum:
 * q = (h, hu, hv, hw), 3 waves, 16 aux components laid out by the reference's setaux.f:10-25
 * (test/shallow_sphere/setaux.f; 1 kappa, 2-4 / 5-7 normal and tangent of the LEFT edge, 8-10 / 11-13 of the
 * BOTTOM edge, 14-16 radial unit vector at the cell centre).
 *
 * The Riemann solvers rpn2_shallow_sphere.f / rpt2_shallow_sphere.f are THIRD-PARTY (clawpack/riemann, named by
 * test/shallow_sphere/Makefile:7 as $(RIEMANN)/src/..., no version pinned) and absent from the reference tree:
 * restated here from the published algorithm -- Roe solver in the edge-normal / edge-tangent frame, waves rotated
 * back to Cartesian momentum, Harten-Hyman entropy fix, fluctuations projected onto the tangent plane of the cell
 * they enter; speeds scaled by (edge length / computational cell width).  PARITY of these two routines is pinned only
 * through the reference's golden test/swsphere_height at its own gate (2-norm < 1e-4, test/test_examples.py:456-472).
 * par = g (common /sw/), dxcom, dycom (common /comxyt/, set by the app: shallow_4_Rossby_Haurwitz_wave.py:449-451).
 * ------------------------------------------------------------------------------------------------------------ */
static void rpn2_sphere(int ixy, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                        double *wave, double *s, double *amdq, double *apdq, const double *par)
{
    const double *auxl = orc_aux1d, *auxr = orc_auxr1d ? orc_auxr1d : orc_aux1d;
    const int maux = orc_maux1d;
    const double g = par[0];
    const double dy = (ixy == 1) ? par[2] : par[1];
    const int ioff = (ixy == 1) ? 1 : 7;
#define AXL(ma, i) auxl[((ma)-1) + maux * IX(i)]
#define AXR(ma, i) auxr[((ma)-1) + maux * IX(i)]
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double enx = AXL(ioff + 1, i), eny = AXL(ioff + 2, i), enz = AXL(ioff + 3, i);
        double etx = AXL(ioff + 4, i), ety = AXL(ioff + 5, i), etz = AXL(ioff + 6, i);
        const double gamma = sqrt(etx * etx + ety * ety + etz * etz);
        etx = etx / gamma; ety = ety / gamma; etz = etz / gamma;
        /* normal and tangential momentum at the edge: "l" = ql(i) (right of the interface), "r" = qr(i-1) */
        const double hunl = enx * A2(ql, 2, i) + eny * A2(ql, 3, i) + enz * A2(ql, 4, i);
        const double hunr = enx * A2(qr, 2, i - 1) + eny * A2(qr, 3, i - 1) + enz * A2(qr, 4, i - 1);
        const double hutl = etx * A2(ql, 2, i) + ety * A2(ql, 3, i) + etz * A2(ql, 4, i);
        const double hutr = etx * A2(qr, 2, i - 1) + ety * A2(qr, 3, i - 1) + etz * A2(qr, 4, i - 1);
        /* Roe averages */
        const double h = (A2(qr, 1, i - 1) + A2(ql, 1, i)) * 0.50;
        const double hsqr = sqrt(A2(qr, 1, i - 1)), hsql = sqrt(A2(ql, 1, i)), hsq = hsqr + hsql;
        const double u = (hunr / hsqr + hunl / hsql) / hsq;
        const double v = (hutr / hsqr + hutl / hsql) / hsq;
        const double a = sqrt(g * h);
        const double delta1 = A2(ql, 1, i) - A2(qr, 1, i - 1);
        const double delta2 = hunl - hunr;
        const double delta3 = hutl - hutr;
        const double a1 = ((u + a) * delta1 - delta2) * (0.50 / a);
        const double a2 = -v * delta1 + delta3;
        const double a3 = (-(u - a) * delta1 + delta2) * (0.50 / a);
        W(1, 1, i) = a1;
        W(2, 1, i) = a1 * (u - a) * enx + a1 * v * etx;
        W(3, 1, i) = a1 * (u - a) * eny + a1 * v * ety;
        W(4, 1, i) = a1 * (u - a) * enz + a1 * v * etz;
        S(1, i) = (u - a) * gamma / dy;
        W(1, 2, i) = 0.0;
        W(2, 2, i) = a2 * etx;
        W(3, 2, i) = a2 * ety;
        W(4, 2, i) = a2 * etz;
        S(2, i) = u * gamma / dy;
        W(1, 3, i) = a3;
        W(2, 3, i) = a3 * (u + a) * enx + a3 * v * etx;
        W(3, 3, i) = a3 * (u + a) * eny + a3 * v * ety;
        W(4, 3, i) = a3 * (u + a) * enz + a3 * v * etz;
        S(3, i) = (u + a) * gamma / dy;

        /* Harten-Hyman entropy fix: amdq = sum of s*wave over the left-going parts */
        for (int m = 1; m <= 4; m++) A2(amdq, m, i) = 0.0;
        int done = 0;
        const double him1 = A2(qr, 1, i - 1);
        const double s0 = (hunr / him1 - sqrt(g * him1)) * gamma / dy;
        if (s0 > 0.0 && S(1, i) > 0.0) done = 1;            /* fully supersonic to the right */
        if (!done) {
            const double h1 = A2(qr, 1, i - 1) + W(1, 1, i);
            const double hu1 = hunr + enx * W(2, 1, i) + eny * W(3, 1, i) + enz * W(4, 1, i);
            const double s1 = (hu1 / h1 - sqrt(g * h1)) * gamma / dy;
            double sfract;
            if (s0 < 0.0 && s1 > 0.0) sfract = s0 * ((s1 - S(1, i)) / (s1 - s0));
            else if (S(1, i) < 0.0) sfract = S(1, i);
            else sfract = 0.0;
            for (int m = 1; m <= 4; m++) A2(amdq, m, i) = sfract * W(m, 1, i);
            if (S(2, i) > 0.0) done = 1;                    /* 2- and 3-waves go right */
        }
        if (!done) {
            for (int m = 1; m <= 4; m++) A2(amdq, m, i) = A2(amdq, m, i) + S(2, i) * W(m, 2, i);
            const double hi = A2(ql, 1, i);
            const double s03 = (hunl / hi + sqrt(g * hi)) * gamma / dy;
            const double h3 = A2(ql, 1, i) - W(1, 3, i);
            const double hu3 = hunl - (enx * W(2, 3, i) + eny * W(3, 3, i) + enz * W(4, 3, i));
            const double s3 = (hu3 / h3 + sqrt(g * h3)) * gamma / dy;
            double sfract = 0.0;
            int add = 1;
            if (s3 < 0.0 && s03 > 0.0) sfract = s3 * ((s03 - S(3, i)) / (s03 - s3));
            else if (S(3, i) < 0.0) sfract = S(3, i);
            else add = 0;
            if (add) for (int m = 1; m <= 4; m++) A2(amdq, m, i) = A2(amdq, m, i) + sfract * W(m, 3, i);
        }
        for (int m = 1; m <= 4; m++) {
            double df = 0.0;
            for (int mw = 1; mw <= mwaves; mw++) df = df + S(mw, i) * W(m, mw, i);
            A2(apdq, m, i) = df - A2(amdq, m, i);
        }
        /* project the momentum parts onto the tangent plane of the cell each fluctuation enters */
        {
            const double erx = AXR(14, i - 1), ery = AXR(15, i - 1), erz = AXR(16, i - 1);
            const double amn = erx * A2(amdq, 2, i) + ery * A2(amdq, 3, i) + erz * A2(amdq, 4, i);
            A2(amdq, 2, i) = A2(amdq, 2, i) - amn * erx;
            A2(amdq, 3, i) = A2(amdq, 3, i) - amn * ery;
            A2(amdq, 4, i) = A2(amdq, 4, i) - amn * erz;
        }
        {
            const double erx = AXL(14, i), ery = AXL(15, i), erz = AXL(16, i);
            const double apn = erx * A2(apdq, 2, i) + ery * A2(apdq, 3, i) + erz * A2(apdq, 4, i);
            A2(apdq, 2, i) = A2(apdq, 2, i) - apn * erx;
            A2(apdq, 3, i) = A2(apdq, 3, i) - apn * ery;
            A2(apdq, 4, i) = A2(apdq, 4, i) - apn * erz;
        }
    }
#undef AXL
#undef AXR
}

/* Transverse solver, restated (third-party rpt2_shallow_sphere.f).  asdq sits in cell i1 = i-2+imp (left of the
 * interface for A^-dq, right for A^+dq).  Up-going part: Roe-type split in the frame of the edge ABOVE that cell
 * (= the bottom/left edge of the cell in the next slice, aux3) with the cell's own depth and velocity, projected
 * onto the tangent plane of the cell above; down-going part: the cell's own lower edge (aux2), projected onto the
 * tangent plane of the cell below (aux1). */
static void rpt2_sphere(int ixy, int imp, int meqn, int mbc, int mx, const double *q, const double *asdq,
                        double *bmasdq, double *bpasdq, const double *par)
{
    const int maux = orc_maux1d;
    const double *aux1 = orc_auxb1d, *aux2 = orc_aux1d, *aux3 = orc_auxa1d;
    const double g = par[0];
    const double dx = (ixy == 1) ? par[1] : par[2];
    const int ioff = (ixy == 1) ? 7 : 1;
#define AXN(arr, ma, i) arr[((ma)-1) + maux * IX(i)]
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const int i1 = i - 2 + imp;
        for (int up = 1; up >= 0; up--) {
            const double *ae = up ? aux3 : aux2;       /* edge geometry */
            const double *ap = up ? aux3 : aux1;       /* tangent plane of the receiving cell */
            double enx = AXN(ae, ioff + 1, i1), eny = AXN(ae, ioff + 2, i1), enz = AXN(ae, ioff + 3, i1);
            double etx = AXN(ae, ioff + 4, i1), ety = AXN(ae, ioff + 5, i1), etz = AXN(ae, ioff + 6, i1);
            const double gamma = sqrt(etx * etx + ety * ety + etz * etz);
            etx = etx / gamma; ety = ety / gamma; etz = etz / gamma;
            const double h = A2(q, 1, i1);
            const double u = (enx * A2(q, 2, i1) + eny * A2(q, 3, i1) + enz * A2(q, 4, i1)) / h;
            const double v = (etx * A2(q, 2, i1) + ety * A2(q, 3, i1) + etz * A2(q, 4, i1)) / h;
            const double a = sqrt(g * h);
            const double delta1 = A2(asdq, 1, i);
            const double delta2 = enx * A2(asdq, 2, i) + eny * A2(asdq, 3, i) + enz * A2(asdq, 4, i);
            const double delta3 = etx * A2(asdq, 2, i) + ety * A2(asdq, 3, i) + etz * A2(asdq, 4, i);
            const double a1 = ((u + a) * delta1 - delta2) * (0.50 / a);
            const double a2 = -v * delta1 + delta3;
            const double a3 = (-(u - a) * delta1 + delta2) * (0.50 / a);
            double wb[5][4], sb[4];
            wb[1][1] = a1;
            wb[2][1] = a1 * (u - a) * enx + a1 * v * etx;
            wb[3][1] = a1 * (u - a) * eny + a1 * v * ety;
            wb[4][1] = a1 * (u - a) * enz + a1 * v * etz;
            sb[1] = (u - a) * gamma / dx;
            wb[1][2] = 0.0;
            wb[2][2] = a2 * etx;
            wb[3][2] = a2 * ety;
            wb[4][2] = a2 * etz;
            sb[2] = u * gamma / dx;
            wb[1][3] = a3;
            wb[2][3] = a3 * (u + a) * enx + a3 * v * etx;
            wb[3][3] = a3 * (u + a) * eny + a3 * v * ety;
            wb[4][3] = a3 * (u + a) * enz + a3 * v * etz;
            sb[3] = (u + a) * gamma / dx;
            double *out = up ? bpasdq : bmasdq;
            for (int m = 1; m <= 4; m++) {
                double acc = 0.0;
                for (int mw = 1; mw <= 3; mw++)
                    acc = acc + (up ? dmax(sb[mw], 0.0) : dmin(sb[mw], 0.0)) * wb[m][mw];
                A2(out, m, i) = acc;
            }
            const double erx = AXN(ap, 14, i1), ery = AXN(ap, 15, i1), erz = AXN(ap, 16, i1);
            const double bn = erx * A2(out, 2, i) + ery * A2(out, 3, i) + erz * A2(out, 4, i);
            A2(out, 2, i) = A2(out, 2, i) - bn * erx;
            A2(out, 3, i) = A2(out, 3, i) - bn * ery;
            A2(out, 4, i) = A2(out, 4, i) - bn * erz;
        }
    }
#undef AXN
}

/* qcor.f:1-72 (test/shallow_sphere/qcor.f): correction that keeps the scheme conservative on the sphere; aux2 and
 * q1d are the current slice.  qc[1..4]. */
static void sphere_qcor(int ixy, int i, const double *aux, int maux, const double *q, int meqn, int mbc,
                        const double *par, double *qc)
{
#define AXQ(ma, i) aux[((ma)-1) + maux * IX(i)]
    const double g = par[0];
    const int in = (ixy == 1) ? 2 : 8;
    const double dy = (ixy == 1) ? par[2] : par[1];
    const double etxl = AXQ(in + 3, i), etyl = AXQ(in + 4, i), etzl = AXQ(in + 5, i);
    const double gammal = sqrt(etxl * etxl + etyl * etyl + etzl * etzl) / dy;
    const double enxl = AXQ(in, i) * gammal, enyl = AXQ(in + 1, i) * gammal, enzl = AXQ(in + 2, i) * gammal;
    const double etxr = AXQ(in + 3, i + 1), etyr = AXQ(in + 4, i + 1), etzr = AXQ(in + 5, i + 1);
    const double gammar = sqrt(etxr * etxr + etyr * etyr + etzr * etzr) / dy;
    const double enxr = AXQ(in, i + 1) * gammar, enyr = AXQ(in + 1, i + 1) * gammar, enzr = AXQ(in + 2, i + 1) * gammar;
    const double q1 = A2(q, 1, i), q2 = A2(q, 2, i), q3 = A2(q, 3, i), q4 = A2(q, 4, i);
    qc[1] = (enxr - enxl) * q2 + (enyr - enyl) * q3 + (enzr - enzl) * q4;
    qc[2] = (enxr - enxl) * (q2 * q2 / q1 + 0.5 * g * (q1 * q1)) + (enyr - enyl) * (q2 * q3 / q1) +
            (enzr - enzl) * (q2 * q4 / q1);
    qc[3] = (enxr - enxl) * (q2 * q3 / q1) + (enyr - enyl) * (q3 * q3 / q1 + 0.5 * g * (q1 * q1)) +
            (enzr - enzl) * (q3 * q4 / q1);
    qc[4] = (enxr - enxl) * (q2 * q4 / q1) + (enyr - enyl) * (q3 * q4 / q1) +
            (enzr - enzl) * (q4 * q4 / q1 + 0.5 * g * (q1 * q1));
    const double erx = AXQ(14, i), ery = AXQ(15, i), erz = AXQ(16, i);
    const double qcn = erx * qc[2] + ery * qc[3] + erz * qc[4];
    qc[2] = qc[2] - qcn * erx;
    qc[3] = qc[3] - qcn * ery;
    qc[4] = qc[4] - qcn * erz;
#undef AXQ
}
/* step2qcor.f is the app's replacement of step2.f (test/shallow_sphere/Makefile:16): orc_step2 follows it when
 * this switch is on (the capa branch then also subtracts dtdx*qc/capa, step2qcor.f:146-159,232-245). */
static int orc_qcor_on = 0;
void orc_set_qcor(int on) { orc_qcor_on = on; }


/* ------------------------------------------------------------------------------------------------------------
 * f-wave Riemann solvers (flux2fw.f / step1fw.f take the jump in the FLUX split into waves).  Both are THIRD-PARTY
 * (clawpack/riemann: rp1_nonlinear_elasticity_fwave.f named by apps/elasticity/1d/stegoton/Makefile, rpn2_psystem.f /
 * rpt2_psystem.f by test/psystem/Makefile:5), absent from the reference tree and pinned by no golden (the
 * reference's own psystem verifier returns True, test/test_examples.py:437-441): restated from the published
 * eigen-structure, PARITY UNPINNED at the solver boundary.  The f-wave PATH (flux2fw.f:151-152, step1fw.f:135-141)
 * is in the tree and is what these solvers exercise.
 *   eps_t - (m/rho)_x = 0,  m_t - sigma(eps, x)_x = 0     (2-D: + the same in y for the second momentum)
 *   stress law per cell: aux(3) == 1: sigma = K eps (linear);  otherwise sigma = exp(K eps) - 1 (LeVeque & Yong 2003;
 *   the reference apps: stegoton.py:12-13 / psystem.py:108, setaux aux(1) = rho, aux(2) = K [, aux(3) = flag])
 * Interface i, left cell i-1 (suffix m), right cell i:  c = sqrt(sigma'/rho), Z = rho c,
 *   b1 = -(Z_i du + dsig)/(Z_m + Z_i)  on (1, Z_m) at speed -c_m,   b2 = -(Z_m du - dsig)/(Z_m + Z_i) on (1, -Z_i) at +c_i.
 * ------------------------------------------------------------------------------------------------------------ */
static inline double ps_sigma(double eps, double K, double lin) { return lin == 1.0 ? K * eps : exp(K * eps) - 1.0; }
static inline double ps_sigmap(double eps, double K, double lin) { return lin == 1.0 ? K : K * exp(K * eps); }

static void rp_fwave_normal(int mu, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                            double *fwave, double *s, double *amdq, double *apdq)
{
    const double *auxl = orc_aux1d, *auxr = orc_auxr1d ? orc_auxr1d : orc_aux1d;
    const int maux = orc_maux1d;
    double *wave = fwave;
#define AXL(ma, i) auxl[((ma)-1) + maux * IX(i)]
#define AXR(ma, i) auxr[((ma)-1) + maux * IX(i)]
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const double rhoi = AXL(1, i), rhoim = AXR(1, i - 1);
        const double epsi = A2(ql, 1, i), epsim = A2(qr, 1, i - 1);
        const double urhoi = A2(ql, mu, i), urhoim = A2(qr, mu, i - 1);
        const double bulki = ps_sigmap(epsi, AXL(2, i), AXL(3, i));
        const double bulkim = ps_sigmap(epsim, AXR(2, i - 1), AXR(3, i - 1));
        const double ci = sqrt(bulki / rhoi), cim = sqrt(bulkim / rhoim);
        const double zi = ci * rhoi, zim = cim * rhoim;
        const double du = urhoi / rhoi - urhoim / rhoim;
        const double dsig = ps_sigma(epsi, AXL(2, i), AXL(3, i)) - ps_sigma(epsim, AXR(2, i - 1), AXR(3, i - 1));
        const double b1 = -(zi * du + dsig) / (zim + zi);
        const double b2 = -(zim * du - dsig) / (zim + zi);
        for (int m = 1; m <= meqn; m++) { W(m, 1, i) = 0.0; W(m, 2, i) = 0.0; }
        W(1, 1, i) = b1;
        W(mu, 1, i) = b1 * zim;
        S(1, i) = -cim;
        W(1, 2, i) = b2;
        W(mu, 2, i) = b2 * (-zi);
        S(2, i) = ci;
        for (int m = 1; m <= meqn; m++) {
            A2(amdq, m, i) = W(m, 1, i);
            A2(apdq, m, i) = W(m, 2, i);
        }
    }
#undef AXL
#undef AXR
}

/* transverse solver of the p-system: asdq sits in cell i1 = i-2+imp; the down-going part enters the row below with
 * ITS impedance and speed, the up-going part the row above.  The rows' strains come from aux(4) (the app copies
 * q(1) there before each step: psystem.py:96-99, "required in rptpv.f").  asdq = b1 (1,0,Z_m) + b3 (1,0,-Z_p). */
static void rpt2_psystem(int ixy, int imp, int meqn, int mbc, int mx, const double *asdq, double *bmasdq,
                         double *bpasdq)
{
    const int maux = orc_maux1d;
    const double *aux1 = orc_auxb1d, *aux3 = orc_auxa1d;
#define AXN(arr, ma, i) arr[((ma)-1) + maux * IX(i)]
    const int mu = ixy + 1, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const int i1 = i - 2 + imp;
        const double rhom = AXN(aux1, 1, i1), rhop = AXN(aux3, 1, i1);
        const double bulkm = ps_sigmap(AXN(aux1, 4, i1), AXN(aux1, 2, i1), AXN(aux1, 3, i1));
        const double bulkp = ps_sigmap(AXN(aux3, 4, i1), AXN(aux3, 2, i1), AXN(aux3, 3, i1));
        const double cm = sqrt(bulkm / rhom), cp = sqrt(bulkp / rhop);
        const double zm = cm * rhom, zp = cp * rhop;
        const double b1 = (A2(asdq, mv, i) + zp * A2(asdq, 1, i)) / (zm + zp);
        const double b3 = (zm * A2(asdq, 1, i) - A2(asdq, mv, i)) / (zm + zp);
        A2(bmasdq, 1, i) = -cm * b1;
        A2(bmasdq, mu, i) = 0.0;
        A2(bmasdq, mv, i) = -cm * b1 * zm;
        A2(bpasdq, 1, i) = cp * b3;
        A2(bpasdq, mu, i) = 0.0;
        A2(bpasdq, mv, i) = cp * b3 * (-zp);
    }
#undef AXN
}

/* 2-D acoustics normal solver, restated (third-party rpn2_acoustics.f) */
static void rpn2_acoustics(int ixy, int meqn, int mwaves, int mbc, int mx,
                           const double *ql, const double *qr, double *wave, double *s, double *amdq,
                           double *apdq, const double *par)
{
    double cc = par[2], zz = par[3];
    int mu = (ixy == 1) ? 2 : 3, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double d1 = A2(ql, 1, i) - A2(qr, 1, i - 1);
        double d2 = A2(ql, mu, i) - A2(qr, mu, i - 1);
        double a1 = (-d1 + zz * d2) / (2.0 * zz);
        double a2 = (d1 + zz * d2) / (2.0 * zz);
        W(1, 1, i) = -a1 * zz;
        W(mu, 1, i) = a1;
        W(mv, 1, i) = 0.0;
        S(1, i) = -cc;
        W(1, 2, i) = a2 * zz;
        W(mu, 2, i) = a2;
        W(mv, 2, i) = 0.0;
        S(2, i) = cc;
    }
    for (int m = 1; m <= meqn; m++)
        for (int i = 2 - mbc; i <= mx + mbc; i++) {
            A2(amdq, m, i) = S(1, i) * W(m, 1, i);
            A2(apdq, m, i) = S(2, i) * W(m, 2, i);
        }
}

/* 2-D acoustics transverse solver, restated (third-party rpt2_acoustics.f) */
static void rpt2_acoustics(int ixy, int meqn, int mbc, int mx, const double *asdq,
                           double *bmasdq, double *bpasdq, const double *par)
{
    double cc = par[2], zz = par[3];
    int mu = (ixy == 1) ? 2 : 3, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double a1 = (-A2(asdq, 1, i) + zz * A2(asdq, mv, i)) / (2.0 * zz);
        double a2 = (A2(asdq, 1, i) + zz * A2(asdq, mv, i)) / (2.0 * zz);
        A2(bmasdq, 1, i) = cc * a1 * zz;
        A2(bmasdq, mu, i) = 0.0;
        A2(bmasdq, mv, i) = -cc * a1;
        A2(bpasdq, 1, i) = cc * a2 * zz;
        A2(bpasdq, mu, i) = 0.0;
        A2(bpasdq, mv, i) = cc * a2;
    }
}

/* Roe averages of one Euler interface; rpn2_euler_5wave.f:87-104 */
typedef struct { double u, v, enth, a, g1a2, euv, u2v2; } roe_t;

static inline roe_t euler_roe(const double *ql, const double *qr, int meqn, int mbc, int i, int mu,
                              int mv, double gamma1)
{
    roe_t r;
    double rhsqrtl = sqrt(A2(qr, 1, i - 1));
    double rhsqrtr = sqrt(A2(ql, 1, i));
    double pl = gamma1 * (A2(qr, 4, i - 1) -
                          0.5 * (A2(qr, 2, i - 1) * A2(qr, 2, i - 1) +
                                 A2(qr, 3, i - 1) * A2(qr, 3, i - 1)) / A2(qr, 1, i - 1));
    double pr = gamma1 * (A2(ql, 4, i) -
                          0.5 * (A2(ql, 2, i) * A2(ql, 2, i) + A2(ql, 3, i) * A2(ql, 3, i)) /
                              A2(ql, 1, i));
    double rhsq2 = rhsqrtl + rhsqrtr;
    r.u = (A2(qr, mu, i - 1) / rhsqrtl + A2(ql, mu, i) / rhsqrtr) / rhsq2;
    r.v = (A2(qr, mv, i - 1) / rhsqrtl + A2(ql, mv, i) / rhsqrtr) / rhsq2;
    r.enth = (((A2(qr, 4, i - 1) + pl) / rhsqrtl + (A2(ql, 4, i) + pr) / rhsqrtr)) / rhsq2;
    r.u2v2 = r.u * r.u + r.v * r.v;
    double a2 = gamma1 * (r.enth - .5 * r.u2v2);
    r.a = sqrt(a2);
    r.g1a2 = gamma1 / a2;
    r.euv = r.enth - r.u2v2;
    return r;
}

/* rpn2_euler_5wave.f:5-302, efix = .true.; par = gamma, gamma1 */
static void rpn2_euler5(int ixy, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                        double *wave, double *s, double *amdq, double *apdq,
                        const double *par)
{
    double gamma = par[0], gamma1 = par[1];
    int mu = (ixy == 1) ? 2 : 3, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        roe_t r = euler_roe(ql, qr, meqn, mbc, i, mu, mv, gamma1);
        double u = r.u, v = r.v, enth = r.enth, a = r.a;
        double delta1 = A2(ql, 1, i) - A2(qr, 1, i - 1);
        double delta2 = A2(ql, mu, i) - A2(qr, mu, i - 1);
        double delta3 = A2(ql, mv, i) - A2(qr, mv, i - 1);
        double delta4 = A2(ql, 4, i) - A2(qr, 4, i - 1);
        double a3 = r.g1a2 * (r.euv * delta1 + u * delta2 + v * delta3 - delta4);
        double a2 = delta3 - v * delta1;
        double a4 = (delta2 + (a - u) * delta1 - a * a3) / (2.0 * a);
        double a1 = delta1 - a3 - a4;

        W(1, 1, i) = a1;
        W(mu, 1, i) = a1 * (u - a);
        W(mv, 1, i) = a1 * v;
        W(4, 1, i) = a1 * (enth - u * a);
        W(5, 1, i) = 0.0;
        S(1, i) = u - a;

        W(1, 2, i) = 0.0;
        W(mu, 2, i) = 0.0;
        W(mv, 2, i) = a2;
        W(4, 2, i) = a2 * v;
        W(5, 2, i) = 0.0;
        S(2, i) = u;

        W(1, 3, i) = a3;
        W(mu, 3, i) = a3 * u;
        W(mv, 3, i) = a3 * v;
        W(4, 3, i) = a3 * 0.5 * r.u2v2;
        W(5, 3, i) = 0.0;
        S(3, i) = u;

        W(1, 4, i) = a4;
        W(mu, 4, i) = a4 * (u + a);
        W(mv, 4, i) = a4 * v;
        W(4, 4, i) = a4 * (enth + u * a);
        W(5, 4, i) = 0.0;
        S(4, i) = u + a;

        W(1, 5, i) = 0.0;
        W(mu, 5, i) = 0.0;
        W(mv, 5, i) = 0.0;
        W(4, 5, i) = 0.0;
        W(5, 5, i) = A2(ql, 5, i) - A2(qr, 5, i - 1);
        S(5, i) = u;
    }

    /* entropy fix, rpn2_euler_5wave.f:205-286 */
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double rhoim1 = A2(qr, 1, i - 1);
        double pim1 = gamma1 * (A2(qr, 4, i - 1) -
                                0.5 * (A2(qr, mu, i - 1) * A2(qr, mu, i - 1) +
                                       A2(qr, mv, i - 1) * A2(qr, mv, i - 1)) / rhoim1);
        double cim1 = sqrt(gamma * pim1 / rhoim1);
        double s0 = A2(qr, mu, i - 1) / rhoim1 - cim1;

        if (s0 >= 0.0 && S(1, i) > 0.0) {
            for (int m = 1; m <= meqn; m++) A2(amdq, m, i) = 0.0;
            continue;
        }
        double rho1 = A2(qr, 1, i - 1) + W(1, 1, i);
        double rhou1 = A2(qr, mu, i - 1) + W(mu, 1, i);
        double rhov1 = A2(qr, mv, i - 1) + W(mv, 1, i);
        double en1 = A2(qr, 4, i - 1) + W(4, 1, i);
        double p1 = gamma1 * (en1 - 0.5 * (rhou1 * rhou1 + rhov1 * rhov1) / rho1);
        double c1 = sqrt(gamma * p1 / rho1);
        double s1 = rhou1 / rho1 - c1;
        double sfract;
        if (s0 < 0.0 && s1 > 0.0)
            sfract = s0 * (s1 - S(1, i)) / (s1 - s0);
        else if (S(1, i) < 0.0)
            sfract = S(1, i);
        else
            sfract = 0.0;
        for (int m = 1; m <= meqn; m++) A2(amdq, m, i) = sfract * W(m, 1, i);

        if (S(2, i) >= 0.0) continue;
        for (int m = 1; m <= meqn; m++) {
            A2(amdq, m, i) = A2(amdq, m, i) + S(2, i) * W(m, 2, i);
            A2(amdq, m, i) = A2(amdq, m, i) + S(3, i) * W(m, 3, i);
            A2(amdq, m, i) = A2(amdq, m, i) + S(5, i) * W(m, 5, i);
        }

        double rhoi = A2(ql, 1, i);
        double pi = gamma1 * (A2(ql, 4, i) -
                              0.5 * (A2(ql, mu, i) * A2(ql, mu, i) +
                                     A2(ql, mv, i) * A2(ql, mv, i)) / rhoi);
        double ci = sqrt(gamma * pi / rhoi);
        double s3 = A2(ql, mu, i) / rhoi + ci;

        double rho2 = A2(ql, 1, i) - W(1, 4, i);
        double rhou2 = A2(ql, mu, i) - W(mu, 4, i);
        double rhov2 = A2(ql, mv, i) - W(mv, 4, i);
        double en2 = A2(ql, 4, i) - W(4, 4, i);
        double p2 = gamma1 * (en2 - 0.5 * (rhou2 * rhou2 + rhov2 * rhov2) / rho2);
        double c2 = sqrt(gamma * p2 / rho2);
        double s2 = rhou2 / rho2 + c2;
        if (s2 < 0.0 && s3 > 0.0)
            sfract = s2 * (s3 - S(4, i)) / (s3 - s2);
        else if (S(4, i) < 0.0)
            sfract = S(4, i);
        else
            continue;
        for (int m = 1; m <= meqn; m++)
            A2(amdq, m, i) = A2(amdq, m, i) + sfract * W(m, 4, i);
    }

    for (int m = 1; m <= meqn; m++)
        for (int i = 2 - mbc; i <= mx + mbc; i++) {
            double df = 0.0;
            for (int mw = 1; mw <= mwaves; mw++) df = df + S(mw, i) * W(m, mw, i);
            A2(apdq, m, i) = df - A2(amdq, m, i);
        }
}

/* rpt2_euler_5wave_rec_loc.f:39-118 */
static void rpt2_euler5(int ixy, int meqn, int mbc, int mx, const double *q,
                        const double *asdq, double *bmasdq, double *bpasdq,
                        const double *par)
{
    double gamma1 = par[1];
    int mu = (ixy == 1) ? 2 : 3, mv = (ixy == 1) ? 3 : 2;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        roe_t r = euler_roe(q, q, meqn, mbc, i, mu, mv, gamma1);
        double u = r.u, v = r.v, enth = r.enth, a = r.a;
        double a3 = r.g1a2 * (r.euv * A2(asdq, 1, i) + u * A2(asdq, mu, i) +
                              v * A2(asdq, mv, i) - A2(asdq, 4, i));
        double a2 = A2(asdq, mu, i) - u * A2(asdq, 1, i);
        double a4 = (A2(asdq, mv, i) + (a - v) * A2(asdq, 1, i) - a * a3) / (2.0 * a);
        double a1 = A2(asdq, 1, i) - a3 - a4;
        double waveb[6][5], sb[5];
#define WB(m, mw) waveb[m][mw]
        WB(1, 1) = a1;
        WB(mu, 1) = a1 * u;
        WB(mv, 1) = a1 * (v - a);
        WB(4, 1) = a1 * (enth - v * a);
        WB(5, 1) = 0.0;
        sb[1] = v - a;
        WB(1, 2) = a3;
        WB(mu, 2) = a3 * u + a2;
        WB(mv, 2) = a3 * v;
        WB(4, 2) = a3 * 0.5 * r.u2v2 + a2 * u;
        WB(5, 2) = 0.0;
        sb[2] = v;
        WB(1, 3) = a4;
        WB(mu, 3) = a4 * u;
        WB(mv, 3) = a4 * (v + a);
        WB(4, 3) = a4 * (enth + v * a);
        WB(5, 3) = 0.0;
        sb[3] = v + a;
        WB(1, 4) = 0.0;
        WB(mu, 4) = 0.0;
        WB(mv, 4) = 0.0;
        WB(4, 4) = 0.0;
        WB(5, 4) = A2(asdq, 5, i);
        sb[4] = v;
        for (int m = 1; m <= meqn; m++) {
            double bm = 0.0, bp = 0.0;
            for (int mw = 1; mw <= 4; mw++) {
                bm = bm + dmin(sb[mw], 0.0) * WB(m, mw);
                bp = bp + dmax(sb[mw], 0.0) * WB(m, mw);
            }
            A2(bmasdq, m, i) = bm;
            A2(bpasdq, m, i) = bp;
        }
#undef WB
    }
}

static int rpn2_dispatch(int rp, int ixy, int meqn, int mwaves, int mbc, int mx,
                         const double *ql, const double *qr, double *wave, double *s, double *amdq,
                         double *apdq, const double *par)
{
    switch (rp) {
    case RP_ADVECTION_2D:
        rpn2_advection(ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par);
        return 0;
    case RP_SHALLOW_2D:
        rpn2_shallow(ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par);
        return 0;
    case RP_VC_ACOUSTICS_2D:
        if (!orc_aux1d || orc_maux1d < 2) return -1;
        rpn2_vc_acoustics(ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq);
        return 0;
    case RP_VC_ADVECTION_2D:
        if (!orc_aux1d || orc_maux1d < 2) return -1;
        rpn2_vc_advection(ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq);
        return 0;
    case RP_PSYSTEM_FWAVE_2D:
        if (!orc_aux1d || orc_maux1d < 3 || meqn != 3 || mwaves != 2) return -1;
        rp_fwave_normal(ixy + 1, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq);
        return 0;
    case RP_SHALLOW_SPHERE_2D:
        if (!orc_aux1d || orc_maux1d < 16 || meqn != 4 || mwaves != 3) return -1;
        rpn2_sphere(ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par);
        return 0;
    case RP_ACOUSTICS_2D:
        rpn2_acoustics(ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par);
        return 0;
    case RP_EULER5_2D:
        rpn2_euler5(ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par);
        return 0;
    }
    return -1;
}

static int rpt2_dispatch(int rp, int ixy, int meqn, int mbc, int mx, const double *q,
                         const double *asdq, double *bmasdq, double *bpasdq,
                         const double *par, int imp)
{
    switch (rp) {
    case RP_VC_ACOUSTICS_2D:
        if (!orc_aux1d || !orc_auxb1d || !orc_auxa1d) return -1;
        rpt2_vc_acoustics(ixy, imp, meqn, mbc, mx, asdq, bmasdq, bpasdq);
        return 0;
    case RP_VC_ADVECTION_2D:
        if (!orc_aux1d || !orc_auxa1d) return -1;
        rpt2_vc_advection(ixy, imp, meqn, mbc, mx, asdq, bmasdq, bpasdq);
        return 0;
    case RP_PSYSTEM_FWAVE_2D:
        if (!orc_aux1d || !orc_auxb1d || !orc_auxa1d || orc_maux1d < 4) return -1;
        rpt2_psystem(ixy, imp, meqn, mbc, mx, asdq, bmasdq, bpasdq);
        return 0;
    case RP_SHALLOW_SPHERE_2D:
        if (!orc_aux1d || !orc_auxb1d || !orc_auxa1d) return -1;
        rpt2_sphere(ixy, imp, meqn, mbc, mx, q, asdq, bmasdq, bpasdq, par);
        return 0;
    case RP_ADVECTION_2D:
        rpt2_advection(ixy, meqn, mbc, mx, asdq, bmasdq, bpasdq, par);
        return 0;
    case RP_SHALLOW_2D:
        rpt2_shallow(ixy, meqn, mbc, mx, q, asdq, bmasdq, bpasdq, par);
        return 0;
    case RP_ACOUSTICS_2D:
        rpt2_acoustics(ixy, meqn, mbc, mx, asdq, bmasdq, bpasdq, par);
        return 0;
    case RP_EULER5_2D:
        rpt2_euler5(ixy, meqn, mbc, mx, q, asdq, bmasdq, bpasdq, par);
        return 0;
    }
    return -1;
}

/* ------------------------------------------------------------------ flux2 */
typedef struct {
    double *wave, *s, *amdq, *apdq, *cqxx, *bmasdq, *bpasdq;
    double *q1d, *qadd, *fadd, *gadd, *dtdx1d;
} work_t;

static int work_alloc(work_t *w, int maxm, int mbc, int meqn, int mwaves)
{
    size_t n = (size_t)(maxm + 2 * mbc);
    w->wave = calloc(n * meqn * mwaves, sizeof(double));
    w->s = calloc(n * mwaves, sizeof(double));
    w->amdq = calloc(n * meqn, sizeof(double));
    w->apdq = calloc(n * meqn, sizeof(double));
    w->cqxx = calloc(n * meqn, sizeof(double));
    w->bmasdq = calloc(n * meqn, sizeof(double));
    w->bpasdq = calloc(n * meqn, sizeof(double));
    w->q1d = calloc(n * meqn, sizeof(double));
    w->qadd = calloc(n * meqn, sizeof(double));
    w->fadd = calloc(n * meqn, sizeof(double));
    w->gadd = calloc(n * meqn * 2, sizeof(double));
    w->dtdx1d = calloc(n, sizeof(double));
    return 0;
}
static void work_free(work_t *w)
{
    free(w->wave); free(w->s); free(w->amdq); free(w->apdq); free(w->cqxx);
    free(w->bmasdq); free(w->bpasdq); free(w->q1d); free(w->qadd); free(w->fadd);
    free(w->gadd); free(w->dtdx1d);
}

#define GADD(m, k, i) gadd[((m)-1) + meqn * (((k)-1) + 2 * IX(i))]

/* flux2.f:80-191; fwave selects flux2fw.f:151-152 */
static int flux2(int rp, const double *par, int fwave, int ixy, int meqn, int mwaves,
                 int mbc, int mx, const int *method, const int *mthlim, work_t *w,
                 double *cfl1d_out)
{
    double *wave = w->wave, *s = w->s, *amdq = w->amdq, *apdq = w->apdq;
    double *cqxx = w->cqxx, *bmasdq = w->bmasdq, *bpasdq = w->bpasdq;
    double *q1d = w->q1d, *qadd = w->qadd, *fadd = w->fadd, *gadd = w->gadd;
    double *dtdx1d = w->dtdx1d;
#define DT(i) dtdx1d[IX(i)]
    int limit = 0;
    for (int mw = 0; mw < mwaves; mw++)
        if (mthlim[mw] > 0) limit = 1;

    for (int i = 1 - mbc; i <= mx + mbc; i++)
        for (int m = 1; m <= meqn; m++) {
            A2(qadd, m, i) = 0.0;
            A2(fadd, m, i) = 0.0;
            GADD(m, 1, i) = 0.0;
            GADD(m, 2, i) = 0.0;
        }

    if (rpn2_dispatch(rp, ixy, meqn, mwaves, mbc, mx, q1d, q1d, wave, s, amdq, apdq, par))
        return -1;

    /* forall semantics (flux2.f:103-106): all apdq updates, then all amdq updates */
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++)
            A2(qadd, m, i) = A2(qadd, m, i) - DT(i) * A2(apdq, m, i);
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++)
            A2(qadd, m, i - 1) = A2(qadd, m, i - 1) - DT(i - 1) * A2(amdq, m, i);

    double cfl1d = 0.0;
    for (int mw = 1; mw <= mwaves; mw++)
        for (int i = 1; i <= mx + 1; i++)
            cfl1d = dmax(dmax(cfl1d, DT(i) * S(mw, i)), -DT(i - 1) * S(mw, i));
    *cfl1d_out = cfl1d;

    if (method[1] != 1) {
        if (limit) limiter(meqn, mwaves, mbc, mx, wave, s, mthlim);
        for (int i = 2 - mbc; i <= mx + mbc; i++) {
            double dtdxave = 0.5 * (DT(i - 1) + DT(i));
            for (int m = 1; m <= meqn; m++) {
                double c = 0.0;
                for (int mw = 1; mw <= mwaves; mw++) {
                    double sa = fabs(S(mw, i));
                    if (fwave)
                        c = c + copysign(1.0, S(mw, i)) * (1.0 - sa * dtdxave) * W(m, mw, i);
                    else
                        c = c + sa * (1.0 - sa * dtdxave) * W(m, mw, i);
                }
                A2(cqxx, m, i) = c;
                A2(fadd, m, i) = A2(fadd, m, i) + 0.5 * c;
            }
        }
    }

    if (method[2] <= 0) return 0;

    if (method[1] > 1 && method[2] == 2)
        for (int i = 1; i <= mx + 1; i++)
            for (int m = 1; m <= meqn; m++) {
                A2(amdq, m, i) = A2(amdq, m, i) + A2(cqxx, m, i);
                A2(apdq, m, i) = A2(apdq, m, i) - A2(cqxx, m, i);
            }

    if (rpt2_dispatch(rp, ixy, meqn, mbc, mx, q1d, amdq, bmasdq, bpasdq, par, 1)) return -1;
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) {
            GADD(m, 1, i - 1) = GADD(m, 1, i - 1) - 0.5 * DT(i - 1) * A2(bmasdq, m, i);
            GADD(m, 2, i - 1) = GADD(m, 2, i - 1) - 0.5 * DT(i - 1) * A2(bpasdq, m, i);
        }
    if (rpt2_dispatch(rp, ixy, meqn, mbc, mx, q1d, apdq, bmasdq, bpasdq, par, 2)) return -1;
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) {
            GADD(m, 1, i) = GADD(m, 1, i) - 0.5 * DT(i) * A2(bmasdq, m, i);
            GADD(m, 2, i) = GADD(m, 2, i) - 0.5 * DT(i) * A2(bpasdq, m, i);
        }
    return 0;
#undef DT
}

/* 3-index accessors on the full grid */
#define Q3(arr, m, i, j) \
    arr[((m)-1) + (size_t)meqn * (((i) + mbc - 1) + (size_t)(mx + 2 * mbc) * ((j) + mbc - 1))]
#define AUX3(ma, i, j) \
    aux[((ma)-1) + (size_t)maux * (((i) + mbc - 1) + (size_t)(mx + 2 * mbc) * ((j) + mbc - 1))]

/* ---------------------------------------------------------------- step2ds */
/* step2ds.f:64-244.  qold may alias qnew (second call of the dim-split step). */
int orc_step2ds(int rp, const double *par, int fwave, int maxm, int meqn, int mwaves,
                int maux, int mbc, int mx, int my, const double *qold, double *qnew,
                const double *aux, double dx, double dy, double dt, const int *method,
                const int *mthlim, double *cfl_out, int ids)
{
    work_t w;
    work_alloc(&w, maxm, mbc, meqn, mwaves);
    double *q1d = w.q1d, *qadd = w.qadd, *fadd = w.fadd, *dtdx1d = w.dtdx1d;
    int mcapa = method[5];
    double cfl = 0.0, cfl1d;
    double dtdx = dt / dx, dtdy = dt / dy;
    int rc = 0;
    double *aux1d = calloc((size_t)(maxm + 2 * mbc) * (maux > 0 ? maux : 1), sizeof(double));
    orc_aux1d = aux1d;
    orc_maux1d = maux;

    if (ids == 1) {
        if (mcapa == 0)
            for (int i = 1 - mbc; i <= maxm + mbc; i++) dtdx1d[IX(i)] = dtdx;
        for (int j = 1 - mbc; j <= my + mbc; j++) {
            for (int i = 1 - mbc; i <= mx + mbc; i++)
                for (int m = 1; m <= meqn; m++) A2(q1d, m, i) = Q3(qold, m, i, j);
            if (mcapa > 0)
                for (int i = 1 - mbc; i <= mx + mbc; i++)
                    dtdx1d[IX(i)] = dtdx / AUX3(mcapa, i, j);
            for (int i = 1 - mbc; i <= mx + mbc; i++)
                for (int ma = 1; ma <= maux; ma++) aux1d[(ma - 1) + maux * IX(i)] = AUX3(ma, i, j);
            rc |= flux2(rp, par, fwave, 1, meqn, mwaves, mbc, mx, method, mthlim, &w, &cfl1d);
            cfl = dmax(cfl, cfl1d);
            if (mcapa == 0) {
                for (int i = 1; i <= mx; i++)
                    for (int m = 1; m <= meqn; m++)
                        Q3(qnew, m, i, j) = Q3(qnew, m, i, j) + A2(qadd, m, i) -
                                            dtdx * (A2(fadd, m, i + 1) - A2(fadd, m, i));
            } else {
                for (int i = 1; i <= mx; i++)
                    for (int m = 1; m <= meqn; m++)
                        Q3(qnew, m, i, j) = Q3(qnew, m, i, j) + A2(qadd, m, i) -
                                            dtdx * (A2(fadd, m, i + 1) - A2(fadd, m, i)) /
                                                AUX3(mcapa, i, j);
            }
        }
    } else {
        if (mcapa == 0)
            for (int i = 1 - mbc; i <= maxm + mbc; i++) dtdx1d[IX(i)] = dtdy;
        for (int i = 1 - mbc; i <= mx + mbc; i++) {
            for (int j = 1 - mbc; j <= my + mbc; j++)
                for (int m = 1; m <= meqn; m++) A2(q1d, m, j) = Q3(qold, m, i, j);
            if (mcapa > 0)
                for (int j = 1 - mbc; j <= my + mbc; j++)
                    dtdx1d[IX(j)] = dtdy / AUX3(mcapa, i, j);
            for (int j = 1 - mbc; j <= my + mbc; j++)
                for (int ma = 1; ma <= maux; ma++) aux1d[(ma - 1) + maux * IX(j)] = AUX3(ma, i, j);
            rc |= flux2(rp, par, fwave, 2, meqn, mwaves, mbc, my, method, mthlim, &w, &cfl1d);
            cfl = dmax(cfl, cfl1d);
            if (mcapa == 0) {
                for (int j = 1; j <= my; j++)
                    for (int m = 1; m <= meqn; m++)
                        Q3(qnew, m, i, j) = Q3(qnew, m, i, j) + A2(qadd, m, j) -
                                            dtdy * (A2(fadd, m, j + 1) - A2(fadd, m, j));
            } else {
                for (int j = 1; j <= my; j++)
                    for (int m = 1; m <= meqn; m++)
                        Q3(qnew, m, i, j) = Q3(qnew, m, i, j) + A2(qadd, m, j) -
                                            dtdy * (A2(fadd, m, j + 1) - A2(fadd, m, j)) /
                                                AUX3(mcapa, i, j);
            }
        }
    }
    *cfl_out = cfl;
    orc_aux1d = NULL;
    free(aux1d);
    work_free(&w);
    return rc;
}

/* ------------------------------------------------------------------ step2 */
/* step2.f:66-238 (unsplit, with transverse corrections through gadd) */
int orc_step2(int rp, const double *par, int fwave, int maxm, int meqn, int mwaves,
              int maux, int mbc, int mx, int my, const double *qold, double *qnew,
              const double *aux, double dx, double dy, double dt, const int *method,
              const int *mthlim, double *cfl_out)
{
    work_t w;
    work_alloc(&w, maxm, mbc, meqn, mwaves);
    double *q1d = w.q1d, *qadd = w.qadd, *fadd = w.fadd, *gadd = w.gadd;
    double *dtdx1d = w.dtdx1d;
    int mcapa = method[5];
    double cfl = 0.0, cfl1d;
    double dtdx = dt / dx, dtdy = dt / dy;
    int rc = 0;
    const size_t nal = (size_t)(maxm + 2 * mbc) * (maux > 0 ? maux : 1);
    double *aux1d = calloc(nal, sizeof(double)), *auxb = calloc(nal, sizeof(double)), *auxa = calloc(nal, sizeof(double));
    orc_aux1d = aux1d; orc_auxb1d = auxb; orc_auxa1d = auxa; orc_maux1d = maux;

    /* x sweeps */
    if (mcapa == 0)
        for (int i = 1 - mbc; i <= maxm + mbc; i++) dtdx1d[IX(i)] = dtdx;
    for (int j = 0; j <= my + 1; j++) {
        for (int m = 1; m <= meqn; m++)
            for (int i = 1 - mbc; i <= mx + mbc; i++) A2(q1d, m, i) = Q3(qold, m, i, j);
        if (mcapa > 0)
            for (int i = 1 - mbc; i <= mx + mbc; i++) dtdx1d[IX(i)] = dtdx / AUX3(mcapa, i, j);
        for (int i = 1 - mbc; i <= mx + mbc; i++)        /* step2.f:97-101: aux rows j-1, j, j+1 */
            for (int ma = 1; ma <= maux; ma++) {
                auxb[(ma - 1) + maux * IX(i)] = AUX3(ma, i, j - 1);
                aux1d[(ma - 1) + maux * IX(i)] = AUX3(ma, i, j);
                auxa[(ma - 1) + maux * IX(i)] = AUX3(ma, i, j + 1);
            }
        rc |= flux2(rp, par, fwave, 1, meqn, mwaves, mbc, mx, method, mthlim, &w, &cfl1d);
        cfl = dmax(cfl, cfl1d);
        if (mcapa == 0) {
            for (int m = 1; m <= meqn; m++)
                for (int i = 1; i <= mx; i++) {
                    Q3(qnew, m, i, j) = Q3(qnew, m, i, j) + A2(qadd, m, i) -
                                        dtdx * (A2(fadd, m, i + 1) - A2(fadd, m, i)) -
                                        dtdy * (GADD(m, 2, i) - GADD(m, 1, i));
                    Q3(qnew, m, i, j - 1) = Q3(qnew, m, i, j - 1) - dtdy * GADD(m, 1, i);
                    Q3(qnew, m, i, j + 1) = Q3(qnew, m, i, j + 1) + dtdy * GADD(m, 2, i);
                }
        } else {
            for (int m = 1; m <= meqn; m++)
                for (int i = 1; i <= mx; i++) {
                    Q3(qnew, m, i, j) = Q3(qnew, m, i, j) + A2(qadd, m, i) -
                                        (dtdx * (A2(fadd, m, i + 1) - A2(fadd, m, i)) +
                                         dtdy * (GADD(m, 2, i) - GADD(m, 1, i))) /
                                            AUX3(mcapa, i, j);
                    Q3(qnew, m, i, j - 1) = Q3(qnew, m, i, j - 1) -
                                            dtdy * GADD(m, 1, i) / AUX3(mcapa, i, j - 1);
                    Q3(qnew, m, i, j + 1) = Q3(qnew, m, i, j + 1) +
                                            dtdy * GADD(m, 2, i) / AUX3(mcapa, i, j + 1);
                }
            if (orc_qcor_on)        /* step2qcor.f:146-159: qnew(m,i,j) -= dtdx*qc(m)/capa, right after the cell's own update */
                for (int i = 1; i <= mx; i++) {
                    double qc[5];
                    sphere_qcor(1, i, aux1d, maux, q1d, meqn, mbc, par, qc);
                    for (int m = 1; m <= meqn; m++)
                        Q3(qnew, m, i, j) = Q3(qnew, m, i, j) - dtdx * qc[m] / AUX3(mcapa, i, j);
                }
        }
    }

    /* y sweeps */
    if (mcapa == 0)
        for (int i = 1 - mbc; i <= maxm + mbc; i++) dtdx1d[IX(i)] = dtdy;
    for (int i = 0; i <= mx + 1; i++) {
        for (int m = 1; m <= meqn; m++)
            for (int j = 1 - mbc; j <= my + mbc; j++) A2(q1d, m, j) = Q3(qold, m, i, j);
        if (mcapa > 0)
            for (int j = 1 - mbc; j <= my + mbc; j++) dtdx1d[IX(j)] = dtdy / AUX3(mcapa, i, j);
        for (int j = 1 - mbc; j <= my + mbc; j++)        /* step2.f:177-181: aux columns i-1, i, i+1 */
            for (int ma = 1; ma <= maux; ma++) {
                auxb[(ma - 1) + maux * IX(j)] = AUX3(ma, i - 1, j);
                aux1d[(ma - 1) + maux * IX(j)] = AUX3(ma, i, j);
                auxa[(ma - 1) + maux * IX(j)] = AUX3(ma, i + 1, j);
            }
        rc |= flux2(rp, par, fwave, 2, meqn, mwaves, mbc, my, method, mthlim, &w, &cfl1d);
        cfl = dmax(cfl, cfl1d);
        if (mcapa == 0) {
            for (int m = 1; m <= meqn; m++)
                for (int j = 1; j <= my; j++) {
                    Q3(qnew, m, i, j) = Q3(qnew, m, i, j) +
                                        (A2(qadd, m, j) -
                                         dtdy * (A2(fadd, m, j + 1) - A2(fadd, m, j)) -
                                         dtdx * (GADD(m, 2, j) - GADD(m, 1, j)));
                    Q3(qnew, m, i - 1, j) = Q3(qnew, m, i - 1, j) - dtdx * GADD(m, 1, j);
                    Q3(qnew, m, i + 1, j) = Q3(qnew, m, i + 1, j) + dtdx * GADD(m, 2, j);
                }
        } else {
            for (int m = 1; m <= meqn; m++)
                for (int j = 1; j <= my; j++) {
                    Q3(qnew, m, i, j) = Q3(qnew, m, i, j) + A2(qadd, m, j) -
                                        (dtdy * (A2(fadd, m, j + 1) - A2(fadd, m, j)) +
                                         dtdx * (GADD(m, 2, j) - GADD(m, 1, j))) /
                                            AUX3(mcapa, i, j);
                    Q3(qnew, m, i - 1, j) = Q3(qnew, m, i - 1, j) -
                                            dtdx * GADD(m, 1, j) / AUX3(mcapa, i - 1, j);
                    Q3(qnew, m, i + 1, j) = Q3(qnew, m, i + 1, j) +
                                            dtdx * GADD(m, 2, j) / AUX3(mcapa, i + 1, j);
                }
            if (orc_qcor_on)        /* step2qcor.f:232-245 */
                for (int j = 1; j <= my; j++) {
                    double qc[5];
                    sphere_qcor(2, j, aux1d, maux, q1d, meqn, mbc, par, qc);
                    for (int m = 1; m <= meqn; m++)
                        Q3(qnew, m, i, j) = Q3(qnew, m, i, j) - dtdy * qc[m] / AUX3(mcapa, i, j);
                }
        }
    }
    *cfl_out = cfl;
    orc_aux1d = orc_auxb1d = orc_auxa1d = NULL;
    free(aux1d); free(auxb); free(auxa);
    work_free(&w);
    return rc;
}

/* ------------------------------------------------------------------ step1 */
/* step1.f:55-139 ; q updated in place, aux(maux, 1-mbc:mx+mbc) */
static int step1_body(int rp, const double *par, int meqn, int mwaves, int maux, int mbc, int mx,
                      double *q, const double *aux, double dx, double dt, const int *method,
                      const int *mthlim, double *cfl_out, int fwave);
int orc_step1(int rp, const double *par, int meqn, int mwaves, int maux, int mbc, int mx,
              double *q, const double *aux, double dx, double dt, const int *method,
              const int *mthlim, double *cfl_out)
{
    return step1_body(rp, par, meqn, mwaves, maux, mbc, mx, q, aux, dx, dt, method, mthlim, cfl_out, 0);
}
/* step1fw.f:62-156: the f-wave twin (classic1fw): limiter on the f-waves, correction 0.5*dsign(1,s)*(1-|s|dtdxave)*fwave
 * (:139-140), final flux differencing over cells 1..mx (:151-154; step1.f runs 1..mx+1, a ghost cell) */
int orc_step1fw(int rp, const double *par, int meqn, int mwaves, int maux, int mbc, int mx,
                double *q, const double *aux, double dx, double dt, const int *method,
                const int *mthlim, double *cfl_out)
{
    return step1_body(rp, par, meqn, mwaves, maux, mbc, mx, q, aux, dx, dt, method, mthlim, cfl_out, 1);
}
static int step1_body(int rp, const double *par, int meqn, int mwaves, int maux, int mbc, int mx,
                      double *q, const double *aux, double dx, double dt, const int *method,
                      const int *mthlim, double *cfl_out, int fwave)
{
    size_t n = (size_t)(mx + 2 * mbc);
    double *wave = calloc(n * meqn * mwaves, sizeof(double));
    double *s = calloc(n * mwaves, sizeof(double));
    double *amdq = calloc(n * meqn, sizeof(double));
    double *apdq = calloc(n * meqn, sizeof(double));
    double *f = calloc(n * meqn, sizeof(double));
    double *dtdx = calloc(n, sizeof(double));
#define DT(i) dtdx[IX(i)]
    int limit = 0, rc = 0;
    for (int mw = 0; mw < mwaves; mw++)
        if (mthlim[mw] > 0) limit = 1;
    int mcapa = method[5];
    for (int i = 1 - mbc; i <= mx + mbc; i++) {
        if (mcapa > 0)
            DT(i) = dt / (dx * aux[(mcapa - 1) + (size_t)maux * IX(i)]);
        else
            DT(i) = dt / dx;
    }
    switch (rp) {
    case RP_ADVECTION_1D: rp1_advection(meqn, mwaves, mbc, mx, q, q, wave, s, amdq, apdq, par); break;
    case RP_ACOUSTICS_1D: rp1_acoustics(meqn, mwaves, mbc, mx, q, q, wave, s, amdq, apdq, par); break;
    case RP_BURGERS_1D: rp1_burgers(meqn, mwaves, mbc, mx, q, q, wave, s, amdq, apdq, par); break;
    case RP_EULER_1D: rp1_euler(meqn, mwaves, mbc, mx, q, q, wave, s, amdq, apdq, par); break;
    case RP_SHALLOW_1D: rp1_shallow(meqn, mwaves, mbc, mx, q, q, wave, s, amdq, apdq, par); break;
    case RP_ADVECTION_COLOR_1D:
        orc_aux1d = aux; orc_maux1d = maux;       /* step1.f:78: rp1(..., q, q, aux, aux, ...) */
        rp1_advection_color(meqn, mwaves, mbc, mx, q, q, wave, s, amdq, apdq);
        orc_aux1d = NULL;
        break;
    case RP_ELASTICITY_FWAVE_1D:
        if (!fwave || maux < 3 || meqn != 2 || mwaves != 2) { rc = -1; break; }
        orc_aux1d = aux; orc_maux1d = maux;
        rp_fwave_normal(2, meqn, mwaves, mbc, mx, q, q, wave, s, amdq, apdq);
        orc_aux1d = NULL;
        break;
    default: rc = -1;
    }
    if (fwave && rp != RP_ELASTICITY_FWAVE_1D) rc = -1;
    if (!rc) {
        for (int i = 1; i <= mx + 1; i++)
            for (int m = 1; m <= meqn; m++)
                A2(q, m, i) = A2(q, m, i) - DT(i) * A2(apdq, m, i);
        for (int i = 1; i <= mx + 1; i++)
            for (int m = 1; m <= meqn; m++)
                A2(q, m, i - 1) = A2(q, m, i - 1) - DT(i - 1) * A2(amdq, m, i);
        double cfl = 0.0;
        for (int mw = 1; mw <= mwaves; mw++)
            for (int i = 1; i <= mx + 1; i++)
                cfl = dmax(dmax(cfl, DT(i) * S(mw, i)), -DT(i - 1) * S(mw, i));
        *cfl_out = cfl;
        if (method[1] != 1) {
            if (limit) limiter(meqn, mwaves, mbc, mx, wave, s, mthlim);
            for (int i = 1; i <= mx + 1; i++)
                for (int m = 1; m <= meqn; m++)
                    for (int mw = 1; mw <= mwaves; mw++) {
                        double dtdxave = 0.5 * (DT(i - 1) + DT(i));
                        double sa = fabs(S(mw, i));
                        if (fwave)
                            A2(f, m, i) = A2(f, m, i) +
                                          0.5 * copysign(1.0, S(mw, i)) * (1.0 - sa * dtdxave) * W(m, mw, i);
                        else
                            A2(f, m, i) = A2(f, m, i) +
                                          0.5 * sa * (1.0 - sa * dtdxave) * W(m, mw, i);
                    }
            for (int i = 1; i <= (fwave ? mx : mx + 1); i++)
                for (int m = 1; m <= meqn; m++)
                    A2(q, m, i) = A2(q, m, i) - DT(i) * (A2(f, m, i + 1) - A2(f, m, i));
        }
    }
#undef DT
    free(wave); free(s); free(amdq); free(apdq); free(f); free(dtdx);
    return rc;
}

/* Direct access to the slice-level pieces, for unit-level parity tests. */
int orc_rpn2(int rp, const double *par, int ixy, int meqn, int mwaves, int mbc, int mx,
             const double *q1d, double *wave, double *s, double *amdq, double *apdq)
{
    return rpn2_dispatch(rp, ixy, meqn, mwaves, mbc, mx, q1d, q1d, wave, s, amdq, apdq, par);
}

/* separate edge states (SharpClaw: ql/qr from the reconstruction) */
int orc_rpn2_ptr(int rp, const double *par, int ixy, int meqn, int mwaves, int mbc, int mx,
                 const double *ql, const double *qr, double *wave, double *s, double *amdq, double *apdq)
{
    return rpn2_dispatch(rp, ixy, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par);
}

int orc_rp1_ptr(int rp, const double *par, int meqn, int mwaves, int mbc, int mx, const double *ql,
                const double *qr, double *wave, double *s, double *amdq, double *apdq)
{
    switch (rp) {
    case RP_ADVECTION_1D: rp1_advection(meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par); return 0;
    case RP_ACOUSTICS_1D: rp1_acoustics(meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par); return 0;
    case RP_BURGERS_1D: rp1_burgers(meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par); return 0;
    case RP_EULER_1D: rp1_euler(meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par); return 0;
    case RP_SHALLOW_1D: rp1_shallow(meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq, par); return 0;
    case RP_ADVECTION_COLOR_1D:
        if (!orc_aux1d || orc_maux1d < 1) return -1;
        rp1_advection_color(meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq);
        return 0;
    }
    return -1;
}

/* qcor.f through the C ABI (tests): aux1d(16, maxm+2mbc), q1d(meqn, maxm+2mbc), Fortran cell index i; qc4[4] */
void orc_sphere_qcor(int ixy, int i, const double *aux1d, const double *q1d, int meqn, int mbc, const double *par,
                     double *qc4)
{
    double qc[5];
    sphere_qcor(ixy, i, aux1d, 16, q1d, meqn, mbc, par, qc);
    for (int m = 0; m < 4; m++) qc4[m] = qc[m + 1];
}

int orc_rpt2(int rp, const double *par, int ixy, int meqn, int mbc, int mx,
             const double *q1d, const double *asdq, double *bmasdq, double *bpasdq)
{
    return rpt2_dispatch(rp, ixy, meqn, mbc, mx, q1d, asdq, bmasdq, bpasdq, par, 1);
}

void orc_limiter(int meqn, int mwaves, int mbc, int mx, double *wave, const double *s,
                 const int *mthlim)
{
    limiter(meqn, mwaves, mbc, mx, wave, s, mthlim);
}

double orc_philim(double a, double b, int meth) { return philim(a, b, meth); }


/* ======================================================================== 3-D, dimension split */
/* variable-coefficient acoustics in 3-D, restated (third-party rpn3_vc_acoustics.f):
 * q = (p,u,v,w); aux(1) = impedance Z, aux(2) = sound speed c of each cell; two waves. */
static void rpn3_vc_acoustics(int ixyz, int meqn, int mwaves, int maux, int mbc, int mx,
                              const double *ql, const double *qr, const double *auxl, const double *auxr,
                              double *wave, double *s, double *amdq, double *apdq)
{
#define AX(arr, ma, i) arr[((ma)-1) + maux * IX(i)]
    int mu = ixyz + 1;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        double d1 = A2(ql, 1, i) - A2(qr, 1, i - 1);
        double d2 = A2(ql, mu, i) - A2(qr, mu, i - 1);
        double zi = AX(auxl, 1, i), zim = AX(auxr, 1, i - 1);
        double a1 = (-d1 + zi * d2) / (zim + zi);
        double a2 = (d1 + zim * d2) / (zim + zi);
        for (int m = 1; m <= meqn; m++) { W(m, 1, i) = 0.0; W(m, 2, i) = 0.0; }
        W(1, 1, i) = -a1 * zim;
        W(mu, 1, i) = a1;
        S(1, i) = -AX(auxr, 2, i - 1);
        W(1, 2, i) = a2 * zi;
        W(mu, 2, i) = a2;
        S(2, i) = AX(auxl, 2, i);
    }
    for (int m = 1; m <= meqn; m++)
        for (int i = 2 - mbc; i <= mx + mbc; i++) {
            A2(amdq, m, i) = S(1, i) * W(m, 1, i);
            A2(apdq, m, i) = S(2, i) * W(m, 2, i);
        }
#undef AX
}

/* flux3.f:168-258 with method(3) < 0 (m3 = -1: returns before the transverse part).
 * aux1d = aux2(:, :, 2) of the caller: the slice's own aux values. */
static int flux3_split(int rp, int ixyz, int meqn, int mwaves, int maux, int mbc, int mx,
                       const int *method, const int *mthlim, work_t *w, const double *aux1d,
                       double *cfl1d_out)
{
    double *wave = w->wave, *s = w->s, *amdq = w->amdq, *apdq = w->apdq, *cqxx = w->cqxx;
    double *q1d = w->q1d, *qadd = w->qadd, *fadd = w->fadd, *dtdx1d = w->dtdx1d;
#define DT(i) dtdx1d[IX(i)]
    int limit = 0;
    for (int mw = 0; mw < mwaves; mw++)
        if (mthlim[mw] > 0) limit = 1;
    for (int i = 1 - mbc; i <= mx + mbc; i++)
        for (int m = 1; m <= meqn; m++) { A2(qadd, m, i) = 0.0; A2(fadd, m, i) = 0.0; }
    if (rp != RP_VC_ACOUSTICS_3D) return -1;
    rpn3_vc_acoustics(ixyz, meqn, mwaves, maux, mbc, mx, q1d, q1d, aux1d, aux1d, wave, s, amdq, apdq);
    /* forall, flux3.f:205-208: all apdq terms, then all amdq terms */
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) A2(qadd, m, i) = A2(qadd, m, i) - DT(i) * A2(apdq, m, i);
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) A2(qadd, m, i - 1) = A2(qadd, m, i - 1) - DT(i - 1) * A2(amdq, m, i);
    double cfl1d = 0.0;
    for (int i = 1; i <= mx + 1; i++)
        for (int mw = 1; mw <= mwaves; mw++)
            cfl1d = dmax(dmax(cfl1d, DT(i) * S(mw, i)), -DT(i - 1) * S(mw, i));
    *cfl1d_out = cfl1d;
    if (method[1] != 1) {
        if (limit) limiter(meqn, mwaves, mbc, mx, wave, s, mthlim);
        for (int i = 2 - mbc; i <= mx + mbc; i++) {
            double dtdxave = 0.5 * (DT(i - 1) + DT(i));
            for (int m = 1; m <= meqn; m++) A2(cqxx, m, i) = 0.0;
            for (int mw = 1; mw <= mwaves; mw++)
                for (int m = 1; m <= meqn; m++)   /* flux3.f:244-247: 0.5 inside every term */
                    A2(cqxx, m, i) = A2(cqxx, m, i) +
                                     0.5 * fabs(S(mw, i)) * (1.0 - fabs(S(mw, i)) * dtdxave) * W(m, mw, i);
            for (int m = 1; m <= meqn; m++) A2(fadd, m, i) = A2(fadd, m, i) + A2(cqxx, m, i);
        }
    }
    if (method[2] >= 0) return -2;   /* unsplit 3-D (rpt3/rptt3) is not restated */
    return 0;
#undef DT
}

#define Q4(arr, m, i, j, k)                                                                            \
    arr[((m)-1) + (size_t)meqn * (((i) + mbc - 1) + (size_t)(mx + 2 * mbc) * (((j) + mbc - 1) +          \
                                                      (size_t)(my + 2 * mbc) * ((k) + mbc - 1)))]
#define AUX4(ma, i, j, k)                                                                              \
    aux[((ma)-1) + (size_t)maux * (((i) + mbc - 1) + (size_t)(mx + 2 * mbc) * (((j) + mbc - 1) +         \
                                                      (size_t)(my + 2 * mbc) * ((k) + mbc - 1)))]

/* step3ds.f:108-374.  qold may alias qnew (2nd and 3rd call of the dim-split step, clawpack.py:682-688). */
int orc_step3ds(int rp, int maxm, int meqn, int mwaves, int maux, int mbc, int mx, int my, int mz,
                const double *qold, double *qnew, const double *aux, double dx, double dy, double dz,
                double dt, const int *method, const int *mthlim, double *cfl_out, int idir)
{
    work_t w;
    work_alloc(&w, maxm, mbc, meqn, mwaves);
    double *q1d = w.q1d, *qadd = w.qadd, *fadd = w.fadd, *dtdx1d = w.dtdx1d;
    double *aux1d = calloc((size_t)(maxm + 2 * mbc) * (maux > 0 ? maux : 1), sizeof(double));
    int mcapa = method[5];
    double cfl = 0.0, cfl1d = 0.0;
    const double dtd[3] = {dt / dx, dt / dy, dt / dz};
    const int n[3] = {mx, my, mz};
    int rc = 0;
    const int d = idir - 1, nd = n[d];
    /* the two transverse directions (outer, inner loop of the Fortran): x: k,j   y: k,i   z: j,i */
    const int o = idir == 3 ? 1 : 2, in = idir == 1 ? 1 : 0;
    if (mcapa == 0)
        for (int i = 1 - mbc; i <= maxm + mbc; i++) dtdx1d[IX(i)] = dtd[d];
    for (int a = 0; a <= n[o] + 1; a++)
        for (int b = 0; b <= n[in] + 1; b++) {
            int c[3];
#define CELL(t) (c[d] = (t), c[o] = a, c[in] = b)
            for (int t = 1 - mbc; t <= nd + mbc; t++) {
                CELL(t);
                for (int m = 1; m <= meqn; m++) A2(q1d, m, t) = Q4(qold, m, c[0], c[1], c[2]);
                if (mcapa > 0) dtdx1d[IX(t)] = dtd[d] / AUX4(mcapa, c[0], c[1], c[2]);
                for (int ma = 1; ma <= maux; ma++) aux1d[(ma - 1) + maux * IX(t)] = AUX4(ma, c[0], c[1], c[2]);
            }
            int r = flux3_split(rp, idir, meqn, mwaves, maux, mbc, nd, method, mthlim, &w, aux1d, &cfl1d);
            if (r) rc = r;
            cfl = dmax(cfl, cfl1d);
            for (int t = 1; t <= nd; t++) {
                CELL(t);
                for (int m = 1; m <= meqn; m++) {
                    if (mcapa == 0)
                        Q4(qnew, m, c[0], c[1], c[2]) = Q4(qnew, m, c[0], c[1], c[2]) + A2(qadd, m, t) -
                                                        dtd[d] * (A2(fadd, m, t + 1) - A2(fadd, m, t));
                    else
                        Q4(qnew, m, c[0], c[1], c[2]) = Q4(qnew, m, c[0], c[1], c[2]) + A2(qadd, m, t) -
                                                        dtd[d] * (A2(fadd, m, t + 1) - A2(fadd, m, t)) /
                                                            AUX4(mcapa, c[0], c[1], c[2]);
                }
            }
#undef CELL
        }
    *cfl_out = cfl;
    free(aux1d);
    work_free(&w);
    return rc;
}

/* ======================================================================== 3-D, unsplit (step3.f + flux3.f) */
/* Transverse solvers of the variable-coefficient acoustics equations in 3-D, restated (THIRD-PARTY
 * rpt3_vc_acoustics.f / rptt3_vc_acoustics.f, named by test/acoustics/3d/Makefile:3, absent from the reference tree).
 * Pinned through the reference's golden test/pressure_3D.txt (test_3D_acoustics_heterogeneous, gate 2-norm < 1e-4,
 * test/test_examples.py:497-514): tests/test_classic3d_unsplit.py.
 * auxN(ma, i, kk): N = 1,2,3 <-> the row below / at / above the slice in the y-like direction, kk = 1,2,3 <-> below /
 * at / above in the z-like direction (step3.f:130-142, 253-260, 445-456).  asdq sits in cell i1 = i-2+imp.
 * The part going down enters the neighbouring row with ITS sound speed and impedance, like the 2-D solver. */
#define AX3(arr, ma, i, kk) arr[((ma)-1) + (size_t)maux * (IX(i) + (size_t)nrow * ((kk)-1))]
static void rpt3_vc_acoustics(int ixyz, int icoor, int meqn, int maux, int mbc, int mx, int nrow,
                              const double *aux1, const double *aux2, const double *aux3, int imp,
                              const double *asdq, double *bmasdq, double *bpasdq)
{
    int iuvw = ixyz + icoor - 1;
    if (iuvw > 3) iuvw = iuvw - 3;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const int i1 = i - 2 + imp;
        double zm, zz, zp, cm, cp;
        if (icoor == 2) {
            zm = AX3(aux1, 1, i1, 2); zz = AX3(aux2, 1, i1, 2); zp = AX3(aux3, 1, i1, 2);
            cm = AX3(aux1, 2, i1, 2); cp = AX3(aux3, 2, i1, 2);
        } else {
            zm = AX3(aux2, 1, i1, 1); zz = AX3(aux2, 1, i1, 2); zp = AX3(aux2, 1, i1, 3);
            cm = AX3(aux2, 2, i1, 1); cp = AX3(aux2, 2, i1, 3);
        }
        const double a1 = (-A2(asdq, 1, i) + A2(asdq, iuvw + 1, i) * zz) / (zm + zz);
        const double a2 = (A2(asdq, 1, i) + A2(asdq, iuvw + 1, i) * zz) / (zz + zp);
        for (int m = 1; m <= meqn; m++) { A2(bmasdq, m, i) = 0.0; A2(bpasdq, m, i) = 0.0; }
        A2(bmasdq, 1, i) = cm * a1 * zm;
        A2(bmasdq, iuvw + 1, i) = -cm * a1;
        A2(bpasdq, 1, i) = cp * a2 * zp;
        A2(bpasdq, iuvw + 1, i) = cp * a2;
    }
}
/* double-transverse: bsasdq came out of a transverse solve that went down (impt = 1) or up (impt = 2) in the OTHER
 * transverse direction, so the three rows of the new split lie in that neighbouring row */
static void rptt3_vc_acoustics(int ixyz, int icoor, int meqn, int maux, int mbc, int mx, int nrow,
                               const double *aux1, const double *aux2, const double *aux3, int imp, int impt,
                               const double *bsasdq, double *cmbsasdq, double *cpbsasdq)
{
    int iuvw = ixyz + icoor - 1;
    if (iuvw > 3) iuvw = iuvw - 3;
    for (int i = 2 - mbc; i <= mx + mbc; i++) {
        const int i1 = i - 2 + imp;
        double zm, zz, zp, cm, cp;
        if (icoor == 2) {             /* new split in the y-like direction, inside the z-like row kk */
            const int kk = impt == 1 ? 1 : 3;
            zm = AX3(aux1, 1, i1, kk); zz = AX3(aux2, 1, i1, kk); zp = AX3(aux3, 1, i1, kk);
            cm = AX3(aux1, 2, i1, kk); cp = AX3(aux3, 2, i1, kk);
        } else {                      /* new split in the z-like direction, inside the y-like row aux1 / aux3 */
            const double *a = impt == 1 ? aux1 : aux3;
            zm = AX3(a, 1, i1, 1); zz = AX3(a, 1, i1, 2); zp = AX3(a, 1, i1, 3);
            cm = AX3(a, 2, i1, 1); cp = AX3(a, 2, i1, 3);
        }
        const double a1 = (-A2(bsasdq, 1, i) + A2(bsasdq, iuvw + 1, i) * zz) / (zm + zz);
        const double a2 = (A2(bsasdq, 1, i) + A2(bsasdq, iuvw + 1, i) * zz) / (zz + zp);
        for (int m = 1; m <= meqn; m++) { A2(cmbsasdq, m, i) = 0.0; A2(cpbsasdq, m, i) = 0.0; }
        A2(cmbsasdq, 1, i) = cm * a1 * zm;
        A2(cmbsasdq, iuvw + 1, i) = -cm * a1;
        A2(cpbsasdq, 1, i) = cp * a2 * zp;
        A2(cpbsasdq, iuvw + 1, i) = cp * a2;
    }
}

/* gadd(m, side 1:2, slice -1:1, i), hadd likewise (flux3.f:133-134) */
#define GA(arr, m, k, j, i) arr[((m)-1) + (size_t)meqn * (((k)-1) + 2 * (((j) + 1) + 3 * (size_t)IX(i)))]

/* flux3.f:168-593, unsplit (method(3) >= 0); the 24 transverse work arrays live in tw[] */
static int flux3_full(int rp, int ixyz, int meqn, int mwaves, int maux, int mbc, int mx, int nrow,
                      const int *method, const int *mthlim, work_t *w, double dtdy, double dtdz,
                      const double *aux1, const double *aux2, const double *aux3, double *gadd, double *hadd,
                      double **tw, double *cfl1d_out)
{
    double *wave = w->wave, *s = w->s, *amdq = w->amdq, *apdq = w->apdq, *cqxx = w->cqxx;
    double *q1d = w->q1d, *qadd = w->qadd, *fadd = w->fadd, *dtdx1d = w->dtdx1d;
    double *bmamdq = tw[0], *bmapdq = tw[1], *bpamdq = tw[2], *bpapdq = tw[3];
    double *cmamdq = tw[4], *cmapdq = tw[5], *cpamdq = tw[6], *cpapdq = tw[7];
    double *cmamdq2 = tw[8], *cmapdq2 = tw[9], *cpamdq2 = tw[10], *cpapdq2 = tw[11];
    double *bmcqxxp = tw[12], *bpcqxxp = tw[13], *bmcqxxm = tw[14], *bpcqxxm = tw[15];
    double *cmcqxxp = tw[16], *cpcqxxp = tw[17], *cmcqxxm = tw[18], *cpcqxxm = tw[19];
    double *bmcmamdq = tw[20], *bmcmapdq = tw[21], *bpcmamdq = tw[22], *bpcmapdq = tw[23];
    double *bmcpamdq = tw[24], *bmcpapdq = tw[25], *bpcpamdq = tw[26], *bpcpapdq = tw[27];
#define DT(i) dtdx1d[IX(i)]
    int limit = 0;
    for (int mw = 0; mw < mwaves; mw++)
        if (mthlim[mw] > 0) limit = 1;
    for (int i = 1 - mbc; i <= mx + mbc; i++)
        for (int m = 1; m <= meqn; m++) {
            A2(qadd, m, i) = 0.0;
            A2(fadd, m, i) = 0.0;
            for (int k = 1; k <= 2; k++)
                for (int j = -1; j <= 1; j++) { GA(gadd, m, k, j, i) = 0.0; GA(hadd, m, k, j, i) = 0.0; }
        }
    const int m3 = method[2] / 10, m4 = method[2] - 10 * m3;
    if (rp != RP_VC_ACOUSTICS_3D) return -1;
    const double *aux22 = aux2 + (size_t)maux * nrow;      /* aux2(:, :, 2): the slice's own aux */
    rpn3_vc_acoustics(ixyz, meqn, mwaves, maux, mbc, mx, q1d, q1d, aux22, aux22, wave, s, amdq, apdq);
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) A2(qadd, m, i) = A2(qadd, m, i) - DT(i) * A2(apdq, m, i);
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) A2(qadd, m, i - 1) = A2(qadd, m, i - 1) - DT(i - 1) * A2(amdq, m, i);
    double cfl1d = 0.0;
    for (int i = 1; i <= mx + 1; i++)
        for (int mw = 1; mw <= mwaves; mw++)
            cfl1d = dmax(dmax(cfl1d, DT(i) * S(mw, i)), -DT(i - 1) * S(mw, i));
    *cfl1d_out = cfl1d;
    if (method[1] != 1) {
        if (limit) limiter(meqn, mwaves, mbc, mx, wave, s, mthlim);
        for (int i = 2 - mbc; i <= mx + mbc; i++) {
            double dtdxave = 0.5 * (DT(i - 1) + DT(i));
            for (int m = 1; m <= meqn; m++) A2(cqxx, m, i) = 0.0;
            for (int mw = 1; mw <= mwaves; mw++)
                for (int m = 1; m <= meqn; m++)
                    A2(cqxx, m, i) = A2(cqxx, m, i) +
                                     0.5 * fabs(S(mw, i)) * (1.0 - fabs(S(mw, i)) * dtdxave) * W(m, mw, i);
            for (int m = 1; m <= meqn; m++) A2(fadd, m, i) = A2(fadd, m, i) + A2(cqxx, m, i);
        }
    }
    if (m3 <= 0) return 0;      /* flux3.f:260: no transverse propagation */

#define RPT3(icoor, imp, in, om, op) rpt3_vc_acoustics(ixyz, icoor, meqn, maux, mbc, mx, nrow, aux1, aux2, aux3, imp, in, om, op)
#define RPTT3(icoor, imp, impt, in, om, op) \
    rptt3_vc_acoustics(ixyz, icoor, meqn, maux, mbc, mx, nrow, aux1, aux2, aux3, imp, impt, in, om, op)
    RPT3(2, 1, amdq, bmamdq, bpamdq);
    RPT3(2, 2, apdq, bmapdq, bpapdq);
    RPT3(3, 1, amdq, cmamdq, cpamdq);
    RPT3(3, 2, apdq, cmapdq, cpapdq);
    if (m3 == 2) {              /* maux > 0: split cqxx with imp = 1 and imp = 2 (flux3.f:299-321) */
        RPT3(2, 1, cqxx, bmcqxxm, bpcqxxm);
        RPT3(2, 2, cqxx, bmcqxxp, bpcqxxp);
        RPT3(3, 1, cqxx, cmcqxxm, cpcqxxm);
        RPT3(3, 2, cqxx, cmcqxxp, cpcqxxp);
    }
    /* ---- G fluxes (y-like direction), flux3.f:347-452 */
    if (m4 == 1) {
        for (int i = 0; i <= mx + 2; i++)
            for (int m = 1; m <= meqn; m++) {
                A2(cpapdq2, m, i) = A2(cpapdq, m, i); A2(cpamdq2, m, i) = A2(cpamdq, m, i);
                A2(cmapdq2, m, i) = A2(cmapdq, m, i); A2(cmamdq2, m, i) = A2(cmamdq, m, i);
            }
    } else if (m4 == 2) {
        for (int i = 0; i <= mx + 2; i++)
            for (int m = 1; m <= meqn; m++) {
                A2(cpapdq2, m, i) = A2(cpapdq, m, i) - 3.0 * A2(cpcqxxp, m, i);
                A2(cpamdq2, m, i) = A2(cpamdq, m, i) + 3.0 * A2(cpcqxxm, m, i);
                A2(cmapdq2, m, i) = A2(cmapdq, m, i) - 3.0 * A2(cmcqxxp, m, i);
                A2(cmamdq2, m, i) = A2(cmamdq, m, i) + 3.0 * A2(cmcqxxm, m, i);
            }
    }
    if (m4 > 0) {
        RPTT3(2, 2, 2, cpapdq2, bmcpapdq, bpcpapdq);
        RPTT3(2, 1, 2, cpamdq2, bmcpamdq, bpcpamdq);
        RPTT3(2, 2, 1, cmapdq2, bmcmapdq, bpcmapdq);
        RPTT3(2, 1, 1, cmamdq2, bmcmamdq, bpcmamdq);
    }
    const double sixth = 1.0 / 6.0;
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) {
            GA(gadd, m, 1, 0, i - 1) = GA(gadd, m, 1, 0, i - 1) - 0.5 * DT(i - 1) * A2(bmamdq, m, i);
            GA(gadd, m, 2, 0, i - 1) = GA(gadd, m, 2, 0, i - 1) - 0.5 * DT(i - 1) * A2(bpamdq, m, i);
            GA(gadd, m, 1, 0, i) = GA(gadd, m, 1, 0, i) - 0.5 * DT(i) * A2(bmapdq, m, i);
            GA(gadd, m, 2, 0, i) = GA(gadd, m, 2, 0, i) - 0.5 * DT(i) * A2(bpapdq, m, i);
            if (m4 > 0) {
                GA(gadd, m, 2, 0, i) = GA(gadd, m, 2, 0, i) + sixth * DT(i) * dtdz * (A2(bpcpapdq, m, i) - A2(bpcmapdq, m, i));
                GA(gadd, m, 1, 0, i) = GA(gadd, m, 1, 0, i) + sixth * DT(i) * dtdz * (A2(bmcpapdq, m, i) - A2(bmcmapdq, m, i));
                GA(gadd, m, 2, 1, i) = GA(gadd, m, 2, 1, i) - sixth * DT(i) * dtdz * A2(bpcpapdq, m, i);
                GA(gadd, m, 1, 1, i) = GA(gadd, m, 1, 1, i) - sixth * DT(i) * dtdz * A2(bmcpapdq, m, i);
                GA(gadd, m, 2, -1, i) = GA(gadd, m, 2, -1, i) + sixth * DT(i) * dtdz * A2(bpcmapdq, m, i);
                GA(gadd, m, 1, -1, i) = GA(gadd, m, 1, -1, i) + sixth * DT(i) * dtdz * A2(bmcmapdq, m, i);
                GA(gadd, m, 2, 0, i - 1) = GA(gadd, m, 2, 0, i - 1) + sixth * DT(i - 1) * dtdz * (A2(bpcpamdq, m, i) - A2(bpcmamdq, m, i));
                GA(gadd, m, 1, 0, i - 1) = GA(gadd, m, 1, 0, i - 1) + sixth * DT(i - 1) * dtdz * (A2(bmcpamdq, m, i) - A2(bmcmamdq, m, i));
                GA(gadd, m, 2, 1, i - 1) = GA(gadd, m, 2, 1, i - 1) - sixth * DT(i - 1) * dtdz * A2(bpcpamdq, m, i);
                GA(gadd, m, 1, 1, i - 1) = GA(gadd, m, 1, 1, i - 1) - sixth * DT(i - 1) * dtdz * A2(bmcpamdq, m, i);
                GA(gadd, m, 2, -1, i - 1) = GA(gadd, m, 2, -1, i - 1) + sixth * DT(i - 1) * dtdz * A2(bpcmamdq, m, i);
                GA(gadd, m, 1, -1, i - 1) = GA(gadd, m, 1, -1, i - 1) + sixth * DT(i - 1) * dtdz * A2(bmcmamdq, m, i);
            }
            if (m3 < 2) continue;
            GA(gadd, m, 2, 0, i) = GA(gadd, m, 2, 0, i) + DT(i) * A2(bpcqxxp, m, i);
            GA(gadd, m, 1, 0, i) = GA(gadd, m, 1, 0, i) + DT(i) * A2(bmcqxxp, m, i);
            GA(gadd, m, 2, 0, i - 1) = GA(gadd, m, 2, 0, i - 1) - DT(i - 1) * A2(bpcqxxm, m, i);
            GA(gadd, m, 1, 0, i - 1) = GA(gadd, m, 1, 0, i - 1) - DT(i - 1) * A2(bmcqxxm, m, i);
        }
    /* ---- H fluxes (z-like direction), flux3.f:462-590 */
    if (m4 == 2)
        for (int i = 0; i <= mx + 2; i++)
            for (int m = 1; m <= meqn; m++) {
                A2(bpapdq, m, i) = A2(bpapdq, m, i) - 3.0 * A2(bpcqxxp, m, i);
                A2(bpamdq, m, i) = A2(bpamdq, m, i) + 3.0 * A2(bpcqxxm, m, i);
                A2(bmapdq, m, i) = A2(bmapdq, m, i) - 3.0 * A2(bmcqxxp, m, i);
                A2(bmamdq, m, i) = A2(bmamdq, m, i) + 3.0 * A2(bmcqxxm, m, i);
            }
    if (m4 > 0) {
        RPTT3(3, 2, 2, bpapdq, bmcpapdq, bpcpapdq);
        RPTT3(3, 1, 2, bpamdq, bmcpamdq, bpcpamdq);
        RPTT3(3, 2, 1, bmapdq, bmcmapdq, bpcmapdq);
        RPTT3(3, 1, 1, bmamdq, bmcmamdq, bpcmamdq);
    }
    for (int i = 1; i <= mx + 1; i++)
        for (int m = 1; m <= meqn; m++) {
            GA(hadd, m, 1, 0, i - 1) = GA(hadd, m, 1, 0, i - 1) - 0.5 * DT(i - 1) * A2(cmamdq, m, i);
            GA(hadd, m, 2, 0, i - 1) = GA(hadd, m, 2, 0, i - 1) - 0.5 * DT(i - 1) * A2(cpamdq, m, i);
            GA(hadd, m, 1, 0, i) = GA(hadd, m, 1, 0, i) - 0.5 * DT(i) * A2(cmapdq, m, i);
            GA(hadd, m, 2, 0, i) = GA(hadd, m, 2, 0, i) - 0.5 * DT(i) * A2(cpapdq, m, i);
            if (m4 > 0) {
                GA(hadd, m, 2, 0, i) = GA(hadd, m, 2, 0, i) + sixth * DT(i) * dtdy * (A2(bpcpapdq, m, i) - A2(bpcmapdq, m, i));
                GA(hadd, m, 1, 0, i) = GA(hadd, m, 1, 0, i) + sixth * DT(i) * dtdy * (A2(bmcpapdq, m, i) - A2(bmcmapdq, m, i));
                GA(hadd, m, 2, 1, i) = GA(hadd, m, 2, 1, i) - sixth * DT(i) * dtdy * A2(bpcpapdq, m, i);
                GA(hadd, m, 1, 1, i) = GA(hadd, m, 1, 1, i) - sixth * DT(i) * dtdy * A2(bmcpapdq, m, i);
                GA(hadd, m, 2, -1, i) = GA(hadd, m, 2, -1, i) + sixth * DT(i) * dtdy * A2(bpcmapdq, m, i);
                GA(hadd, m, 1, -1, i) = GA(hadd, m, 1, -1, i) + sixth * DT(i) * dtdy * A2(bmcmapdq, m, i);
                GA(hadd, m, 2, 0, i - 1) = GA(hadd, m, 2, 0, i - 1) + sixth * DT(i - 1) * dtdy * (A2(bpcpamdq, m, i) - A2(bpcmamdq, m, i));
                GA(hadd, m, 1, 0, i - 1) = GA(hadd, m, 1, 0, i - 1) + sixth * DT(i - 1) * dtdy * (A2(bmcpamdq, m, i) - A2(bmcmamdq, m, i));
                GA(hadd, m, 2, 1, i - 1) = GA(hadd, m, 2, 1, i - 1) - sixth * DT(i - 1) * dtdy * A2(bpcpamdq, m, i);
                GA(hadd, m, 1, 1, i - 1) = GA(hadd, m, 1, 1, i - 1) - sixth * DT(i - 1) * dtdy * A2(bmcpamdq, m, i);
                GA(hadd, m, 2, -1, i - 1) = GA(hadd, m, 2, -1, i - 1) + sixth * DT(i - 1) * dtdy * A2(bpcmamdq, m, i);
                GA(hadd, m, 1, -1, i - 1) = GA(hadd, m, 1, -1, i - 1) + sixth * DT(i - 1) * dtdy * A2(bmcmamdq, m, i);
            }
            if (m3 < 2) continue;
            GA(hadd, m, 2, 0, i) = GA(hadd, m, 2, 0, i) + DT(i) * A2(cpcqxxp, m, i);
            GA(hadd, m, 1, 0, i) = GA(hadd, m, 1, 0, i) + DT(i) * A2(cmcqxxp, m, i);
            GA(hadd, m, 2, 0, i - 1) = GA(hadd, m, 2, 0, i - 1) - DT(i - 1) * A2(cpcqxxm, m, i);
            GA(hadd, m, 1, 0, i - 1) = GA(hadd, m, 1, 0, i - 1) - DT(i - 1) * A2(cmcqxxm, m, i);
        }
    return 0;
#undef DT
#undef RPT3
#undef RPTT3
}

/* step3.f:96-592 (unsplit; no capacity function: the reference apps in 3-D have none and the product rejects it) */
int orc_step3(int rp, int maxm, int meqn, int mwaves, int maux, int mbc, int mx, int my, int mz,
              const double *qold, double *qnew, const double *aux, double dx, double dy, double dz, double dt,
              const int *method, const int *mthlim, double *cfl_out)
{
    if (method[5] != 0 || maux <= 0) return -3;
    work_t w;
    work_alloc(&w, maxm, mbc, meqn, mwaves);
    const int nrow = maxm + 2 * mbc;
    double *q1d = w.q1d, *qadd = w.qadd, *fadd = w.fadd, *dtdx1d = w.dtdx1d;
    double *aux1 = calloc((size_t)maux * nrow * 3, sizeof(double)), *aux2 = calloc((size_t)maux * nrow * 3, sizeof(double));
    double *aux3 = calloc((size_t)maux * nrow * 3, sizeof(double));
    double *gadd = calloc((size_t)meqn * 6 * nrow, sizeof(double)), *hadd = calloc((size_t)meqn * 6 * nrow, sizeof(double));
    double *tw[28];
    for (int k = 0; k < 28; k++) tw[k] = calloc((size_t)meqn * nrow, sizeof(double));
    double cfl = 0.0, cfl1d = 0.0;
    const double dtd[3] = {dt / dx, dt / dy, dt / dz};
    const int n[3] = {mx, my, mz};
    int rc = 0;
    for (int idir = 1; idir <= 3 && !rc; idir++) {
        const int d = idir - 1, e = (d + 1) % 3, f = (d + 2) % 3;      /* sweep, y-like, z-like directions */
        const int nd = n[d];
        /* loop nest of the Fortran: x: k outer, j inner; y: k outer, i inner; z: j outer, i inner */
        const int outer = idir == 3 ? 1 : 2, inner = idir == 1 ? 1 : 0;
        for (int i = 1 - mbc; i <= maxm + mbc; i++) dtdx1d[IX(i)] = dtd[d];
        for (int a = 0; a <= n[outer] + 1 && !rc; a++)
            for (int b = 0; b <= n[inner] + 1 && !rc; b++) {
                int c[3];
                c[outer] = a;
                c[inner] = b;
                for (int t = 1 - mbc; t <= nd + mbc; t++) {
                    c[d] = t;
                    for (int m = 1; m <= meqn; m++) A2(q1d, m, t) = Q4(qold, m, c[0], c[1], c[2]);
                    for (int oe = -1; oe <= 1; oe++)
                        for (int of = -1; of <= 1; of++) {
                            int cc[3] = {c[0], c[1], c[2]};
                            cc[e] += oe;
                            cc[f] += of;
                            double *dst = oe < 0 ? aux1 : (oe == 0 ? aux2 : aux3);
                            for (int ma = 1; ma <= maux; ma++)
                                dst[(ma - 1) + (size_t)maux * (IX(t) + (size_t)nrow * (of + 1))] = AUX4(ma, cc[0], cc[1], cc[2]);
                        }
                }
                rc = flux3_full(rp, idir, meqn, mwaves, maux, mbc, nd, nrow, method, mthlim, &w, dtd[e], dtd[f], aux1, aux2,
                                aux3, gadd, hadd, tw, &cfl1d);
                cfl = dmax(cfl, cfl1d);
                const double dty = dtd[e], dtz = dtd[f];
                for (int t = 1; t <= nd; t++)
                    for (int m = 1; m <= meqn; m++) {
                        c[d] = t;
#define QN(oe, of) (*qn_at(qnew, meqn, mbc, mx, my, c, e, f, oe, of, m))
#define G_(k, j) GA(gadd, m, k, j, t)
#define H_(k, j) GA(hadd, m, k, j, t)
                        double *p;
                        int cc[3];
#define AT(oe, of) (cc[0] = c[0], cc[1] = c[1], cc[2] = c[2], cc[e] += (oe), cc[f] += (of), p = &Q4(qnew, m, cc[0], cc[1], cc[2]))
                        AT(0, 0);   *p = *p + A2(qadd, m, t) - dtd[d] * (A2(fadd, m, t + 1) - A2(fadd, m, t)) -
                                         dty * (G_(2, 0) - G_(1, 0)) - dtz * (H_(2, 0) - H_(1, 0));
                        AT(-1, 0);  *p = *p - dty * G_(1, 0) - dtz * (H_(2, -1) - H_(1, -1));
                        AT(-1, -1); *p = *p - dty * G_(1, -1) - dtz * H_(1, -1);
                        AT(0, -1);  *p = *p - dty * (G_(2, -1) - G_(1, -1)) - dtz * H_(1, 0);
                        AT(1, -1);  *p = *p + dty * G_(2, -1) - dtz * H_(1, 1);
                        AT(1, 0);   *p = *p + dty * G_(2, 0) - dtz * (H_(2, 1) - H_(1, 1));
                        AT(1, 1);   *p = *p + dty * G_(2, 1) + dtz * H_(2, 1);
                        AT(0, 1);   *p = *p - dty * (G_(2, 1) - G_(1, 1)) + dtz * H_(2, 0);
                        AT(-1, 1);  *p = *p - dty * G_(1, 1) + dtz * H_(2, -1);
#undef AT
#undef G_
#undef H_
#undef QN
                    }
            }
    }
    *cfl_out = cfl;
    free(aux1); free(aux2); free(aux3); free(gadd); free(hadd);
    for (int k = 0; k < 28; k++) free(tw[k]);
    work_free(&w);
    return rc;
}

/* ======================================================================== the restated solvers, one by one
 * For oracle/ref_rp_shim.c: the reference's own step and flux Fortran calls rp1 / rpn2 / rpt2 / rpn3 / rpt3 / rptt3 by
 * name, and the shim answers with these.  The aux rows go in through orc_aux1d / orc_auxr1d / orc_auxb1d / orc_auxa1d
 * as for the oracle's own drivers (1-D, 2-D) or as arguments (3-D). */
int orc_rp1_any(int rp, const double *par, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                double *wave, double *s, double *amdq, double *apdq)
{
    if (rp == RP_ELASTICITY_FWAVE_1D) {
        if (!orc_aux1d || orc_maux1d < 3 || meqn != 2 || mwaves != 2) return -1;
        rp_fwave_normal(2, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq);
        return 0;
    }
    return orc_rp1_ptr(rp, par, meqn, mwaves, mbc, mx, ql, qr, wave, s, amdq, apdq);
}

int orc_rpt2_imp(int rp, const double *par, int ixy, int imp, int meqn, int mbc, int mx, const double *q1d,
                 const double *asdq, double *bmasdq, double *bpasdq)
{
    if (imp != 1 && imp != 2) return -1;
    return rpt2_dispatch(rp, ixy, meqn, mbc, mx, q1d, asdq, bmasdq, bpasdq, par, imp);
}

int orc_rpn3(int rp, int ixyz, int meqn, int mwaves, int maux, int mbc, int mx, const double *ql, const double *qr,
             const double *auxl, const double *auxr, double *wave, double *s, double *amdq, double *apdq)
{
    if (rp != RP_VC_ACOUSTICS_3D || maux < 2 || meqn != 4 || mwaves != 2) return -1;
    rpn3_vc_acoustics(ixyz, meqn, mwaves, maux, mbc, mx, ql, qr, auxl, auxr, wave, s, amdq, apdq);
    return 0;
}

/* aux1 / aux2 / aux3 are (maux, nrow, 3) */
int orc_rpt3(int rp, int ixyz, int icoor, int meqn, int maux, int mbc, int mx, int nrow, const double *aux1,
             const double *aux2, const double *aux3, int imp, const double *asdq, double *bmasdq, double *bpasdq)
{
    if (rp != RP_VC_ACOUSTICS_3D || maux < 2 || meqn != 4 || (icoor != 2 && icoor != 3) || (imp != 1 && imp != 2)) return -1;
    rpt3_vc_acoustics(ixyz, icoor, meqn, maux, mbc, mx, nrow, aux1, aux2, aux3, imp, asdq, bmasdq, bpasdq);
    return 0;
}

int orc_rptt3(int rp, int ixyz, int icoor, int meqn, int maux, int mbc, int mx, int nrow, const double *aux1,
              const double *aux2, const double *aux3, int imp, int impt, const double *bsasdq, double *cmbsasdq,
              double *cpbsasdq)
{
    if (rp != RP_VC_ACOUSTICS_3D || maux < 2 || meqn != 4 || (icoor != 2 && icoor != 3) || (imp != 1 && imp != 2) ||
        (impt != 1 && impt != 2))
        return -1;
    rptt3_vc_acoustics(ixyz, icoor, meqn, maux, mbc, mx, nrow, aux1, aux2, aux3, imp, impt, bsasdq, cmbsasdq, cpbsasdq);
    return 0;
}
