/*
 * oracle/ref_rp_shim.c  --  TEST INFRASTRUCTURE ONLY.
 *
 * The reference's classic step and flux routines (step1.f, step1fw.f, step2.f, step2ds.f, flux2.f, flux2fw.f, step3.f,
 * step3ds.f, flux3.f) call the Riemann solvers by name: rp1, rpn2, rpt2, rpn3, rpt3, rptt3.  Most of those solvers are
 * third-party and absent from the reference tree.  This file defines the six names, in the Fortran calling convention
 * (every argument by reference, trailing underscore), and forwards each call to THIS repository's restatement of the
 * solver in classic_oracle.c.  oracle/Makefile links it with the reference's Fortran, unchanged, into oracle/_ref/.
 *
 * What such a build pins is the step around the solver -- slicing, aux rows, Godunov update, CFL, limiter, second-order
 * and transverse corrections, flux differencing with and without capa -- in the reference's own code.  The solver
 * arithmetic is the oracle's on both sides and stays unpinned.
 *
 * Argument lists from the call sites: step1.f:80, step1fw.f:93, flux2.f:99,167 (flux2fw.f likewise), flux3.f:203,267,371.
 * rp1, rpn2 and rpt2 receive no maux: ref_shim_select() sets it, with the solver id and its parameters, before a step.
 */
#include <stddef.h>

extern const double *orc_aux1d, *orc_auxr1d, *orc_auxb1d, *orc_auxa1d;
extern int orc_maux1d;
int orc_rp1_any(int rp, const double *par, int meqn, int mwaves, int mbc, int mx, const double *ql, const double *qr,
                double *wave, double *s, double *amdq, double *apdq);
int orc_rpn2_ptr(int rp, const double *par, int ixy, int meqn, int mwaves, int mbc, int mx, const double *ql,
                 const double *qr, double *wave, double *s, double *amdq, double *apdq);
int orc_rpt2_imp(int rp, const double *par, int ixy, int imp, int meqn, int mbc, int mx, const double *q1d,
                 const double *asdq, double *bmasdq, double *bpasdq);
int orc_rpn3(int rp, int ixyz, int meqn, int mwaves, int maux, int mbc, int mx, const double *ql, const double *qr,
             const double *auxl, const double *auxr, double *wave, double *s, double *amdq, double *apdq);
int orc_rpt3(int rp, int ixyz, int icoor, int meqn, int maux, int mbc, int mx, int nrow, const double *aux1,
             const double *aux2, const double *aux3, int imp, const double *asdq, double *bmasdq, double *bpasdq);
int orc_rptt3(int rp, int ixyz, int icoor, int meqn, int maux, int mbc, int mx, int nrow, const double *aux1,
              const double *aux2, const double *aux3, int imp, int impt, const double *bsasdq, double *cmbsasdq,
              double *cpbsasdq);

static int sel_rp = -1, sel_maux = 0;
static double sel_par[8];
static int failures = 0;

/* the solver the next step runs with: id (oracle.py RP_*), its eight parameters, and the aux components per cell */
void ref_shim_select(int rp, const double *par, int maux)
{
    sel_rp = rp;
    sel_maux = maux;
    for (int k = 0; k < 8; k++) sel_par[k] = par ? par[k] : 0.0;
    failures = 0;
}

/* calls since ref_shim_select that no restated solver answered (the step then ran on whatever the work arrays held) */
int ref_shim_failures(void) { return failures; }

static void rows(const double *b, const double *m, const double *mr, const double *a)
{
    orc_auxb1d = b;
    orc_aux1d = m;
    orc_auxr1d = mr == m ? NULL : mr;
    orc_auxa1d = a;
    orc_maux1d = sel_maux;
}

void rp1_(const int *maxmx, const int *meqn, const int *mwaves, const int *mbc, const int *mx, const double *ql,
          const double *qr, const double *auxl, const double *auxr, double *wave, double *s, double *amdq, double *apdq)
{
    (void)maxmx;
    rows(NULL, auxl, auxr, NULL);
    if (orc_rp1_any(sel_rp, sel_par, *meqn, *mwaves, *mbc, *mx, ql, qr, wave, s, amdq, apdq)) failures++;
    rows(NULL, NULL, NULL, NULL);
}

void rpn2_(const int *ixy, const int *maxm, const int *meqn, const int *mwaves, const int *mbc, const int *mx,
           const double *ql, const double *qr, const double *auxl, const double *auxr, double *wave, double *s,
           double *amdq, double *apdq)
{
    (void)maxm;
    rows(NULL, auxl, auxr, NULL);
    if (orc_rpn2_ptr(sel_rp, sel_par, *ixy, *meqn, *mwaves, *mbc, *mx, ql, qr, wave, s, amdq, apdq)) failures++;
    rows(NULL, NULL, NULL, NULL);
}

void rpt2_(const int *ixy, const int *maxm, const int *meqn, const int *mwaves, const int *mbc, const int *mx,
           const double *ql, const double *qr, const double *aux1, const double *aux2, const double *aux3,
           const int *imp, const double *asdq, double *bmasdq, double *bpasdq)
{
    (void)maxm; (void)mwaves; (void)qr;
    rows(aux1, aux2, aux2, aux3);
    if (orc_rpt2_imp(sel_rp, sel_par, *ixy, *imp, *meqn, *mbc, *mx, ql, asdq, bmasdq, bpasdq)) failures++;
    rows(NULL, NULL, NULL, NULL);
}

void rpn3_(const int *ixyz, const int *maxm, const int *meqn, const int *mwaves, const int *mbc, const int *mx,
           const double *ql, const double *qr, const double *auxl, const double *auxr, const int *maux, double *wave,
           double *s, double *amdq, double *apdq)
{
    (void)maxm;
    if (orc_rpn3(sel_rp, *ixyz, *meqn, *mwaves, *maux, *mbc, *mx, ql, qr, auxl, auxr, wave, s, amdq, apdq)) failures++;
}

/* aux1 / aux2 / aux3 are (maux, 1-mbc:maxm+mbc, 3): rows of maxm + 2*mbc cells */
void rpt3_(const int *ixyz, const int *icoor, const int *maxm, const int *meqn, const int *mwaves, const int *mbc,
           const int *mx, const double *ql, const double *qr, const double *aux1, const double *aux2, const double *aux3,
           const int *maux, const int *imp, const double *asdq, double *bmasdq, double *bpasdq)
{
    (void)mwaves; (void)ql; (void)qr;
    if (orc_rpt3(sel_rp, *ixyz, *icoor, *meqn, *maux, *mbc, *mx, *maxm + 2 * *mbc, aux1, aux2, aux3, *imp, asdq, bmasdq,
                 bpasdq))
        failures++;
}

void rptt3_(const int *ixyz, const int *icoor, const int *maxm, const int *meqn, const int *mwaves, const int *mbc,
            const int *mx, const double *ql, const double *qr, const double *aux1, const double *aux2, const double *aux3,
            const int *maux, const int *imp, const int *impt, const double *bsasdq, double *cmbsasdq, double *cpbsasdq)
{
    (void)mwaves; (void)ql; (void)qr;
    if (orc_rptt3(sel_rp, *ixyz, *icoor, *meqn, *maux, *mbc, *mx, *maxm + 2 * *mbc, aux1, aux2, aux3, *imp, *impt, bsasdq,
                  cmbsasdq, cpbsasdq))
        failures++;
}
