/*
 * pyclaw_amd.h -- C ABI of libpyclaw_amd.so (MI355X / gfx950 HIP implementation of
 * PyClaw's classic + SharpClaw hot path).
 *
 * What this boundary replaces in the reference (paths relative to the reference tree):
 * the f2py extension modules classic1/classic2/(classic3)/sharpclaw1/sharpclaw2 that
 * src/pyclaw/clawpack.py:323,538-552 and src/pyclaw/sharpclaw.py:385,558 import and
 * call, plus the ghost-cell/backup array traffic those Python drivers do around them
 * (src/pyclaw/solver.py:315-452, :660, :690; src/petclaw/state.py:236-269 for the
 * halo exchange and src/petclaw/cfl.py:29-31 for the CFL all-reduce).
 *
 * Two layers:
 *   1. "f2py-shaped" stateless calls on HOST arrays (pcl_step1 / pcl_step2ds /
 *      pcl_step2): same argument meaning as the Fortran subroutines, Fortran array
 *      order, caller owns every array.  A maintainer can bind these in place of the
 *      f2py modules without touching the Python drivers (PCIe traffic every call).
 *   2. A resident solver handle (pcl_create ...): q/aux live in HBM across steps,
 *      ghost cells, backup/restore, CFL reduction and halo exchange run on the device.
 *      This is what the pyclaw_amd ClawSolver / SharpClawSolver classes use.
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * PCL_E* code and leaves a message for pcl_last_error(); host arrays are Fortran
 * ordered float64 with the component index fastest, q(m,i,j) at
 * q[(m) + meqn*((i) + (mx+2*mbc)*(j))] (0-based, ghost cells included) exactly like the
 * reference's qbc (doc/differences.rst:9-17).  One host thread per solver handle.
 * There is NO CPU fallback: every entry point fails with PCL_ENODEVICE without a GPU.
 */
#ifndef PYCLAW_AMD_H
#define PYCLAW_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define PCL_MAX_WAVES 8
#define PCL_MAX_RP_PARAMS 8

/* error codes */
#define PCL_OK 0
#define PCL_EINVAL (-1)    /* bad argument / unsupported configuration           */
#define PCL_ENODEVICE (-2) /* no usable HIP device                               */
#define PCL_EHIP (-3)      /* a HIP runtime call failed                          */
#define PCL_ECOMM (-4)     /* RCCL failure                                       */
#define PCL_ESTATE (-5)    /* call not valid in the handle's current state       */

/* Riemann solver ids.  The reference selects the solver at link time (the rpn2/rpt2
 * symbols of the app Makefile, e.g. apps/euler/2d/shockbubble/Makefile:3) and passes
 * its scalars through `common /cparam/` (src/pyclaw/state.py:142-162); here it is an
 * id plus the cparam values in declaration order. */
#define PCL_RP_ADVECTION_1D 1 /* rp1_advection.f            cparam: u                   */
#define PCL_RP_ACOUSTICS_1D 2 /* rp1_acoustics.f            cparam: rho,bulk,cc,zz      */
#define PCL_RP_BURGERS_1D 3     /* rp1_burgers.f90 (transonic entropy fix); no cparam            */
#define PCL_RP_EULER_1D 4       /* rp1_euler_with_efix.f          cparam: gamma,gamma1            */
#define PCL_RP_SHALLOW_1D 5     /* rp1_shallow_roe_with_efix.f    cparam: g                       */
#define PCL_RP_ADVECTION_COLOR_1D 6 /* rp1_advection_color.f; aux(1) = velocity at the cell's left edge */
#define PCL_RP_ELASTICITY_FWAVE_1D 7 /* rp1_nonlinear_elasticity_fwave.f (stegoton); F-WAVE solver: fwave = 1;  */
                                     /* aux(1)=rho, aux(2)=K, aux(3)=1: sigma=K eps, else exp(K eps)-1;         */
                                     /* classic solver only (PCL_KIND_SHARPCLAW is refused)                     */
#define PCL_RP_ACOUSTICS_2D 10 /* rpn2/rpt2_acoustics.f     cparam: rho,bulk,cc,zz      */
#define PCL_RP_EULER5_2D 11    /* rpn2/rpt2_euler_5wave.f   cparam: gamma,gamma1        */
#define PCL_RP_ADVECTION_2D 12  /* rpn2/rpt2_advection.f      cparam: u,v                  */
#define PCL_RP_SHALLOW_2D 13    /* rpn2/rpt2_shallow_roe_with_efix.f  cparam: g            */
#define PCL_RP_VC_ACOUSTICS_2D 14 /* rpn2/rpt2_vc_acoustics.f; aux(1)=Z, aux(2)=c */
#define PCL_RP_VC_ADVECTION_2D 15 /* rpn2/rpt2_vc_advection.f; aux(1)=u at the left edge, aux(2)=v at the bottom edge */
#define PCL_RP_SHALLOW_SPHERE_2D 16 /* rpn2/rpt2_shallow_sphere.f (apps/shallow-sphere/Makefile:7); common /sw/ g + comxyt dxcom,dycom */
                                    /* -> rp_params g, dx, dy; aux = the 16 components of apps/shallow-sphere/setaux.f:10-25;      */
                                    /* the unsplit step follows the app's step2qcor.f (conservation fix qcor.f) instead of step2.f */
#define PCL_RP_PSYSTEM_FWAVE_2D 17 /* rpn2/rpt2_psystem.f (test/psystem/Makefile:5); F-WAVE solver: fwave = 1; aux as above + aux(4)=eps */
                                   /* (read by rpt2 only); classic and SharpClaw (weno_order 5: mbc 3), fwave = 1 for both      */
#define PCL_RP_VC_ACOUSTICS_3D 20 /* rpn3_vc_acoustics.f (test/acoustics/3d/Makefile); aux(1)=Z, aux(2)=c; dim-split, and unsplit  */
                                  /* (rpt3/rptt3_vc_acoustics.f) without a capacity function                                   */
#define PCL_RP_CELL 100 /* a user-written normal Riemann solver compiled at run time (pcl_cellrp_compile / _attach below):  */
                        /* meqn, mwaves <= 8 from the config, rp_params = the body's p[8]; classic 1-D and dimension-split  */
                        /* 2-D steps (unsplit with a transverse body); the body may read listed aux components              */
                        /* (pcl_cellrp_compile_aux); f-waves and a capacity function through pcl_cellrp_compile_form and    */
                        /* pcl_create_cellrp; the SharpClaw stages through pcl_cellrp_compile_sharp and pcl_create_cellrp;  */
                        /* the dimension-split 3-D step through pcl_cellrp_compile3 and pcl_create_cellrp.                  */
                        /* The dimension-split 2-D step runs as two passes unless the handle also carries the one-kernel    */
                        /* step (pcl_cellrp_compile_onek): then in either form, chosen as for a built-in solver.            */
                        /* Not a built-in solver: pcl_rp_info refuses the id                                                */

/* boundary condition types = pyclaw.BC (src/pyclaw/solver.py:17-23) */
#define PCL_BC_CUSTOM 0
#define PCL_BC_OUTFLOW 1
#define PCL_BC_PERIODIC 2
#define PCL_BC_REFLECTING 3
/* not a pyclaw.BC value: the sphere app's custom y boundary (qbc_lower_y / qbc_upper_y,
 * apps/shallow-sphere/shallow_4_Rossby_Haurwitz_wave.py:295-313): ghost row j mirrors interior row 2*mbc-1-j with the
 * x index reversed over the whole ghosted width.  Accepted by pcl_bc for idim = 1. */
#define PCL_BC_SPHERE_MIRROR 4

/* arithmetic mode */
#define PCL_MATH_EXACT 0 /* no FMA contraction, IEEE divide/sqrt: bit-identical to the  */
                         /* reference Fortran built without FMA (the parity mode)        */
#define PCL_MATH_FAST 1  /* FMA contraction + reciprocal-multiply division (each quotient  */
                         /* within ~1 ulp instead of correctly rounded).  Not bit-identical;*/
                         /* tested against the reference goldens at rtol 1e-12.            */
#define PCL_MATH_STRICT 2 /* PCL_MATH_EXACT whose quotients take the IEEE division also when the    */
                          /* numerator lies in the underflow range (|n| < 2^-960: a momentum of      */
                          /* 1e-310 ahead of a front), where EXACT's shared-reciprocal quotient can  */
                          /* be one step of the denormal grid off (measured <= 3.2e-322).  3-5 %     */
                          /* slower than EXACT on compute-bound states, equal on the headline.       */

/* solver kind: classic wave propagation (clawpack.py) or SharpClaw method of lines (sharpclaw.py) */
#define PCL_KIND_CLASSIC 0
#define PCL_KIND_SHARPCLAW 1

/* SharpClaw registers: state q, the two Runge-Kutta stage registers (Solver._rk_stages,
 * solver.py:266-291), the increment dq, and one scratch register (dq_src contributions) */
#define PCL_REG_Q 0
#define PCL_REG_S1 1
#define PCL_REG_S2 2
#define PCL_REG_DQ 3
#define PCL_REG_TMP 4
/* Stage derivatives K_0 .. K_{s-1} of a Runge-Kutta scheme given by its Butcher tableau (pcl_rk_stages): s <= 16.  They are
 * named by their index; PCL_REG_K0 + j is K_j where a register id is asked for (only to be refused: pcl_rk_lincomb). */
#define PCL_RK_MAX_STAGES 16
#define PCL_REG_K0 16

typedef struct pcl_solver pcl_solver;

typedef struct pcl_config {
    int ndim;                       /* 1 or 2                                              */
    int n[3];                       /* interior cells of THIS process' block: mx,my,(mz)   */
    int mbc;                        /* ghost width (classic: 2)                            */
    int meqn, mwaves, maux;
    int method[7];                  /* as ClawSolver.set_method (clawpack.py:192-212):     */
                                    /* [1]=order, [2]=-1 dim-split | order_trans,          */
                                    /* [5]=mcapa+1 (0 = no capa), [6]=maux                 */
    int mthlim[PCL_MAX_WAVES];      /* limiter per wave family (philim.f ids 0..5)         */
    int fwave;                      /* 1: f-wave form (flux2fw.f:151-152)                  */
    int rp;                         /* PCL_RP_*                                            */
    double rp_params[PCL_MAX_RP_PARAMS];
    double d[3];                    /* dx,dy,(dz)                                          */
    int device;                     /* HIP device ordinal                                  */
    int math;                       /* PCL_MATH_*                                          */
    int kind;                       /* PCL_KIND_CLASSIC | PCL_KIND_SHARPCLAW               */
    int lim_type;                   /* SharpClaw: 1 = tvd2 (reconstruct.f90:568-625; mthlim per COMPONENT),     */
                                    /*            2 = PyWENO form (weno.f90), order 2*mbc-1: mbc = 3..9 is      */
                                    /*                weno_order 5..17 (sharpclaw.py:479), 3 = legacy WENO5     */
} pcl_config;

/* ---- library ---------------------------------------------------------------------- */
const char *pcl_last_error(void);
int pcl_version(void);
int pcl_device_count(void);                     /* never initialises a context          */
/* What the library knows about the built-in Riemann solver `rp`, read off the solver itself; touches no GPU.
 * info = ndim, meqn, mwaves, naux (aux components the normal solver reads), fwave (an f-wave solver: cfg.fwave must be
 * 1), onek / onek_aux (the one-kernel dimension-split 2-D step has it, without / with its aux arrays staged), sharp
 * (SharpClaw kernels, weno_order 5), sharp_high (weno_order 7..17 too), sharp_wave (char_decomp = 1).
 * PCL_EINVAL for an id no solver has. */
int pcl_rp_info(int rp, int info[10]);

/* ---- layer 1: f2py-shaped stateless calls on host arrays ---------------------------- */
/* Stateless for the caller like the f2py modules; internally the device buffers of the last call are kept and reused
 * while the array shapes stay the same.  pcl_layer1_release() frees them (optional: also done at unload). */
void pcl_layer1_release(void);
/* Arithmetic mode of the layer-1 calls that follow (default PCL_MATH_EXACT, the f2py modules' results bit for bit). */
int pcl_layer1_math(int math);
/* classic1.step1(mbc,mx,q,aux,dx,dt,method,mthlim) -> (q,cfl)   step1.f:4-5, clawpack.py:323.
 * q(meqn,1-mbc:mx+mbc) is updated in place for cells 1..mx (the two ghost cells the
 * Fortran also touches are left unchanged: no caller reads them, clawpack.py:406). */
int pcl_step1(int rp, const double *rp_params, int meqn, int mwaves, int maux, int mbc, int mx,
              double *q, const double *aux, double dx, double dt, const int *method,
              const int *mthlim, double *cfl);

/* classic1fw.step1(...) -> (q,cfl): the f-wave twin, src/fortran/1d/classic/step1fw.f (clawpack.py:221-222 picks the
 * module name + 'fw' when solver.fwave is set); rp must be an f-wave solver. */
int pcl_step1fw(int rp, const double *rp_params, int meqn, int mwaves, int maux, int mbc, int mx,
                double *q, const double *aux, double dx, double dt, const int *method,
                const int *mthlim, double *cfl);

/* classic2.step2ds(maxm,mbc,mx,my,qold,qnew,aux,dx,dy,dt,method,mthlim,aux1,aux2,aux3,work,ids)
 * -> (qnew,cfl)   step2ds.f:2-5, clawpack.py:538-544.  qold may alias qnew.  The work
 * arrays of the Fortran signature have no meaning here and are not taken. */
int pcl_step2ds(int rp, const double *rp_params, int fwave, int meqn, int mwaves, int maux,
                int mbc, int mx, int my, const double *qold, double *qnew, const double *aux,
                double dx, double dy, double dt, const int *method, const int *mthlim,
                double *cfl, int ids);

/* classic2.step2(...) -> (qnew,cfl)   step2.f:2-5, clawpack.py:550-552 (unsplit). */
int pcl_step2(int rp, const double *rp_params, int fwave, int meqn, int mwaves, int maux,
              int mbc, int mx, int my, const double *qold, double *qnew, const double *aux,
              double dx, double dy, double dt, const int *method, const int *mthlim,
              double *cfl);

/* classic3.step3ds(maxm,mbc,mx,my,mz,qold,qnew,aux,dx,dy,dz,dt,method,mthlim,aux1,aux2,aux3,work,idir)
 * -> (qnew,cfl)   src/fortran/3d/classic/step3ds.f:2-5, clawpack.py:678-688: one directional sweep
 * (idir 1..3) of the dimension-split 3-D algorithm; q(m,i,j,k) component fastest, ghost cells included;
 * slices with transverse indices 0..m+1 are swept, everything else is returned unchanged. */
int pcl_step3ds(int rp, const double *rp_params, int meqn, int mwaves, int maux, int mbc, int mx, int my,
                int mz, const double *qold, double *qnew, const double *aux, double dx, double dy, double dz,
                double dt, const int *method, const int *mthlim, double *cfl, int idir);

/* classic3.step3(maxm,mbc,mx,my,mz,qold,qnew,aux,dx,dy,dz,dt,method,mthlim,aux1,aux2,aux3,work) -> (qnew,cfl)
 * src/fortran/3d/classic/step3.f:2-6, clawpack.py:690-696: the UNSPLIT 3-D step with the transverse solves rpt3 / rptt3
 * (flux3.f:260-593); method[2] = order_trans = 0, 10, 11, 20, 21 or 22.  Interior cells of qnew are updated, ghost
 * cells returned unchanged. */
int pcl_step3(int rp, const double *rp_params, int meqn, int mwaves, int maux, int mbc, int mx, int my, int mz,
              const double *qold, double *qnew, const double *aux, double dx, double dy, double dz, double dt,
              const int *method, const int *mthlim, double *cfl);

/* sharpclaw1.flux1(q,aux,dt,t,ixy,mx,mbc,maxnx) -> (dq,cfl)   1d/sharpclaw/flux1.f90, sharpclaw.py:385
 * sharpclaw2.flux2(q,aux,dt,t,mbc,maxm,mx,my)   -> (dq,cfl)   2d/sharpclaw/flux2.f90:2, sharpclaw.py:558
 * q and dq are (meqn, mx+2mbc[, my+2mbc]) with mbc = (weno_order+1)/2 = 3..9 (clawparams.weno_order is
 * implied by mbc: lim_type 2 with mbc = k runs weno(2k-1); lim_type 1 and 3 take mbc = 3); dq's interior receives
 * dt*dq/dt, its ghost cells are zeroed.  The F90 module state the reference sets through
 * clawparams/workspace/reconstruct (lim_type, mcapa, dx, mwaves) is passed explicitly; clawparams.fwave follows the
 * Riemann solver (set for PCL_RP_PSYSTEM_FWAVE_2D, the one f-wave solver these calls take), as sharpclaw.py:269 sets
 * it from the solver object. */
/* clawparams.mthlim, part of the F90 module state the reference sets before calling flux1/flux2
 * (sharpclaw.py:268); read by lim_type = 1 (tvd2) only, indexed by component.  Default: all 1 (minmod). */
int pcl_sharp_module_mthlim(const int *mthlim, int n);
/* clawparams.char_decomp of the same module state (sharpclaw.py:262), read by pcl_sharp_flux1: 0 = component-wise
 * reconstruction, 1 = wave-based (1d/sharpclaw/flux1.f90:80-107: rp1 on the cell averages, then tvd2_wave for
 * lim_type 1 -- mthlim indexed by WAVE there -- or weno5_wave for lim_type 2; reconstruct.f90:393-478,728-806), for
 * the six 1-D solvers PCL_RP_ADVECTION_1D .. PCL_RP_ADVECTION_COLOR_1D, with aux arrays and a capacity function
 * (mcapa) where the solver or the caller has them; mbc 3, no f-wave solver.
 * 2 and 3 need a user-supplied evec routine the reference only stubs (evec.f90:13-14), and the 2-D flux1.f90 calls
 * rpn2 with a wrong argument list on the char_decomp = 1 path (2d/sharpclaw/flux1.f90:86): neither can run in the
 * reference, neither is offered.  A resident solver takes the value in cfg.method[4] (method(5), unused by SharpClaw). */
int pcl_sharp_module_char_decomp(int char_decomp);
int pcl_sharp_flux1(int rp, const double *rp_params, int lim_type, int meqn, int mwaves, int maux, int mcapa,
                    int mbc, int mx, const double *q, double *dq, const double *aux, double dx, double dt,
                    double *cfl);
int pcl_sharp_flux2(int rp, const double *rp_params, int lim_type, int meqn, int mwaves, int maux, int mcapa,
                    int mbc, int mx, int my, const double *q, double *dq, const double *aux, double dx,
                    double dy, double dt, double *cfl);

/* ---- layer 2: resident solver -------------------------------------------------------- */
int pcl_create(const pcl_config *cfg, pcl_solver **out);
void pcl_destroy(pcl_solver *s);

/* Host <-> device copies of the whole block.  with_ghosts=0: host array is state.q,
 * (meqn,mx[,my]) Fortran order (get_qbc_from_q / set_q_from_qbc, state.py:171-206);
 * with_ghosts=1: host array is qbc, (meqn,mx+2mbc[,my+2mbc]). */
int pcl_put_q(pcl_solver *s, const double *host, int with_ghosts);
int pcl_get_q(pcl_solver *s, double *host, int with_ghosts);
int pcl_put_aux(pcl_solver *s, const double *host_auxbc); /* always with ghosts (auxbc)   */
int pcl_get_aux(pcl_solver *s, double *host_auxbc);       /* its twin: the resident aux, ghosts included (a start_step
                                                           * cell function may have written it, see below)        */

/* Ghost fill of one side of one dimension on the device: solver.py:384-452.
 * side 0 = lower, 1 = upper.  PCL_BC_CUSTOM is not accepted here: use the strip calls
 * (arbitrary user numpy code) or pcl_bc_const (inflow of a constant state). */
int pcl_bc(pcl_solver *s, int idim, int side, int bctype);
int pcl_bc_const(pcl_solver *s, int idim, int side, const double *state /* [meqn] */);
/* Same fill for the aux array (auxbc_lower/upper, solver.py:526-596: reflecting does not negate). */
int pcl_bc_aux(pcl_solver *s, int idim, int side, int bctype);
/* Copy the `width` outermost layers (ghost cells first) of one side to/from a host
 * array shaped like qbc with that dimension cut to `width`: for custom BCs written in
 * Python that only touch the strip (user_bc_lower/upper, solver.py:404-405,439-440).  1-D, 2-D and 3-D. */
int pcl_get_strip(pcl_solver *s, int idim, int side, int width, double *host);
int pcl_put_strip(pcl_solver *s, int idim, int side, int width, const double *host);
/* the aux twin of pcl_put_strip: a ghost strip of auxbc filled by a Python aux-BC callback (user_aux_bc_lower/upper,
 * solver.py:526-596), placed after the aux halo exchange of a decomposed run */
int pcl_put_aux_strip(pcl_solver *s, int idim, int side, int width, const double *host);
/* Gauges (Solver.write_gauge_values, solver.py:731-741: q[:,x,y] and aux[:,x,y] of a few cells
 * after every step): gather `ncell` interior cells (0-based interior indices ij[2*c], ij[2*c+1];
 * the second is ignored in 1-D; on a 3-D grid the tuples are triples ij[3*c], ij[3*c+1], ij[3*c+2]) of the resident q -- and of aux when `aux` is not NULL -- into
 * q[ncell][meqn] / aux[ncell][maux].  One small kernel + one D2H of ncell*(meqn+maux) doubles
 * instead of reading the whole state back every step.  Read-only for the bits, not for the time: the call ends with a
 * synchronisation of the solver's stream, so behind a pcl_bc_step that has enqueued the next step ahead (pcl_step_ahead)
 * it waits for that whole step as well.  A caller that wants the gauge cells of EVERY step uses the gauge log below. */
int pcl_get_cells(pcl_solver *s, int ncell, const int *ij, double *q, double *aux);
/* Device gauge log: the same cells recorded by every step itself, read whenever the caller likes.  While the log is armed,
 * pcl_bc_step and pcl_step_hyperbolic enqueue one more small kernel behind the step (every plan and form of it; behind an
 * adopted step of pcl_step_ahead too, in front of the step they enqueue ahead) that copies the gauge cells of the NEW
 * state into the next record of a device-resident log -- on the solver's stream, no synchronisation, no host copy.  There
 * is no per-step call by design: it would have to make the next one-kernel step compute every tile and drop a step
 * enqueued ahead, every step.
 * pcl_gauge_log arms: ij as for pcl_get_cells (checked the same way: PCL_EINVAL for a cell outside the interior), uploaded
 * once; capacity >= 1 records of ncell * per doubles, per = meqn + maux (maux counts when the handle has an aux array; per
 * is fixed while the log is armed, and a step that finds it changed fails with PCL_ESTATE).  Arming again replaces the log
 * and its counters; ncell = 0 disarms and frees, as pcl_destroy does.  Classic solvers only: PCL_ESTATE on a SharpClaw
 * handle (its stages are not steps).
 * A step with the log full (capacity records held) fails with PCL_ESTATE before it launches anything: the log never
 * writes past its end.  pcl_undo_step and pcl_restore take the record of the last step back with the step, once: a
 * rejected step leaves no record, and the retake writes the same slot.
 * pcl_gauge_log_read: ONE device-to-host copy of the *nrecords records held and one synchronisation; out[r][c][m], record
 * major (oldest first), then cell, then the meqn components of q, then the aux components.  The log is empty afterwards.
 * PCL_EINVAL, and nothing read, when max_records is smaller than the records held.
 * pcl_gauge_log_stats: records written, records taken back and reads since the log was armed.
 * None of the three is a read-only call: a step enqueued ahead is dropped by the next pcl_bc_step. */
int pcl_gauge_log(pcl_solver *s, int ncell, const int *ij, int capacity);
int pcl_gauge_log_read(pcl_solver *s, int max_records, double *out, int *nrecords);
int pcl_gauge_log_stats(pcl_solver *s, long *recorded, long *popped, long *reads);

/* One homogeneous step of length dt on the resident state (ghost cells must be filled):
 * dim-split  = step2ds(ids=1) then step2ds(ids=2)          clawpack.py:538-546
 * unsplit    = step2                                       clawpack.py:550-552
 * 1-D        = step1                                       clawpack.py:323
 * *cfl receives the max Courant number -- over all blocks once pcl_comm_init has been called (the
 * all-reduce of petclaw/cfl.py:29-31 runs on the device before the read-back).  The pre-step state
 * stays available until the next call: pcl_undo_step() makes it current again (the
 * reference's q_backup / retake path, solver.py:660,690) without any copy. */
int pcl_step_hyperbolic(pcl_solver *s, double dt, double *cfl);
int pcl_undo_step(pcl_solver *s);
/* apply_q_bcs + step_hyperbolic in ONE call (clawpack.py:528-555 with solver.py:354-381): the ghost
 * fills of the listed sides, in the reference's order (dimension by dimension, lower then upper),
 * then the step.  bc[2*idim+side] = PCL_BC_OUTFLOW/PERIODIC/REFLECTING, PCL_BC_CUSTOM with
 * cstate[(2*idim+side)*PCL_MAX_RP_PARAMS ...] = constant state, or -1 = leave that side alone (not at a
 * physical boundary / periodic handled by the halo).  Does the halo exchange first when pcl_comm_init
 * has been called. */
int pcl_bc_step(pcl_solver *s, const int *bc, const double *cstate, double dt, double *cfl);
/* Single directional sweep (ids = 1 or 2), qold -> qnew like step2ds; used by layer 1. */
int pcl_sweep(pcl_solver *s, int ids, double dt, double *cfl);

/* Explicit device-side backup/restore (needed when user code modifies q before the
 * hyperbolic step: Strang source splitting, start_step). */
int pcl_backup(pcl_solver *s);
int pcl_restore(pcl_solver *s);

/* Built-in device source terms for the reference apps' step_src callbacks.
 * id 1: Euler radial-symmetry source, 2-stage RK (test/euler/2d/shockbubble.py:59-94);
 *       aux[0] = radial coordinate; params = {gamma1, ndim}. */
#define PCL_SRC_EULER_RADIAL 1
/* id 2: Coriolis force of the shallow-water-on-the-sphere app, apps/shallow-sphere/src2.f:43-146 (projection onto the
 *       tangent plane, 4-stage RK, projection); aux components 14-16 = radial unit vector; no params. */
#define PCL_SRC_SPHERE_CORIOLIS 2
int pcl_src(pcl_solver *s, int src_id, double dt, const double *params, int nparams);
/* Godunov-split source term (clawpack.py:156-159: step_src(dt) after an accepted hyperbolic step) applied by the LAST
 * pass of the 2-D step (y pass of step2ds, y phase of step2) while it stores its results, instead of one more read + write of q by
 * pcl_src: same arithmetic, same bits.  src_id = PCL_SRC_EULER_RADIAL with params {gamma1, ndim}, or 0 to switch it
 * off.  A rejected step discards the pass' output with the rest (pcl_undo_step), as step() returns before the source. */
int pcl_fuse_source(pcl_solver *s, int src_id, const double *params, int nparams);

/* ---- cell functions: user-written per-cell arithmetic on the resident arrays ----------------------------------
 * The reference's step_src / dq_src / start_step callbacks are arbitrary numpy code on host arrays.  A cell function is
 * the same arithmetic for ONE cell, given as the text of a C++ function body; the library compiles it at run time
 * (libhiprtc, opened on first use; the architecture this library was built for, no device needed) into a wrapper kernel
 * that runs it over the interior cells of the resident arrays: one read and one write of the components it assigns,
 * ghost cells never touched.  The body sees
 *     q[MEQN]      the cell's state (const for a dq_src)          aux[MAUX]   const unless compiled with writes_aux
 *     dq[MEQN]     dq_src only: zero on entry, afterwards deltaq = deltaq + dq[m] (sharpclaw.py:232-235)
 *     c.t, c.dt    time and step length                            p[16]       the parameters of this launch
 *     c.i[NDIM]    GLOBAL 0-based interior indices                 c.d[NDIM]   cell sizes
 *     c.x[NDIM]    cell centre, lower + (i + 0.5) * d with the global i (grid.py)
 * and whatever `preamble` (helper functions, file scope) declares.  Diagnostics carry the body's own line numbers behind
 * the kind's name ("step_src:2:...").  math: PCL_MATH_EXACT / _STRICT compile without FMA contraction and with IEEE
 * division and square root, like the library's own source kernels; PCL_MATH_FAST allows contraction. */
#define PCL_CELLFN_STEP_SRC 1
#define PCL_CELLFN_DQ_SRC 2
#define PCL_CELLFN_START_STEP 3
#define PCL_CELLFN_BC 4         /* a boundary condition: its own body surface and launch, pcl_cellbc_apply below */
#define PCL_CELLFN_MAX_PARAMS 16
#define PCL_CELLFN_MAX_REACH 8  /* the largest mbc the library takes */
typedef struct pcl_cellfn pcl_cellfn;
/* Compile (host only, no device needed).  Functions are cached per process by (kind, body, preamble, meqn, maux, ndim,
 * math, writes_aux): compiling the same text again returns the cached handle with one more reference.  *code_size (may
 * be NULL) = bytes of the code object.  A compile error is PCL_EINVAL with the compiler's log in pcl_last_error().
 * writes_aux: aux[] is writable in the body (PCL_CELLFN_START_STEP only, maux > 0). */
int pcl_cellfn_compile(int kind, const char *body, const char *preamble, int meqn, int maux, int ndim, int math,
                       int writes_aux, pcl_cellfn **out, long *code_size);
/* The same with neighbour reads (kinds _STEP_SRC, _DQ_SRC, _START_STEP; writes_aux = 0).  reach, 0..PCL_CELLFN_MAX_REACH,
 * is the largest index offset in any dimension at which the body reads other cells, and part of the cache key;
 * reach = 0 IS pcl_cellfn_compile (same options, key and handle).  With reach > 0 the body also sees
 *     qn(m, di[, dj[, dk]])     component m of the cell at that index offset from the lane's own, AS IT WAS WHEN THE
 *                               LAUNCH BEGAN (qn(m, 0) is the cell's own old value); ghost cells up to reach layers
 *     auxn(m, di[, dj[, dk]])   the same for aux (maux > 0)
 * Offsets are clamped to [-reach, reach] and m to the components there are, so whatever the body passes no read leaves
 * the ghosted block as long as reach <= cfg.mbc, which pcl_cellfn_apply checks.  The ghost cells read are the caller's:
 * fill them (pcl_halo_exchange, pcl_bc ...) in front of the launch.  qn() in a reach = 0 body is a compile error. */
int pcl_cellfn_compile_reach(int kind, const char *body, const char *preamble, int meqn, int maux, int ndim, int math,
                             int writes_aux, int reach, pcl_cellfn **out, long *code_size);
int pcl_cellfn_release(pcl_cellfn *f);          /* drops one reference; the compiled function stays cached for
                                                 * the life of the process (host memory: its code object) */
/* compiles done and cache hits of this process */
int pcl_cellfn_stats(long *compiles, long *cache_hits);
/* Host-only argument check of pcl_cellfn_apply / pcl_cellbc_apply: the handle is live and was compiled for these shape constants. */
int pcl_cellfn_check(const pcl_cellfn *f, int meqn, int maux, int ndim);
/* Where the handle's block sits in the global grid: lower[ndim] = lower edge of the GLOBAL grid, nstart[ndim] = global
 * index of the block's first interior cell (both 0 until set). */
int pcl_cellfn_geometry(pcl_solver *s, const double *lower, const int *nstart);
/* One launch on the solver's stream over the interior cells of the SELECTED register (pcl_select); a dq_src reads the
 * selected register and adds into PCL_REG_DQ.  params[nparams <= 16] travel by value with the launch.  Like pcl_src it
 * makes the next one-kernel step compute every tile and the next step exchange its halo again.  A function compiled
 * with reach > 0 needs reach <= cfg.mbc (PCL_EINVAL otherwise); a step_src / start_step of that kind first copies the
 * selected register into a scratch array of the handle (allocated at the first such launch, freed by pcl_destroy), on
 * the solver's stream, reads that copy and stores into the register; a dq_src reads the register itself.  The module is loaded
 * into the handle's device on first use and unloaded by pcl_destroy.  After a function that wrote aux the caller
 * refreshes the aux ghost cells: pcl_halo_exchange_aux, then pcl_bc_aux per dimension and side. */
int pcl_cellfn_apply(pcl_solver *s, pcl_cellfn *f, double t, double dt, const double *params, int nparams);
/* A boundary condition as a cell function (kind PCL_CELLFN_BC; writes_aux = 0): one launch on the solver's stream over the
 * ghost cells of side (idim, side: 0 lower, 1 upper) of the SELECTED register -- mbc layers times the WHOLE ghosted
 * extent of the transverse dimensions, corner cells included, one lane per ghost cell.  The body sees
 *     q[MEQN]      the ghost cell, read/write, initialised with     aux[MAUX]   the ghost cell's own aux, const
 *                  its current contents                              p[16]       the parameters of this launch
 *     c.t          time of the state being filled (stage time)      c.idim, c.side
 *     c.g          layer, 0 = next to the boundary face .. mbc-1    c.d[NDIM]   cell sizes
 *     c.i[NDIM]    GLOBAL 0-based indices of the ghost cell (negative on a lower side, >= n on an upper side, in the
 *                  normal and in the transverse directions);  c.x[NDIM] = lower + (i + 0.5) * d
 *     qin(m, r), auxin(m, r)   component m of the cell r cells inward from the boundary face on this ghost cell's own
 *                  normal line (r = 0: the first interior cell); r is clamped to [0, n[idim] - 1]
 * A component is stored only where its bits changed.  The caller keeps the order of apply_q_bcs: halo exchange, then per
 * dimension lower and upper, only on blocks that own that boundary.  The argument checks are host-only and come first;
 * otherwise the bookkeeping of pcl_bc_const. */
int pcl_cellbc_apply(pcl_solver *s, pcl_cellfn *f, int idim, int side, double t, const double *params, int nparams);
/* A functional: per-cell integrands reduced over the interior cells of the block (pyclaw.CellFunctional).  The body sees
 * what a cell function's body sees -- q[MEQN] and aux[MAUX], both const, c.t, c.i, c.x, c.d, p[16], with reach > 0 also
 * qn / auxn, which read the register itself; c.dt is 0 -- and assigns f[NOUT], which is zero on entry.  ops[nout],
 * 1 <= nout <= 8, name the operation of each output: the sum of f, the sum of |f|, or the largest / smallest f with
 * fmax / fmin semantics (a NaN integrand is passed over; the sums propagate it).  Host-only, no device needed; the
 * per-process cache and the counters of pcl_cellfn_stats; nout and ops are -D constants of the compile and part of
 * the key.  The handle is released with pcl_cellfn_release.  pcl_cellfn_compile / _compile_reach do not make such a
 * handle, and pcl_cellfn_apply / pcl_cellbc_apply refuse one. */
#define PCL_REDUCE_SUM 0
#define PCL_REDUCE_ABS_SUM 1
#define PCL_REDUCE_MAX 2
#define PCL_REDUCE_MIN 3
int pcl_cellfn_compile_reduce(const char *body, const char *preamble, int meqn, int maux, int ndim, int math,
                              int reach, int nout, const int *ops, pcl_cellfn **out, long *code_size);
/* Evaluates a functional on the interior cells of the SELECTED register, on the solver's stream, writes the nout values
 * to out (host memory) and returns when they are there.  Two launches: the compiled wrapper leaves one partial per
 * workgroup and output in a buffer of the handle (allocated at the first call for the block's size, freed by
 * pcl_destroy), a fixed kernel of the library reduces those.  Both combine in an order fixed by the block's shape --
 * cross-lane butterfly, wavefronts in order, partials in order, no atomics -- so the result is a function of the state,
 * the text and the shape alone and has the same bits on every call.  Ghost cells are never part of the reduction; with
 * reach > 0 they are read, and filling them is the caller's business.
 * A READ-ONLY call in the sense of the quiet tiles and of pcl_step_ahead below: it stores nothing into the state, sees
 * the state the caller knows (behind a step enqueued ahead: the accepted one), and that step is still adopted by the
 * next pcl_bc_step.  Like pcl_get_cells it ends with a synchronisation of the stream, so it waits for a step enqueued
 * ahead.  The argument checks are host-only and come first: PCL_EINVAL for a handle of another kind, for one compiled
 * for other shape constants (pcl_cellfn_check), for reach > cfg.mbc and for nparams > 16. */
int pcl_cellfn_reduce(pcl_solver *s, pcl_cellfn *f, double t, const double *params, int nparams, double *out);

/* ---- user-written Riemann solvers (cfg.rp = PCL_RP_CELL) ---------------------------------------------------------
 * The normal Riemann solver of one interface (Clawpack's rp1 / rpn2) as the text of a C++ function body.  The library
 * wraps it in a solver struct and compiles its own sweep kernel (the text of csrc/classic.hpp, with the flags of the
 * arithmetic mode `math`) with it at run time: the classic 1-D step and the x and y passes of the dimension-split 2-D
 * step then run the user's solver with the tiles, limiter, jump-free shortcut and Courant reduction of the built-in
 * solvers.  The body sees
 *     ql[MEQN], qr[MEQN]   the cells left and right of the interface (const)     p[8]   cfg.rp_params / pcl_cellrp_params
 *     ixy                  compile-time constant: 1 = x (always in 1-D), 2 = y
 *     wave[MWAVES][MEQN], s[MWAVES], amdq[MEQN], apdq[MEQN]   the results, zero on entry
 * the helpers of csrc/rp.hpp (dmax, dmin, dsqrt, fdiv, Recip) and whatever `preamble` declares.  For bitwise-equal ql
 * and qr the waves and fluctuations must be zero (any consistent solver): a wavefront without a jump takes the speeds
 * alone.  Diagnostics carry the body's line numbers ("riemann:3:...", "preamble:1:...").
 * Compile is host-only and shares the per-process cache and counters of the cell functions (pcl_cellfn_stats); the key
 * is (body, preamble, meqn, mwaves, ndim, math).  1 <= meqn, mwaves <= 8, ndim 1 or 2. */
typedef struct pcl_cellrp pcl_cellrp;
int pcl_cellrp_compile(const char *body, const char *preamble, int meqn, int mwaves, int ndim, int math, pcl_cellrp **out,
                       long *code_size);
/* The same for a solver with cell-wise coefficients: aux_index[0..naux) lists the components of the aux array (0-based)
 * the body reads.  The sweep stages those planes next to q in its tile, as it does for the built-in solvers with aux, and
 * the body also sees
 *     auxl[NAUX], auxr[NAUX]   the listed components, in list order, of the cells left and right of the interface (const);
 *                              Clawpack's "aux(1) = the value at the left edge of cell i" is auxr[0]
 * One list serves both sweeps; a body that reads another component per direction branches on ixy.
 * Contract: for bitwise-equal ql and qr the waves and fluctuations must be zero WHATEVER aux holds -- a wavefront without
 * a jump in q takes the speeds alone, each interface with its own auxl / auxr.  A flux-difference form over varying
 * coefficients breaks this; that is an f-wave solver: pcl_cellrp_compile_form with PCL_CELLRP_FORM_FWAVE.
 * The tile holds meqn + naux planes in a workgroup's 64 KB: meqn + naux <= 8 (65536 bytes / (8 bytes * the 1024 cells
 * of the y tile)); more is PCL_EINVAL with the limit in the message, and so are naux < 0 and a negative or repeated
 * index.  The list is part of the cache key (another order is another program); naux == 0 is pcl_cellrp_compile itself:
 * the same program, key and handle.  Host-only. */
int pcl_cellrp_compile_aux(const char *body, const char *preamble, int meqn, int mwaves, int ndim, int math, const int *aux_index,
                           int naux, pcl_cellrp **out, long *code_size);
/* The same with a TRANSVERSE body (Clawpack's rpt2 for one interface), which opens the unsplit 2-D step (method[2] >= 0)
 * to the solver: the code object then also holds the x and y phases of that step (csrc/classic.hpp: unsplit_x_kernel,
 * unsplit_y_kernel) around the two bodies.  Without an aux list the transverse body sees
 *     ql[MEQN], qr[MEQN]   the cells left and right of the interface whose fluctuation is split (const) -- the same pair
 *                          for A-dq and for A+dq of one interface; there is no imp
 *     asdq[MEQN], p[8]     the fluctuation and the parameters (const)
 *     ixy                  compile-time constant: the direction of the NORMAL solve; the split is across it
 *     bmasdq[MEQN], bpasdq[MEQN]   the down- and up-going parts, zero on entry
 * and with one
 *     q1[MEQN], aux1[NAUX]             the cell the fluctuation belongs to: left of the interface for A-dq, right for A+dq
 *     aux_below[NAUX], aux_above[NAUX] the listed components of its neighbours at the lower / upper transverse index
 * next to asdq, p, ixy and the results (a transverse body that needs both cells AND aux is not served).
 * Contract: for asdq all zero the results are zero -- a wavefront without a jump never calls the body.
 * Diagnostics: "transverse:<n>:...".  transverse != NULL needs ndim == 2, else PCL_EINVAL; the text is part of the cache
 * key; transverse == NULL is pcl_cellrp_compile_aux itself: the same program, key and handle.  The unsplit kernels take
 * 16 slices per workgroup for meqn <= 6 and 12 above (their static LDS against 160 KB).  Host-only. */
int pcl_cellrp_compile_t(const char *body, const char *transverse, const char *preamble, int meqn, int mwaves, int ndim, int math,
                         const int *aux_index, int naux, pcl_cellrp **out, long *code_size);
/* The same with a FORM: the two facts about the step that are template flags of the kernels, so that a handle is compiled
 * for them and serves them alone.
 *     PCL_CELLRP_FORM_FWAVE   the body assigns f-waves (cfg.fwave = 1; flux2fw.f / step1fw.f): the array is named
 *                             fwave[MWAVES][MEQN] in place of wave, everything else of the body's interface is unchanged
 *                             (the transverse body's too), all of it zero on entry.  The "equal ql and qr: zero waves"
 *                             contract does NOT apply to an f-wave body: no wavefront takes a jump-free shortcut, every
 *                             interface is solved, so a flux-difference solver over varying coefficients is served
 *     PCL_CELLRP_FORM_CAPA    the sweeps run with a capacity function (cfg.method[5] = mcapa >= 1, any component: it is a
 *                             run-time value); the body does not change.  The sweep tile holds one more plane:
 *                             meqn + 1 + naux <= 8, else PCL_EINVAL with the sum and the limit in the message
 * form == 0 is pcl_cellrp_compile_t itself: the same program, key and handle.  Any other form is part of the cache key, a
 * program of its own; only the kernels of that one form are compiled.  A bit outside the two is PCL_EINVAL.  Every refusal
 * comes before the compiler.  Host-only. */
#define PCL_CELLRP_FORM_FWAVE 1
#define PCL_CELLRP_FORM_CAPA 2
int pcl_cellrp_compile_form(const char *body, const char *transverse, const char *preamble, int meqn, int mwaves, int ndim,
                            int math, const int *aux_index, int naux, int form, pcl_cellrp **out, long *code_size);
/* Host-only: the PCL_CELLRP_FORM_* bits a live handle was compiled with. */
int pcl_cellrp_form(const pcl_cellrp *r, int *form);
/* pcl_cellrp_compile_form for ndim = 2 with the ONE-KERNEL form of the dimension-split 2-D step next to the sweeps: the
 * code object also holds step2ds_kernel (csrc/classic_fused.hpp: both sweeps on a 16 x 64 tile in LDS, q through HBM once
 * per step) around the body, in the handle's form.  A dimension-split solver with such a handle attached chooses between
 * the two forms of the step exactly as for a built-in solver that has the kernel: a wave-form body without an aux list
 * and without a capacity function gets quiet tiles, tile lists, row reuse, the column shortcut, the form trials and step
 * ahead -- all of which rest on the contract "bitwise-equal ql and qr: zero waves" alone; a body with an aux list or a
 * capacity function the kernel over the whole block without that bookkeeping; an f-wave body the f-wave instantiation, in
 * which no wavefront takes the shortcut.  The unsplit step of a handle with a transverse body is unchanged.
 * Another cache entry than the same call without it (key piece "onek"), a larger code object.  PCL_EINVAL before the
 * compiler, with the reason: meqn > 5 (the one-kernel tile holds up to 5 equations, the rule for every solver), and
 * everything pcl_cellrp_compile_form refuses.  There is no 1-D, 3-D or SharpClaw form of this call.  Host-only. */
int pcl_cellrp_compile_onek(const char *body, const char *transverse, const char *preamble, int meqn, int mwaves, int math,
                            const int *aux_index, int naux, int form, pcl_cellrp **out, long *code_size);
/* Host-only: has = 1 if a live handle carries the one-kernel step (pcl_cellrp_compile_onek), 0 for every other handle. */
int pcl_cellrp_onek(const pcl_cellrp *r, int *has);
/* The same body in the SHARPCLAW stages (cfg.kind = PCL_KIND_SHARPCLAW): the library compiles its SharpClaw kernels (the
 * text of csrc/sharpclaw.hpp) around the body in place of the classic sweeps -- the one reconstruction asked for and no
 * other: lim_type 1 (tvd2), 2 (WENO) or 3 (legacy WENO5) at weno_order 5, weno_order 7..17 (odd) with lim_type 2, for any
 * system; char_decomp = 1 (wave-based reconstruction) under pcl_create's conditions: ndim 1, lim_type 1 or 2, weno_order 5,
 * no PCL_CELLRP_FORM_FWAVE.  Everything else is PCL_EINVAL before the compiler.  The body, the preamble, the aux list and
 * `form` mean what they mean above (an f-wave body assigns fwave[][]; SharpClaw reads s, amdq and apdq alone).  The "equal
 * ql and qr: zero waves" contract is not relied on: SharpClaw solves every interface and the problem inside every cell,
 * both edge states of a cell with the cell's own aux values.
 * Plane limit: the tile of the SharpClaw kernel is 64 cells x TA strips per plane in the 64 KB a workgroup may declare; TA
 * is 16, or 8 in the y pass from six listed aux components on.  The x pass (and the 1-D pass) stages q and the capacity
 * function, meqn + capa <= 8; the y pass the listed aux components too, meqn + capa + naux <= 8 (<= 16 from naux = 6 on);
 * more is PCL_EINVAL with the sum and the limit.  char_decomp = 1 has no tile.
 * lim_type, weno_order and char_decomp are part of the cache key.  Such a handle serves pcl_create_cellrp with cfg.kind =
 * PCL_KIND_SHARPCLAW and nothing else.  Host-only. */
int pcl_cellrp_compile_sharp(const char *body, const char *preamble, int meqn, int mwaves, int ndim, int math, const int *aux_index,
                             int naux, int form, int lim_type, int weno_order, int char_decomp, pcl_cellrp **out, long *code_size);
/* Host-only: what a live handle was compiled for by pcl_cellrp_compile_sharp; three zeros for a classic handle. */
int pcl_cellrp_sharp(const pcl_cellrp *r, int *lim_type, int *weno_order, int *char_decomp);
/* The same body in the dimension-split 3-D step (cfg.ndim = 3, method[2] < 0, mbc = 2; step3ds): the library compiles the
 * x, y and z passes of its 3-D sweep kernel (csrc/classic.hpp: sweep3_kernel, DIR 1..3) around the body and nothing else.
 * ixy is 1, 2 or 3; the body, the preamble and the aux list mean what they mean above (maux may be 0: no list).  form may
 * carry PCL_CELLRP_FORM_CAPA only: PCL_CELLRP_FORM_FWAVE is PCL_EINVAL (the 3-D kernel has no f-wave form).
 * Plane limit: all three passes stage q, the listed aux components and the capacity function in one tile of the 64 KB a
 * workgroup may declare, 64 cells x (16 + 1) columns per plane in the y and z passes: meqn + naux + capa <= 7; more is
 * PCL_EINVAL with the sum and the limit.  Such a handle serves pcl_create_cellrp with cfg.ndim = 3 and nothing else, and a
 * 3-D configuration is served by such a handle alone: the calls above go on refusing ndim == 3, pcl_create goes on
 * refusing PCL_RP_CELL with ndim == 3, and pcl_create_cellrp refuses the unsplit 3-D step (method[2] >= 0: it needs rpt3 and
 * rptt3 bodies), cfg.fwave and every cfg.kind but PCL_KIND_CLASSIC for it.  One block.  Host-only. */
int pcl_cellrp_compile3(const char *body, const char *preamble, int meqn, int mwaves, int math, const int *aux_index, int naux,
                        int form, pcl_cellrp **out, long *code_size);
/* The same body in the SHARPCLAW stages of a 3-D solver (cfg.ndim = 3, cfg.kind = PCL_KIND_SHARPCLAW): the library compiles the
 * x, y and z passes of its 3-D SharpClaw kernel (csrc/sharpclaw.hpp: sharp3_kernel, DIR 1..3) of the one (lim_type,
 * weno_order) around the body and nothing else.  This is the only way SharpClaw runs in 3-D: no SharpClaw kernel of a
 * built-in 3-D solver is instantiated (the library's own vc_acoustics_3d runs as its body), pcl_create goes on refusing a
 * built-in id with ndim == 3 under SharpClaw, and pcl_cellrp_compile_sharp goes on refusing ndim == 3.  ixy is 1, 2 or 3;
 * the body, the preamble and the aux list mean what they mean above; char_decomp is 0.  A line is swept where both of its
 * transverse indices lie in 0 .. m+1 (the rule of the reference's 2-D flux2.f90, which has no 3-D counterpart).
 * Refused before the compiler (PCL_EINVAL, each with its reason): PCL_CELLRP_FORM_FWAVE (form may carry
 * PCL_CELLRP_FORM_CAPA only); lim_type outside 1..3; weno_order not odd in 5..17, or above 5 with lim_type != 2; meqn or
 * mwaves outside 1..8; meqn + capa + naux > 8 (the tile of each pass holds q, the capacity function and, in the y and z
 * passes, the listed aux components in the 64 KB a workgroup may declare).  lim_type and weno_order are part of the cache
 * key.  Such a handle serves pcl_create_cellrp with cfg.ndim = 3, cfg.kind = PCL_KIND_SHARPCLAW, the same lim_type,
 * cfg.mbc = (weno_order + 1) / 2, cfg.method[4] = 0 and method[5] > 0 if and only if it has PCL_CELLRP_FORM_CAPA; a classic
 * 3-D handle on such a configuration and such a handle on a classic configuration are PCL_EINVAL.  One block, no fused dq
 * source.  Host-only. */
int pcl_cellrp_compile3_sharp(const char *body, const char *preamble, int meqn, int mwaves, int math, const int *aux_index, int naux,
                              int form, int lim_type, int weno_order, pcl_cellrp **out);
/* pcl_cellrp_compile3 with the transverse solvers of the UNSPLIT 3-D step (cfg.method[2] >= 0; step3.f + flux3.f): rpt3 is
 * the inside of Clawpack's rpt3 for one interface, rptt3 (may be null) the inside of rptt3.  The code object also holds
 * the pieces kernels of the general unsplit step (csrc/classic3.hpp: pieces3_kernel, DIR 1..3); the library's own gather
 * kernel applies what they leave in scratch planes in the order of step3.f's loop nest.
 * Both texts see the compile-time constants ixyz (alias ixy: the direction of the normal solve, 1..3) and icoor (2: the
 * split is in the y-like direction ixyz+1, 3: in the z-like direction ixyz+2, cyclic) and p[8].  Without an aux list they
 * see ql[MEQN], qr[MEQN], the cells left and right of the interface (one pair for A-dq, A+dq and the correction wave; no
 * imp); with one, imp (1, 2), q1[MEQN] (the cell i-2+imp the fluctuation belongs to) and auxb[3][3][NAUX], auxb[a][b][k]
 * the k-th listed component of that cell's neighbour at y-like offset a-1 and z-like offset b-1.
 *     rpt3:   asdq[MEQN] in; assigns bmasdq[MEQN], bpasdq[MEQN] (zero on entry)
 *     rptt3:  impt (1: the input came out of a split that went down in the other transverse direction, 2: up) and
 *             bsasdq[MEQN] in; assigns cmbsasdq[MEQN], cpbsasdq[MEQN] (zero on entry)
 * For an all-zero input the results must be zero.  Diagnostics carry "rpt3:<n>" / "rptt3:<n>".
 * Refused (PCL_EINVAL, before the compiler): rptt3 without rpt3; PCL_CELLRP_FORM_FWAVE; PCL_CELLRP_FORM_CAPA together with
 * rpt3 (step3 with mcapa is not built for any solver).  Both texts null: pcl_cellrp_compile3 itself.
 * A handle with rpt3 alone serves method[2] = 0, 10 and 20, one with both 0, 10, 11, 20, 21 and 22 (pcl_create_cellrp
 * refuses the rest); either still serves the dimension-split step where meqn + naux <= 7, and the unsplit step alone above
 * that.  Attaching such a handle to an unsplit configuration allocates pcl_unsplit3_scratch_bytes of device memory, freed
 * by pcl_destroy; a failed allocation is refused with the bytes.  mbc = 2, one block.  Host-only. */
int pcl_cellrp_compile3t(const char *body, const char *rpt3, const char *rptt3, const char *preamble, int meqn, int mwaves,
                         int math, const int *aux_index, int naux, int form, pcl_cellrp **out, long *code_size);
/* Host-only: *trans3 = 0 (no 3-D transverse body), 1 (rpt3) or 2 (rpt3 and rptt3) of a live handle. */
int pcl_cellrp_transverse3(const pcl_cellrp *r, int *trans3);
/* The scratch of the general unsplit 3-D step: 14 * meqn doubles per cell, ghost cells included (the one rule,
 * csrc/sweep_args.hpp), and the bytes of it that live solvers of this process hold. */
long long pcl_unsplit3_scratch_bytes(int meqn, int nx, int ny, int nz, int mbc);
long long pcl_unsplit3_scratch_live(void);
/* Host-only: *has = 1 if the live handle was compiled with a transverse body, and then *slices (may be null) = the slices
 * per workgroup of its unsplit kernels; else *has = 0, *slices = 0. */
int pcl_cellrp_transverse(const pcl_cellrp *r, int *has, int *slices);
/* pcl_create of a PCL_RP_CELL solver and pcl_cellrp_attach in one call, so that the configuration is checked against what
 * the handle can do: method[2] >= 0 in 2-D (the unsplit step) is accepted if and only if the handle has a transverse
 * body, else PCL_EINVAL.  Every other refusal is pcl_create's and pcl_cellrp_attach's.  All argument checks are host-only
 * and come before the device is touched (no device, acceptable arguments: PCL_ENODEVICE).  pcl_create itself goes on
 * refusing method[2] >= 0 for PCL_RP_CELL: it cannot know the handle.  The unsplit step of such a solver runs whole
 * blocks, the y phase always in its tile form.
 * The form likewise: cfg.fwave != 0 is accepted if and only if the handle has PCL_CELLRP_FORM_FWAVE, cfg.method[5] > 0
 * (1 <= method[5] <= maux as for any solver) if and only if it has PCL_CELLRP_FORM_CAPA; every other combination is
 * PCL_EINVAL, in either direction.  pcl_create goes on refusing cfg.fwave and method[5] != 0 for PCL_RP_CELL.
 * SharpClaw likewise: cfg.kind = PCL_KIND_SHARPCLAW is accepted if and only if the handle was compiled by
 * pcl_cellrp_compile_sharp and its lim_type, (weno_order + 1) / 2 and char_decomp equal cfg.lim_type, cfg.mbc and
 * cfg.method[4] (and its form bits cfg.fwave and method[5] > 0, as above); such a handle on cfg.kind = PCL_KIND_CLASSIC, a
 * classic handle on SharpClaw and every mismatch are PCL_EINVAL with both sides in the message.  pcl_create goes on
 * refusing PCL_RP_CELL under SharpClaw.  One block (pcl_comm_init* refuses PCL_RP_CELL), no fused dq source
 * (pcl_sharp_fuse_dq_src refuses it: a source term runs as its own pass). */
int pcl_create_cellrp(const pcl_config *cfg, pcl_cellrp *r, pcl_solver **out);
/* Host-only: the list a live handle was compiled with; aux_index (may be null) gets *naux <= 8 entries. */
int pcl_cellrp_aux(const pcl_cellrp *r, int *naux, int *aux_index);
int pcl_cellrp_release(pcl_cellrp *r);
/* Host-only: the handle is live and was compiled for these constants (what pcl_cellrp_attach asks of it). */
int pcl_cellrp_check(const pcl_cellrp *r, int meqn, int mwaves, int ndim, int math);
/* Gives a PCL_RP_CELL solver its Riemann solver: the module is loaded into the handle's device (one attached at a time;
 * pcl_destroy unloads it).  Until then every step of such a solver is refused with PCL_ESTATE.  A handle whose largest
 * listed aux component is >= cfg.maux is refused (PCL_EINVAL, both numbers in the message) before anything is loaded, and
 * the sweeps of a solver that reads aux are refused (PCL_EINVAL) until pcl_put_aux has uploaded the array.  A solver
 * created unsplit (pcl_create_cellrp) refuses a handle without a transverse body (PCL_EINVAL), and any solver a handle
 * whose form (pcl_cellrp_form) is not the solver's cfg.fwave and method[5] > 0; the module attached before stays
 * attached.  The sweeps of a solver with a capacity function are refused until pcl_put_aux has uploaded the array. */
int pcl_cellrp_attach(pcl_solver *s, pcl_cellrp *r);
/* The body's p[0..nparams-1] from the next sweep on (nparams <= 8; the rest are zero): they travel by value with every
 * launch, so changing them compiles nothing. */
int pcl_cellrp_params(pcl_solver *s, const double *params, int nparams);

/* ---- SharpClaw (kind = PCL_KIND_SHARPCLAW) ----------------------------------------------------- */
/* Which register the put/get/bc/strip/halo calls act on (default PCL_REG_Q): the RK stages get
 * their ghost cells filled exactly like q (apply_q_bcs(stage), sharpclaw.py:546). */
int pcl_select(pcl_solver *s, int reg);
/* deltaq += dq_src(stage) of sharpclaw.py:232-235 evaluated by the LAST pass of every stage while it stores deltaq (or
 * its RK combination), for the built-in twin of the shock-bubble app's dq_Euler_radial
 * (apps/euler/2d/shockbubble/shockbubble.py:95-122): src_id = PCL_SRC_EULER_RADIAL with params {gamma1, ndim}; 0 switches
 * it off.  Needs euler_5wave_2d, lim_type 2 with mbc 3 (WENO5), no capacity function, aux(1) = radial coordinate. */
int pcl_sharp_fuse_dq_src(pcl_solver *s, int src_id, const double *params, int nparams);

/* sharpclaw1.flux1 / sharpclaw2.flux2 (sharpclaw.py:385,558; flux1.f90, flux2.f90): dq register :=
 * dt * dq/dt of the selected register (ghost cells must be filled); *cfl = max Courant number (global
 * after pcl_comm_init). */
int pcl_sharp_dq(pcl_solver *s, double dt, double *cfl);
/* One Runge-Kutta stage in two kernels (2-D): dq of the selected register (pcl_sharp_dq) with the
 * combination that consumes it fused into the last directional pass, so deltaq is never written:
 *   op 1: D = A + dq/ca      op 2: D = ca*A + cb*(B + dq)      op 5: D = A + cb*B + cc*dq
 * (the expressions of SharpClawSolver.step, sharpclaw.py:168-206, in the numpy evaluation order).
 * The stage's Courant number (all-reduced over the blocks in a decomposed run) is returned in *cfl; the
 * result becomes register D only if cfl <= cfl_max (dq() raises CFLError before the update otherwise,
 * sharpclaw.py:228-230).  D, A, B in {PCL_REG_Q, PCL_REG_S1, PCL_REG_S2}; D's ghost cells are left
 * unset (the next dq fills them, like the reference's apply_q_bcs on each stage). */
int pcl_sharp_stage(pcl_solver *s, double dt, int op, int D, int A, int B, double ca, double cb, double cc,
                    double cfl_max, double *cfl);

/* pcl_sharp_dq / pcl_sharp_stage preceded by the stage's apply_q_bcs (sharpclaw.py:347, solver.py:354-381) in the
 * same call: halo exchange of the selected register in a decomposed run, then the physical BCs (`bc`, `cstate` as
 * for pcl_bc_step: 2*ndim types, <0 = no fill on that side, PCL_BC_CUSTOM = constant state).  In a decomposed 2-D
 * run the ghost frame is built on the halo stream while the x pass runs the tiles that read no ghost cell
 * (PCL_HALO_OVERLAP=0 keeps everything on one stream). */
int pcl_sharp_bc_dq(pcl_solver *s, const int *bc, const double *cstate, double dt, double *cfl);
int pcl_sharp_bc_stage(pcl_solver *s, const int *bc, const double *cstate, double dt, int op, int D, int A, int B,
                       double ca, double cb, double cc, double cfl_max, double *cfl);

/* Register arithmetic of the Runge-Kutta schemes (sharpclaw.py:168-206), evaluated in the order
 * written: op 1: D = A + B/ca   2: D = ca*A + cb*(B + C)   3: D = A/ca + cb*B
 *          4: D = ca*A - cb*B   5: D = A + cb*B + cc*C
 *          6: C = A/ca + cb*B, then D = cc*C - 5*B with D == B (ops 3 and 4 of SSP104's mid-step, sharpclaw.py:186-187,
 *             in one pass over the registers).  D, A, B, C are PCL_REG_* ids. */
int pcl_rk_op(pcl_solver *s, int op, int D, int A, int B, int Cc, double ca, double cb, double cc);

/* ---- explicit Runge-Kutta schemes from a Butcher tableau (time_integrator = 'RK' and the named tableaus) -------------
 * y_i = q + sum_j a_ij K_j,  K_i = dt L(y_i),  q <- q + sum_j b_j K_j, with K_j kept in stage registers of their own.
 * All three calls check their arguments on the host before any device call and leave the handle as it was when they
 * refuse: PCL_ESTATE on a classic solver, and (take, lincomb) before any stage register exists; PCL_EINVAL otherwise.
 *
 * pcl_rk_stages: hold exactly `nstages` stage registers (0 .. PCL_RK_MAX_STAGES), each the size of q and zero-filled;
 * 0 frees them, pcl_destroy does too.  A count that is already held is kept as it is, any other frees the registers held
 * (after a synchronisation of the stream) and allocates anew.  nstages < 0 changes nothing.  *held (may be null) gets the
 * number held after the call.  If the memory is not there nothing is held, and PCL_EHIP's message names the stages and the
 * bytes asked for.  A solver that never calls this allocates nothing for them. */
int pcl_rk_stages(pcl_solver *s, int nstages, int *held);
/* What pcl_sharp_dq / pcl_sharp_bc_dq (and a dq_src after them) left in PCL_REG_DQ becomes K_stage, without a copy: the
 * two buffers swap their names, so PCL_REG_DQ then holds what K_stage held, for the next dq to write over.  The stage's
 * Courant number was returned by the dq call. */
int pcl_rk_take(pcl_solver *s, int stage);
/* D = A + coef[0]*K_{stages[0]} + ... + coef[n-1]*K_{stages[n-1]} over the whole allocation, ghost cells included, n <=
 * PCL_RK_MAX_STAGES, one kernel.  Per element r = A, then r = r + coef[k]*K for ascending k: in the exact and strict
 * modes every product is rounded before its sum (no FMA), `fast` may contract.  A term whose coefficient is exactly 0.0
 * is dropped on the host and its register is not read; every other coefficient is multiplied, 1.0 included.  D, A in
 * {PCL_REG_Q, PCL_REG_S1, PCL_REG_S2}; D == A is served in place; D = PCL_REG_K0 + j with j among `stages` is refused as
 * aliasing an input.  D's ghost cells are left unset, as by pcl_rk_op. */
int pcl_rk_lincomb(pcl_solver *s, int D, int A, int n, const int *stages, const double *coef);

int pcl_sync(pcl_solver *s);

/* Timing hooks for bench.py: HIP events recorded on the solver's compute stream. */
int pcl_timer_start(pcl_solver *s);
int pcl_timer_stop(pcl_solver *s, float *ms);
/* Cumulative device time (ms) and launch count of the sweep kernels since the last reset, from HIP events around
 * the sweep launches (enable before use).  enable = 0: off; 1: every step; N > 1: every N-th step (the event
 * records sit between the kernels and cost a few microseconds of dispatch gap each; sampling keeps the average
 * launch duration and removes most of that). */
int pcl_kernel_timing(pcl_solver *s, int enable);
int pcl_kernel_timing_read(pcl_solver *s, double *ms_total, long *launches);
/* The dimension-split 2-D step has two forms with identical results (step2ds.f:83-159 as x pass + y pass, or both sweeps
 * in one kernel, q through HBM once per step); under pcl_step_hyperbolic / pcl_bc_step one block runs the faster one,
 * decided afresh every 256 steps: where the last one-kernel launch ran over a tile list of at most a quarter of the tiles the
 * one kernel stays without a trial (a rule on the state, not on timing), otherwise a few steps of each form are timed
 * (PCL_TUNE_FUSED_STEP = 0 / 1 pins a form).  The one-kernel form exists for mbc = 2 and
 * euler_5wave_2d, acoustics_2d, advection_2d, shallow_2d, vc_acoustics_2d, vc_advection_2d and psystem_fwave_2d, with or
 * without a capacity function (aux planes and aux(mcapa) are staged in the kernel's tile next to q); decomposed blocks of
 * the last three, and of any solver with a capacity function, keep the two passes, as does mbc > 2.  Since the last pcl_kernel_timing reset: cumulative device time (ms)
 * and sampled launch count of the one-kernel step (pcl_kernel_timing_read holds the two passes), and the steps each
 * form has run. */
int pcl_step_form_stats(pcl_solver *s, double *ms_total, long *launches, long *steps_one_kernel, long *steps_two_pass);
/* Quiet tiles of the one-kernel step (on by default): a tile whose update was the identity in the previous step, with
 * its 8 neighbours, is not computed again -- same bits, same Courant number.  enable = 0 computes every tile.  Solvers
 * that read aux arrays and states with a capacity function compute every tile of every step.  Any call
 * other than the step itself and read-only calls makes the next step compute every tile. */
int pcl_tile_skip(pcl_solver *s, int enable);
/* tiles the last one-kernel step computed and skipped (both 0 when no one-kernel step of the whole block has run); a
 * skipping step ran over the tile list built behind the step before it, in the kernel that handed its Courant number
 * over */
int pcl_tile_skip_stats(pcl_solver *s, long *computed, long *skipped);
/* internal, for the test suite only (not part of the user API): the tile grid (*ntx x *nty tiles of 12 x 60 owned cells) and, when host is not null and the last one-kernel
 * step could skip, the per-tile quiet words it read (row-major, one byte per wavefront; not the words the list built
 * behind it wrote); makes the next step compute every tile */
int pcl_tile_words(pcl_solver *s, unsigned *host, int *ntx, int *nty);
/* internal, for the test suite only: the listed tiles of the last one-kernel step by class -- *na had computed something
 * in the step before, *nq had been quiet there (both 0 when that step did not run over a list); makes the next step
 * compute every tile */
int pcl_tile_list_classes(pcl_solver *s, long *na, long *nq);
/* The ring check of the one-kernel step's listed tiles (on by default): a listed tile that was quiet in the step before
 * compares the cells around its own with them and, where all are equal, is done without loading the tile -- same bits,
 * same Courant number.  enable = 0: every listed tile is loaded and swept.  Not under the fused source. */
int pcl_tile_ring(pcl_solver *s, int enable);
/* internal, for the test suite only: how many listed tiles of the last one-kernel step the ring check settled (0 when
 * that step did not run over a list); makes the next step compute every tile */
int pcl_tile_ring_stats(pcl_solver *s, long *short_path);
/* Row reuse of the one-kernel step (on by default): an x sweep whose row, halo columns included, holds the same bits as
 * the row the wavefront swept before it takes that row's result instead of computing it again -- same bits, same
 * Courant number.  enable = 0: every row is swept.  Solvers without aux arrays and without a capacity function. */
int pcl_tile_rowreuse(pcl_solver *s, int enable);
/* internal, for the test suite only: the x sweeps the last one-kernel step of the whole block reused, over the tiles it
 * computed (0 when none has run); makes the next step compute every tile */
int pcl_tile_rowreuse_stats(pcl_solver *s, long *sweeps_reused);
/* Column shortcut of the one-kernel step (on by default): a y sweep whose four columns are each constant over the 16
 * rows of the tile's window, while the columns differ from each other, computes the wave speeds of its cells and stores
 * nothing -- the update of every stored cell is the identity there.  Not taken where a stored cell holds a -0 or a
 * non-finite component.  Same bits, same Courant number, same quiet words.  enable = 0: such sweeps run the full solve.
 * Solvers without aux arrays and without a capacity function. */
int pcl_tile_ycol(pcl_solver *s, int enable);
/* internal, for the test suite only: the y-sweep calls (four columns each) of the last one-kernel step of the whole block
 * that took the column shortcut, over the tiles it computed (0 when none has run); makes the next step compute every
 * tile */
int pcl_tile_ycol_stats(pcl_solver *s, long *groups);
/* hyperbolic steps (classic) / right-hand sides (SharpClaw) attempted since pcl_create, rejected ones included */
int pcl_step_count(pcl_solver *s, long *steps);

/* ---- step ahead: the next step is enqueued before pcl_bc_step returns ------------------------------------------
 * A caller that steps with a variable dt learns a step's Courant number when pcl_bc_step returns, computes the next dt
 * and comes back; the device idles meanwhile.  Armed (on != 0; off by default), pcl_bc_step enqueues the step after the
 * one it was asked for itself, before it returns, whenever that step ran as the one-kernel dim-split 2-D step over the
 * whole undecomposed block (mbc 2, no aux arrays, no capacity function), its Courant number c is finite with
 * 0 < c < cfl_max, and the step to come is an ordinary one-kernel step of its form window: with the boundary spec of
 * that call and dt' = pcl_step_ahead_dt(dt, c, cfl_desired, dt_max) (on = 1: the loop of evolve_to_time(tend)) or
 * dt' = dt (on = 2: a caller that keeps dt after an accepted step, as evolve_to_time does when it is called for one
 * step at a time).  Only short launches are run ahead of -- the last one ran over at most 4096 tiles or a quarter of
 * the grid -- since what is saved is one host turn-round per step and what a wrong guess costs is a whole launch.  The
 * state is not advanced and nothing is counted.  The next pcl_bc_step ADOPTS the pending step -- the result becomes the state, the counters advance, the call
 * waits for the Courant number -- if its dt has the same 64 bits as dt', its bc and constant states are bytewise the
 * same, and only read-only calls (pcl_get_q, pcl_get_cells, pcl_get_strip, pcl_cellfn_reduce, pcl_sync, the timers, pcl_step_count,
 * pcl_step_form_stats; they see the state the caller knows) came in between.  Otherwise the pending step is DROPPED: a
 * finished kernel whose output nobody uses; the call proceeds as if nothing had been enqueued, and its one-kernel launch
 * computes every tile.  A drop with nothing in between means the caller follows another rule: the next step is not run
 * ahead of, then the next two, four, ... up to 64 while that goes on; an adopted step ends it.  Results are the same bits either way: an adopted step is the launch the call would have made.
 * pcl_undo_step, the tile hooks (pcl_tile_words, pcl_tile_list_classes, pcl_tile_*_stats) and pcl_step_ahead itself
 * drop a pending step first; behind such a drop pcl_tile_skip_stats still reports the last step the caller asked for,
 * the other hooks report nothing (as behind a step that was no one-kernel step).
 * The one restriction, and why arming is explicit: the launch enqueued ahead overwrites the pre-step buffer of the step
 * just taken, so behind an ACCEPTED step (c < cfl_max) of an armed solver pcl_undo_step returns PCL_ESTATE.  A step
 * with c >= cfl_max is never run ahead of: it can be undone and retaken as before. */
int pcl_step_ahead(pcl_solver *s, int on, double cfl_desired, double cfl_max, double dt_max);
/* the dt of that rule: x = dt * cfl_desired / cfl evaluated left to right in double, then x < dt_max ? x : dt_max --
 * what Python's min(dt_max, dt * cfl_desired / cfl) gives, bit for bit; a pure host function */
double pcl_step_ahead_dt(double dt, double cfl, double cfl_desired, double dt_max);
/* steps enqueued ahead since pcl_create, adopted, dropped; not a read-only call: a pending step is dropped by the
 * next pcl_bc_step */
int pcl_step_ahead_stats(pcl_solver *s, long *enqueued, long *adopted, long *dropped);

/* ---- multi-GPU: one block per process, RCCL over xGMI -------------------------------- */
/* Replaces PETSc DMDA globalToLocal (src/petclaw/state.py:254-269) and Vec.max
 * (src/petclaw/cfl.py:29-31).  uid is the 128-byte ncclUniqueId produced by
 * pcl_comm_unique_id() on rank 0 and distributed by the caller (any side channel).
 * neighbors[8]: rank of the W,E,S,N,SW,SE,NW,NE neighbour block or -1 (physical
 * boundary without periodic wrap). */
int pcl_comm_unique_id(char uid[128]);
int pcl_comm_init(pcl_solver *s, int nranks, int rank, const char uid[128],
                  const int neighbors[8]);
/* Exchange-ahead for the overlapped dimension-split 2-D step (pcl_bc_step): with on = 1 the halo exchange of the NEW
 * state is enqueued on the halo stream right behind the y pass that produced it -- it travels while the Courant number
 * is handed over, the host decides accept / retake and the next x pass starts its interior tiles -- and the next
 * pcl_bc_step skips its own exchange when nothing has touched the state in between (any other call that changes q
 * or its ghost cells makes it exchange again; a rejected step goes back to the pre-step buffer, whose ghost frame is
 * still filled).  petclaw has no counterpart (globalToLocal is blocking, petclaw/state.py:254-262).  EVERY rank of
 * the communicator must make the same choice (the order of operations on the communicator depends on it):
 * pcl_halo_can_overlap tells whether this rank's block qualifies (decomposed, dim-split 2-D, interior x-pass tiles,
 * PCL_HALO_OVERLAP=1); the caller agrees over all ranks (pyclaw_amd/clawpack.py) and then switches it on everywhere.
 * pcl_halo_can_overlap: 0 no, 1 yes, 2 yes and the block can also run the one-kernel form of the step (both sweeps in
 * one launch) with interior / rim tile subsets.  The rule (csrc/halo_plan.hpp: OverlapPlan::offers): 0 unless a
 * communicator is set up, the solver takes the classic dimension-split 2-D step with at most 8 equations and
 * PCL_HALO_OVERLAP is 1 (set or not); else 2 if the block may take the one-kernel step and its tiles leave an interior
 * box; else 1 if the x pass' tiles leave an interior box and the two-pass overlap is not off by default -- it is, with
 * PCL_HALO_OVERLAP not set, for the aux-free solvers of the one-kernel step without a capacity function; else 0.  The
 * one-kernel form sends the new state's halo behind its RIM tiles, beside the
 * interior launch and BEFORE the Courant number's all-reduce: on = 2 selects that order and is only valid when every
 * rank reported 2; on = 1 keeps the two-pass order (all-reduce, then the exchange) on every rank. */
int pcl_halo_can_overlap(pcl_solver *s, int *yes);
int pcl_halo_exchange_ahead(pcl_solver *s, int on);
/* The same decomposed device path with a host-staged wire instead of RCCL (diagnostics, and multi-process tests on
 * ONE device: RCCL refuses two ranks per GPU).  Packed strips go to pinned host memory, `xfn` carries them between
 * the processes, the received strips go back up; the CFL maximum goes through `rfn`.  send/recv: all 8 directions'
 * strips back to back, direction d at doubles [off[d]*nm, (off[d]+cnt[d])*nm); what is SENT towards d arrives in the
 * receiver's region opposite(d).  Both callbacks return 0 on success and are called by every rank of the group at
 * the same points (collectives).  No reference counterpart. */
typedef int (*pcl_host_exchange_fn)(void *user, const double *send, double *recv, const long *off, const long *cnt,
                                    const int *nbr, int nm);
typedef int (*pcl_host_reduce_fn)(void *user, double *value);     /* in-place max over the ranks */
int pcl_comm_init_host(pcl_solver *s, int nranks, int rank, const int neighbors[8], pcl_host_exchange_fn xfn,
                       pcl_host_reduce_fn rfn, void *user);
/* Host-only argument check of pcl_comm_init (no GPU, no RCCL): rank inside 0..nranks-1, every neighbour a
 * rank of the communicator or -1, a self-neighbour only on both faces of a dimension.  pcl_comm_init runs it
 * first, so misuse fails with a message instead of RCCL's "invalid usage". */
int pcl_comm_check(int nranks, int rank, const int neighbors[8]);
int pcl_halo_exchange(pcl_solver *s);          /* faces + corners, width mbc            */
int pcl_halo_exchange_aux(pcl_solver *s);
int pcl_allreduce_max(pcl_solver *s, double *value);
/* Host-only helper (no GPU needed): the cell window [i0,i0+ni) x [j0,j0+nj) of a block of
 * I x J cells (ghosts included, width mbc) that is SENT towards direction dir (send=1: interior
 * cells next to that edge/corner) or FILLED from direction dir (send=0: ghost cells).  dir:
 * 0..7 = W,E,S,N,SW,SE,NW,NE.  Exactly the geometry the device pack/unpack kernels use. */
int pcl_halo_region(int dir, int send, int I, int J, int mbc, int out_i0_j0_ni_nj[4]);
/* Host-only helper (no GPU needed): the ghost-cell rule of the built-in boundary conditions (solver.py:384-452) as the
 * kernels apply it.  Cell k of a dimension of n cells (ghosts included, width mbc) whose lower / upper side has the
 * type lo / hi (PCL_BC_*, or -1: no fill on that side) takes its value from cell out[0]; out[1] = 1: the normal
 * momentum component changes sign (reflecting; never for an aux array); out[2] = 1: the value is the constant state
 * of side out[3] (0 lower, 1 upper) instead (PCL_BC_CUSTOM).  An interior cell, and a ghost cell of a side without a
 * fill, maps to itself. */
int pcl_ghost_map(int k, int n, int mbc, int lo, int hi, int out_src_neg_cst_side[4]);
/* Host-only helpers (no GPU needed), for the test suite: three host state machines of the dim-split 2-D step driven
 * through n scripted events, each on a fresh object, the decisions written to out[i].
 * pcl_step_form_trace (csrc/step_form.hpp), event[i]: 0 a step, begin(can = a[i], tune = b[i], listed[i], ntiles) then
 * end(seconds[i]): out = form | 2 * timed; 1 next_is_plain_onek(can = a[i], mode = b[i]); 2 adopted(mode = b[i]) and
 * 3 ran(form = a[i]) and 4 forget_last(): out = last(); 5 out = the steps counted in form a[i].
 * pcl_step_ahead_trace (csrc/step_ahead.hpp), armed once with the first four arguments; event i has the spec bc[4 i ..],
 * cstate[32 i ..]; event[i]: 0 out = wants(c = x[i], ran[i], ntiles[i], next_plain_onek = flag[i]); 1 out_dt =
 * next_dt(dt = x[i], c = y[i]); 2 enqueued(dt = x[i], seq = i, spec, ran[i]); 3 out = matches(spec, dt = x[i],
 * carry = flag[i]); 4 missed(); 5 adopted(); 6 out = dropped(), out_dt = the tile count then reported.
 * pcl_halo_plan_trace (csrc/halo_plan.hpp).  Facts are the bits active 1, split2 2, sel0 4, onek_ok 8, onek_family 16,
 * onek_box 32, x_box 64; buffers are ids 1..7 (distinct addresses inside the function), 0 the null buffer.  event[i]:
 * 0 configure(overlap = a[i], set = b[i]); 1 set_exchange_ahead(a[i]); 2 out = offers(facts a[i]); 3 plan(facts a[i],
 * state buffer b[i]): out = order | 8 * onek | 16 * have | 32 * send_ahead, order 0 not overlapped, 1 rim first,
 * 2 exchange in front, 3 test order, 4 interior first; 4 out = filled(a[i]); 5 exchanged(a[i]); 6 written(a[i]);
 * 7 touched(); 8 failed(); 9 out = unsplit_overlaps(active = a[i]); 10 out = sharp_overlaps(active = a[i], ndim = b[i]);
 * 11 out = frame_sequential(overlapping = a[i]).
 * pcl_gauge_log_trace (csrc/gauge_log.hpp): event[i]: 0 arm with capacity a[i]; 1 a step, value = the slot it writes or
 * -1 (refused: the log is full); 2 pcl_undo_step and 3 pcl_restore, value = 1 if a record was taken back; 4 a read, value
 * = the records it returns; 5 disarm.  out[4 i ..] = value, records held, whether the last step's record is still the
 * newest (what an undo would take), armed -- all behind the event. */
int pcl_step_form_trace(long n, const int *event, const int *a, const int *b, const long *listed, long ntiles,
                        const double *seconds, int *out);
int pcl_step_ahead_trace(int on, double cfl_desired, double cfl_max, double dt_max, long n, const int *event,
                         const int *flag, const double *x, const double *y, const long *ran, const long *ntiles,
                         const int *bc, const double *cstate, int *out, double *out_dt);
int pcl_halo_plan_trace(long n, const int *event, const int *a, const int *b, int *out);
int pcl_gauge_log_trace(long n, const int *event, const int *a, int *out);

/* ---- debug / self-test --------------------------------------------------------------- */
/* Runs the wavefront neighbour-shift primitive on 64 values: left[l]=in[l-1],
 * right[l]=in[l+1] (the end lane without a source reads 0). */
int pcl_debug_wave_shift(const double *in64, double *left64, double *right64);

#ifdef __cplusplus
}
#endif
#endif /* PYCLAW_AMD_H */
