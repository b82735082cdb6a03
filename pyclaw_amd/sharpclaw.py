r"""
SharpClaw (method-of-lines) solvers on MI355X (reference: src/pyclaw/sharpclaw.py).

``SharpClawSolver1D`` / ``SharpClawSolver2D`` / ``SharpClawSolver3D`` keep the reference's attributes, Runge-Kutta
schemes (Euler, SSP33, SSP104: sharpclaw.py:152-210) and CFL handling (``CFLError`` inside
``dq`` => ``step`` returns False and ``evolve_to_time`` retakes the step).  ``dq_hyperbolic``
(sharpclaw.py:343-447, 515-563: ``sharpclaw1.flux1`` / ``sharpclaw2.flux2``) runs in the HIP
kernel of csrc/sharpclaw.hpp; the stage registers and the register arithmetic of the RK
schemes live on the device too (``pcl_rk_op`` evaluates each formula in the order the
reference's numpy expressions do).

``time_integrator`` may also name an explicit Runge-Kutta scheme by its Butcher tableau: ``'RK'`` with ``solver.a`` (s x s,
strictly lower triangular), ``solver.b`` and ``solver.c`` (s each, ``c[0] == 0``; ``c`` is taken as given), 1 <= s <= 16, as
upstream PyClaw spells it, or one of the named entries of ``rk_tableaus.TABLEAUS`` -- ``'SSP22'`` (Heun), ``'RK44'`` (the
classical method), ``'DP5'`` (the six stages of Dormand and Prince's fifth-order solution, no step-size control).  Each stage
derivative has a register of its own on the device (``pcl_rk_stages``; the size of q each, none for the three schemes above),
a stage's increment becomes ``K_i`` by a pointer swap (``pcl_rk_take``) and one kernel forms the combinations in a fixed order
(``pcl_rk_lincomb``).  ``cfl_max`` and ``cfl_desired`` keep the SharpClaw defaults 2.5 / 2.45 whatever the scheme: those are
SSP104's and too large for most tableaus, so a user of ``'RK'`` / ``'RK44'`` / ... sets them; nothing is changed silently.

Implemented reconstruction: ``lim_type=2`` with ``weno_order`` 5 .. 17 (the PyWENO-generated ``weno5`` ...
``weno17``, float32-rounded literals included; orders above 5 for the 1-D solvers and advection_2d, acoustics_2d,
euler_5wave_2d) and ``lim_type=3`` (the legacy ``weno5`` of reconstruct.f90,
the one the reference's golden ``test/ac_sc_solution`` was produced with) and ``lim_type=1`` (tvd2);
``char_decomp=0``, or ``1`` (wave-based reconstruction) in 1-D with ``lim_type`` 1 or 2; ``tfluct_solver=False``.
``solver.fwave`` is ``True`` for ``rp_psystem_fwave_2d`` and only for it (``rp_elasticity_fwave_1d`` is a classic-only
solver).

``solver.rp`` may be a user-written ``riemann.CellRiemann(..., sharpclaw=True)``: ``setup()`` compiles the SharpClaw kernels
around its body for this solver's ``lim_type``, ``weno_order`` and ``char_decomp`` (every order 5 .. 17 for any system), on
one block, with a ``dq_src`` as its own pass.

``SharpClawSolver3D`` runs through such solvers alone: ``solver.rp`` is a ``riemann.SharpCellRiemann3D`` (the library's own
3-D solver as ``apps.problems.VC_ACOUSTICS_3D_RP``), compiled into the x, y and z passes of ``sharp3_kernel``.  The
reference has no ``flux3.f90``; a line is swept where both of its transverse indices lie in ``0 .. m+1``, the rule of
``flux2.f90`` with one more index.  Not served in 3-D: built-in solvers, ``char_decomp``, ``fwave``, decomposed runs.
"""
import ctypes

import numpy as np

from . import _lib, riemann, rk_tableaus
from .solver import CellFunction, CellStartStep, Solver

Q, S1, S2, DQ, TMP = 0, 1, 2, 3, 4


class CFLError(Exception):
    """Error raised when cfl_max is exceeded.  Is this a reasonable mechanism for handling that?"""

    def __init__(self, msg):
        super(CFLError, self).__init__(msg)


def start_step(solver, solution):
    r"""Dummy routine called before each step (sharpclaw.py:26-31)."""
    pass


class DeviceDqSource(object):
    """A SharpClaw source term (``solver.dq_src``) that libpyclaw_amd evaluates on the device.

    It is also a plain ``dq_src(solver,state,dt)`` callable (numpy, same arithmetic), which is what runs -- through
    the host, like any Python ``dq_src`` -- for a configuration the device kernel is not built for."""

    src_id = 0

    def fusable(self, solver, state):
        return False

    def __call__(self, solver, state, dt):
        raise NotImplementedError


class EulerRadialDqSource(DeviceDqSource):
    """Geometric source of the 2-D Euler equations with radial symmetry in SharpClaw form -- the ``dq_Euler_radial``
    callback of the shock-bubble app (apps/euler/2d/shockbubble/shockbubble.py:95-122).  aux[0] must hold the radial
    coordinate.  With euler_5wave_2d, WENO5 and no capacity function the last pass of every stage adds it while
    storing deltaq (``pcl_sharp_fuse_dq_src``): no extra pass over q."""

    src_id = 1

    def __init__(self, gamma1, ndim=2):
        self.gamma1 = float(gamma1)
        self.ndim = int(ndim)
        self.params = np.array([self.gamma1, float(self.ndim)], dtype=np.float64)

    def fusable(self, solver, state):
        return (solver.ndim == 2 and riemann.get(solver.rp).name == 'euler_5wave_2d' and solver.lim_type == 2
                and solver.weno_order == 5 and state.mcapa < 0 and state.maux >= 1)

    def __call__(self, solver, state, dt):
        q, rad = state.q, state.aux[0, :, :]
        rho = q[0, :, :]
        u = q[1, :, :] / rho
        v = q[2, :, :] / rho
        press = self.gamma1 * (q[3, :, :] - 0.5 * rho * (u ** 2 + v ** 2))
        dq = np.empty(q.shape)
        dq[0, :, :] = -dt * (self.ndim - 1) / rad * q[2, :, :]
        dq[1, :, :] = -dt * (self.ndim - 1) / rad * rho * u * v
        dq[2, :, :] = -dt * (self.ndim - 1) / rad * rho * v * v
        dq[3, :, :] = -dt * (self.ndim - 1) / rad * v * (q[3, :, :] + press)
        dq[4:, :, :] = 0
        return dq


class CellDqSource(CellFunction, DeviceDqSource):
    """A SharpClaw source term (``solver.dq_src``) as a cell function (see ``CellFunction``): the body reads the stage's
    ``q[MEQN]`` (const) and fills ``dq[MEQN]``, zero on entry, with what the Python ``dq_src(solver, state, dt)`` would
    return for this cell; ``deltaq = deltaq + dq[m]`` follows on the device.  ``c.t`` is the stage time, ``c.dt`` the
    step length.

    It is never fused into the last pass of a stage: every stage runs its directional passes, this launch (one read of
    q, one read and write of deltaq) and the Runge-Kutta combination as separate kernels.

    ``reach > 0`` gives the body ``qn`` / ``auxn`` (see ``CellFunction``), e.g. for a 4th-order Laplacian with
    ``reach=2``.  The stage's register was filled by the ``apply_q_bcs(stage)`` of ``dq_hyperbolic`` just before and q
    is const here, so the launch needs neither an extra ghost fill nor a snapshot: ``qn`` reads the register itself."""

    kind = 2
    src_id = 0

    def __init__(self, body, params=(), preamble="", reach=0):
        CellFunction.__init__(self, body, params, preamble, reach=reach)

    def __call__(self, solver, state, dt):
        raise NotImplementedError("a CellDqSource runs on the device only")


class _StageState(object):
    """What a Python custom-BC callback sees of an RK stage: time, grid, aux (solver.py:283-291)."""

    def __init__(self, state):
        self.grid = state.grid
        self.aux = state.aux
        self.aux_global = state.aux_global
        self.decomp = state.decomp
        self.t = state.t
        self.q = None
        self.mcapa = state.mcapa


class SharpClawSolver(Solver):
    r"""Superclass for all SharpClawND solvers (sharpclaw.py:34-283)."""

    def __init__(self, data=None):
        for attr in ['limiters', 'start_step', 'lim_type', 'weno_order', 'time_integrator', 'char_decomp',
                     'aux_time_dep', 'mwaves']:
            if attr not in self._required_attrs:
                self._required_attrs.append(attr)
        self._default_attr_values['limiters'] = [1]
        self._default_attr_values['start_step'] = start_step
        self._default_attr_values['lim_type'] = 2
        self._default_attr_values['weno_order'] = 5
        self._default_attr_values['time_integrator'] = 'SSP104'
        self._default_attr_values['char_decomp'] = 0
        self._default_attr_values['tfluct_solver'] = False
        self._default_attr_values['aux_time_dep'] = False
        self._default_attr_values['kernel_language'] = 'HIP'
        self._default_attr_values['mbc'] = 3
        self._default_attr_values['fwave'] = False
        self._default_attr_values['cfl_desired'] = 2.45
        self._default_attr_values['cfl_max'] = 2.5
        self._default_attr_values['dq_src'] = None
        self._default_attr_values['math'] = 'exact'
        self.rp = None
        self._user_rp = None         # the riemann.CellRiemann of this setup() and the params the library last got
        self._user_rp_sent = None
        self._rk = None              # (a, b, c) of a scheme given by its tableau: set by setup()
        super(SharpClawSolver, self).__init__(data)

    # ------------------------------------------------------------------ RK step
    def _op(self, op, D, A, B, Cc, ca=0.0, cb=0.0, cc=0.0):
        _lib.check(_lib.lib().pcl_rk_op(self._h, op, D, A, B, Cc, ca, cb, cc))

    def step(self, solution):
        """Evolve q over one time step (sharpclaw.py:152-210).  Registers: q, s1, s2, dq on device."""
        state = solution.states[0]
        if isinstance(self.start_step, CellStartStep):
            self.start_step.apply(self, state)        # on the resident state, no round trip
        elif self.start_step is not start_step:
            self._pull(state)
            self.start_step(self, solution)
            self._push(state)
        else:
            self.start_step(self, solution)
        if self._user_rp is not None:
            self._user_rp.send_params(self)
        t, dt = state.t, self.dt
        # st(reg, t, op, D, A, B, ...): deltaq = dq(reg, t) followed by the combination that consumes it.
        # Without a Python dq_src (or with a DeviceDqSource the last pass evaluates) both run as ONE fused device stage
        # (pcl_sharp_stage); with one, deltaq has to visit the host and the combination is a separate register operation.
        st = self._stage_fused if (self.dq_src is None or self._dq_src_fused) else self._stage_split
        try:
            if self.time_integrator == 'Euler':
                st(Q, t, 1, Q, Q, Q, ca=1.0)                          # state.q += deltaq
            elif self.time_integrator == 'SSP33':
                st(Q, t, 1, S1, Q, Q, ca=1.0)                         # s.q = state.q + deltaq
                st(S1, t + dt, 2, S1, Q, S1, ca=0.75, cb=0.25)        # 0.75*q + 0.25*(s.q+deltaq)
                st(S1, t + 0.5 * dt, 2, Q, Q, S1, ca=1. / 3., cb=2. / 3.)   # 1/3*q + 2/3*(s.q+deltaq)
            elif self.time_integrator == 'SSP104':
                st(Q, t, 1, S1, Q, Q, ca=6.)                          # s1 = q + deltaq/6
                s1t = t + dt / 6.
                for i in range(4):
                    st(S1, s1t, 1, S1, S1, Q, ca=6.)
                    s1t = s1t + dt / 6.
                self._op(6, S1, Q, S1, S2, ca=25., cb=9. / 25, cc=15.)   # s2 = q/25 + 9/25*s1 ; s1 = 15*s2 - 5*s1
                s1t = t + dt / 3.
                for i in range(4):
                    st(S1, s1t, 1, S1, S1, Q, ca=6.)
                    s1t = s1t + dt / 6.
                st(S1, s1t, 5, Q, S2, S1, cb=0.6, cc=0.1)             # q = s2 + 0.6*s1 + 0.1*deltaq
            elif self._rk is not None:
                self._step_tableau(t, dt)
            else:
                raise Exception('Unrecognized time integrator')
            self._host_stale = True
        except CFLError:
            return False

    def _lincomb(self, D, A, coef):
        """D = A + sum_j coef[j]*K_j on the device, terms in ascending j; a coefficient of exactly 0.0 is no term."""
        js = [j for j in range(len(coef)) if coef[j] != 0.0]
        stages = np.array(js, dtype=np.int32)
        cs = np.array([coef[j] for j in js], dtype=np.float64)
        _lib.check(_lib.lib().pcl_rk_lincomb(self._h, D, A, len(js), _lib.i(stages), _lib.d(cs)))

    def _step_tableau(self, t, dt):
        """One step of the explicit Runge-Kutta scheme of ``self._rk = (a, b, c)`` (rk_tableaus.py):
        y_i = q + sum_j a_ij K_j in S1 (stage 0 reads q itself), K_i = dq(y_i, t + c_i dt) taken from the dq register
        by a pointer swap, q = q + sum_j b_j K_j.  q is written by the last combination only, so a CFLError of any
        stage leaves it as it was."""
        a, b, c = self._rk
        L = _lib.lib()
        for i in range(len(b)):
            reg = Q
            if i > 0:
                self._lincomb(S1, Q, a[i, :i])
                reg = S1
            self.dq(reg, t + c[i] * dt)
            _lib.check(L.pcl_rk_take(self._h, i))
        self._lincomb(Q, Q, b)

    def _stage_split(self, reg, t, op, D, A, B, ca=0.0, cb=0.0, cc=0.0):
        self.dq(reg, t)
        if op == 1:
            self._op(1, D, A, DQ, Q, ca=ca)                           # A + deltaq/ca
        else:
            self._op(op, D, A, B, DQ, ca=ca, cb=cb, cc=cc)

    def _stage_fused(self, reg, t, op, D, A, B, ca=0.0, cb=0.0, cc=0.0):
        """apply_q_bcs(stage) + flux1/flux2 + the RK combination on the device (sharpclaw.py:168-237)."""
        L = _lib.lib()
        stg = self._stage
        stg.t = t
        _lib.check(L.pcl_select(self._h, reg))
        try:
            cfl = ctypes.c_double(0.0)
            spec = self._device_bc_spec(self._state)
            if spec is not None:
                # every ghost fill runs on the device: exchange + BCs + both passes + the combination in one call
                _lib.check(L.pcl_sharp_bc_stage(self._h, spec[2], spec[3], self.dt, op, D, A, B, ca, cb, cc,
                                                float(self.cfl_max), ctypes.cast(ctypes.byref(cfl), _lib.dp)))
            else:
                self.apply_q_bcs(stg)
                _lib.check(L.pcl_sharp_stage(self._h, self.dt, op, D, A, B, ca, cb, cc, float(self.cfl_max),
                                             ctypes.cast(ctypes.byref(cfl), _lib.dp)))
        finally:
            _lib.check(L.pcl_select(self._h, Q))
        self.cfl.update_global_max(cfl.value)
        if self.cfl.get_cached_max() > self.cfl_max:
            raise CFLError('cfl_max exceeded')

    def set_mthlim(self):
        self.mthlim = self.limiters
        if not isinstance(self.limiters, list):
            self.mthlim = [self.mthlim]
        if len(self.mthlim) == 1:
            self.mthlim = self.mthlim * self.mwaves
        if len(self.mthlim) != self.mwaves:
            raise Exception('Length of solver.limiters is not equal to 1 or to solver.mwaves')

    def dq(self, reg, t):
        """Evaluate dq/dt * (delta t) of a register into the dq register (sharpclaw.py:221-237)."""
        self.dq_hyperbolic(reg, t)
        if self.cfl.get_cached_max() > self.cfl_max:
            raise CFLError('cfl_max exceeded')
        if isinstance(self.dq_src, CellDqSource):
            # deltaq += dq_src(stage) by a cell function on the resident registers
            L = _lib.lib()
            _lib.check(L.pcl_select(self._h, reg))
            try:
                self.dq_src.launch(self, t, self.dt)
            finally:
                _lib.check(L.pcl_select(self._h, Q))
        elif self.dq_src is not None and not self._dq_src_fused:
            # arbitrary Python: round trip of the stage through the host
            L = _lib.lib()
            st = self._stage
            st.t = t
            st.q = np.empty(self._state.q.shape, order='F')
            self._pull_aux(self._state)        # the stage shares the state's aux array (time-dependent aux)
            _lib.check(L.pcl_select(self._h, reg))
            _lib.check(L.pcl_get_q(self._h, _lib.d(st.q), 0))
            extra = _lib.fortran64(self.dq_src(self, st, self.dt))
            _lib.check(L.pcl_select(self._h, TMP))
            _lib.check(L.pcl_put_q(self._h, _lib.d(extra), 0))
            _lib.check(L.pcl_select(self._h, Q))
            self._op(1, DQ, DQ, TMP, Q, ca=1.0)                       # deltaq += dq_src(...)

    def dq_hyperbolic(self, reg, t):
        """apply_q_bcs(stage) + flux1/flux2 on the device (sharpclaw.py:343-385, 515-563)."""
        L = _lib.lib()
        st = self._stage
        st.t = t
        _lib.check(L.pcl_select(self._h, reg))
        try:
            cfl = ctypes.c_double(0.0)
            spec = self._device_bc_spec(self._state)
            if spec is not None:
                _lib.check(L.pcl_sharp_bc_dq(self._h, spec[2], spec[3], self.dt,
                                             ctypes.cast(ctypes.byref(cfl), _lib.dp)))
            else:
                self.apply_q_bcs(st)
                _lib.check(L.pcl_sharp_dq(self._h, self.dt, ctypes.cast(ctypes.byref(cfl), _lib.dp)))
        finally:
            _lib.check(L.pcl_select(self._h, Q))
        self.cfl.update_global_max(cfl.value)

    # a rejected SharpClaw step never wrote q (CFLError is raised before the final combination),
    # so no backup is needed unless a user start_step changed q
    def _backup(self, state):
        self._copied_backup = self.start_step is not start_step
        if self._copied_backup:
            _lib.check(_lib.lib().pcl_backup(self._h))

    def _restore(self, state):
        if self._copied_backup:
            _lib.check(_lib.lib().pcl_restore(self._h))
            self._host_stale = True

    # ------------------------------------------------------------------ setup
    def setup(self, solution):
        """Allocate RK registers and the device solver (sharpclaw.py:302-323, 474-495)."""
        if self.kernel_language not in ('HIP', 'Fortran'):
            raise Exception("Unrecognized value of solver.kernel_language.")
        if self.ndim == 3:
            self._check_3d(solution.states[0])
        if self.weno_order not in (5, 7, 9, 11, 13, 15, 17):
            # reconstruct.f90:112
            raise Exception("ERROR: weno_order must be an odd number between 5 and 17 (inclusive).")
        if self.weno_order != 5 and self.lim_type != 2:
            raise NotImplementedError("weno_order > 5 is a lim_type=2 (PyWENO) reconstruction")
        if self.lim_type not in (1, 2, 3):
            raise NotImplementedError("pyclaw_amd SharpClaw implements lim_type 1 (tvd2), 2 (WENO5) and 3 (legacy WENO5)")
        if self.tfluct_solver:
            raise NotImplementedError("pyclaw_amd SharpClaw implements tfluct_solver=False (the reference's tfluct.f90 is a stub)")
        if self.char_decomp not in (0, 1):
            raise NotImplementedError("char_decomp 2 / 3 need a user-supplied evec routine (the reference only stubs evec.f90)")
        if self.char_decomp == 1 and (self.ndim != 1 or self.lim_type not in (1, 2) or self.weno_order != 5 or self.fwave):
            # 1d/sharpclaw/flux1.f90:80-107; the 2-D flux1.f90 calls rpn2 with a wrong argument list on this path
            raise NotImplementedError("char_decomp=1 (wave-based reconstruction): 1-D solvers, lim_type 1 (tvd2_wave) or "
                                      "2 (weno5_wave), weno_order 5, no f-wave solver")
        self._rk = None
        if self.time_integrator == 'RK':
            self._rk = rk_tableaus.validate(getattr(self, 'a', None), getattr(self, 'b', None), getattr(self, 'c', None))
        elif self.time_integrator in rk_tableaus.TABLEAUS:
            tab = rk_tableaus.TABLEAUS[self.time_integrator]
            self._rk = rk_tableaus.validate(tab['a'], tab['b'], tab['c'])
        elif self.time_integrator not in ('Euler', 'SSP33', 'SSP104'):
            raise Exception('Unrecognized time integrator')
        self.mbc = (self.weno_order + 1) // 2
        state = solution.states[0]
        state.set_mbc(self.mbc)
        self.set_mthlim()
        if self.rp is None:
            raise Exception("solver.rp is not set: choose a Riemann solver from pyclaw_amd.riemann")
        rp = riemann.get(self.rp)
        user_rp = isinstance(rp, riemann.CellRiemann)
        if user_rp:
            self._check_user_rp(rp, state)
        self._check_cell_functions(state)
        if rp.ndim != self.ndim or rp.mwaves != self.mwaves or rp.meqn != state.meqn:
            raise Exception("Riemann solver %s does not match ndim/mwaves/meqn of the problem" % rp.name)
        params = rp.all_params(state)
        if user_rp:
            # the SharpClaw kernels of this one reconstruction around the body; raises with the compiler's log before any
            # device work
            rp.compile(self.math, sharp=(self.lim_type, self.weno_order) if self.ndim == 3 else
                       (self.lim_type, self.weno_order, self.char_decomp))

        self._release()
        cfg = _lib.Config()
        cfg.ndim = self.ndim
        for k in range(self.ndim):
            cfg.n[k] = int(state.grid.ng[k])
            cfg.d[k] = float(state.grid.d[k])
        cfg.mbc = self.mbc
        cfg.meqn = state.meqn
        cfg.mwaves = self.mwaves
        cfg.maux = state.maux
        cfg.method[1] = 2
        cfg.method[4] = int(self.char_decomp)          # clawparams.char_decomp (sharpclaw.py:262)
        cfg.method[5] = state.mcapa + 1
        cfg.method[6] = state.maux
        for k, m in enumerate(self.mthlim[:_lib.MAX_WAVES]):      # clawparams.mthlim (sharpclaw.py:268): tvd2 reads it
            cfg.mthlim[k] = int(m)
        cfg.fwave = int(bool(self.fwave))
        cfg.rp = rp.id
        for k, v in enumerate(params):
            cfg.rp_params[k] = v
        from . import parallel
        cfg.device = parallel.device_ordinal() if state.decomp is not None else int(getattr(self, 'device', 0))
        if self.math not in ('exact', 'fast', 'strict'):
            raise Exception("solver.math must be 'exact', 'fast' or 'strict'")
        cfg.math = {'exact': 0, 'fast': 1, 'strict': 2}[self.math]
        cfg.kind = 1
        cfg.lim_type = int(self.lim_type)
        h = ctypes.c_void_p()
        if user_rp:
            # the library checks the configuration against what the handle was compiled for and attaches it
            _lib.check(_lib.lib().pcl_create_cellrp(ctypes.byref(cfg), rp._rp, ctypes.byref(h)))
        else:
            _lib.check(_lib.lib().pcl_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self._user_rp, self._user_rp_sent = (rp, np.array(params)) if user_rp else (None, None)
        self._stage = _StageState(state)
        if self._rk is not None:
            # the stage derivatives K_0 .. K_{s-1}, each the size of q; the three hand-written schemes hold none
            _lib.check(_lib.lib().pcl_rk_stages(self._h, len(self._rk[1]), None))
        self._dq_src_fused = False
        if isinstance(self.dq_src, DeviceDqSource) and self.dq_src.fusable(self, state):
            _lib.check(_lib.lib().pcl_sharp_fuse_dq_src(self._h, self.dq_src.src_id, _lib.d(self.dq_src.params),
                                                        len(self.dq_src.params)))
            self._dq_src_fused = True
        self.allocate_bc_arrays(state)
        self._setup_halo(state)
        self._upload_aux(state)
        self._setup_cell_functions(state)

    def _check_user_rp(self, rp, state):
        """What a user-written Riemann solver (riemann.CellRiemann) asks of a SharpClaw solver, each refusal with its reason.
        (lim_type, weno_order, char_decomp and tfluct_solver were checked above, as for a built-in solver.)"""
        if isinstance(rp, riemann.SharpCellRiemann3D) and self.ndim != 3:
            raise NotImplementedError("SharpCellRiemann3D: this solver is compiled into the three passes of the 3-D SharpClaw "
                                      "kernel and serves SharpClawSolver3D alone; %s takes a CellRiemann(..., ndim=%d, "
                                      "sharpclaw=True)" % (type(self).__name__, self.ndim))
        if self.ndim == 3 and not isinstance(rp, riemann.SharpCellRiemann3D):
            raise NotImplementedError("SharpClawSolver3D takes a SharpCellRiemann3D, compiled into the three passes of the 3-D "
                                      "SharpClaw kernel; a %s is compiled into %s" % (type(rp).__name__,
                                      "the classic 3-D sweeps and serves ClawSolver3D" if rp.ndim == 3 else "the 1-D and 2-D kernels"))
        if not rp.sharpclaw:
            raise NotImplementedError("CellRiemann: the SharpClaw solvers are served by a solver written with sharpclaw=True "
                                      "(compiled into the SharpClaw kernels); without it a user-written Riemann solver is "
                                      "compiled into the classic sweep kernel only (ClawSolver1D / ClawSolver2D)")
        rp.check_solver(self, state)

    def _check_3d(self, state):
        """What SharpClaw in 3-D does not serve, each refusal with its reason, before anything is compiled."""
        from . import parallel
        if self.char_decomp != 0:
            raise NotImplementedError("SharpClawSolver3D: char_decomp = %r is not served in 3-D (char_decomp must be 0: the "
                                      "wave-based reconstruction is 1-D, and 2 / 3 need a user evec routine)" % (self.char_decomp,))
        if self.tfluct_solver:
            raise NotImplementedError("SharpClawSolver3D: tfluct_solver is not served (the reference's tfluct.f90 is a stub)")
        if self.fwave:
            raise NotImplementedError("SharpClawSolver3D: fwave = True is not served: the 3-D SharpClaw kernel has no f-wave form")
        if self.rp is not None and not isinstance(riemann.get(self.rp), riemann.CellRiemann):
            raise NotImplementedError("SharpClawSolver3D: no SharpClaw kernel of a built-in 3-D solver is instantiated; SharpClaw "
                                      "in 3-D runs solvers compiled at run time -- the library's own as "
                                      "SharpCellRiemann3D(problems.VC_ACOUSTICS_3D_RP, 4, 2, aux=(0, 1))")
        if state.decomp is not None and parallel.world_size() > 1:
            raise NotImplementedError("SharpClawSolver3D: a decomposed run (more than one rank) is not served: a user-written "
                                      "solver runs on one block")

    def _custom_bc(self, state, dim, idim, side, fn):
        # Python custom BCs on a stage: same strip protocol as the base class, `state` carries stage time
        super(SharpClawSolver, self)._custom_bc(state, dim, idim, side, fn)


class SharpClawSolver1D(SharpClawSolver):
    """SharpClaw solver for one-dimensional problems (sharpclaw.py:286-447)."""

    def __init__(self, data=None):
        self.ndim = 1
        super(SharpClawSolver1D, self).__init__(data)


class SharpClawSolver2D(SharpClawSolver):
    """SharpClaw evolution routine in 2D (sharpclaw.py:452-563)."""

    def __init__(self, data=None):
        self.ndim = 2
        super(SharpClawSolver2D, self).__init__(data)


class SharpClawSolver3D(SharpClawSolver):
    """SharpClaw evolution routine in 3D (upstream PyClaw's ``SharpClawSolver3D``; the reference has none).  Same attributes
    and defaults as the 2-D class; ``solver.rp`` is a ``riemann.SharpCellRiemann3D`` (see the module text).  ``cfl_max`` and
    ``cfl_desired`` keep the SharpClaw defaults 2.5 / 2.45 in 3-D too: nothing is changed silently."""

    def __init__(self, data=None):
        self.ndim = 3
        super(SharpClawSolver3D, self).__init__(data)
