"""
Riemann solver registry.

The reference picks the Riemann solver when the app's f2py module is linked
(``apps/*/Makefile``: ``$(RIEMANN)/src/rpn2_*.f``) and hands its scalars over through the
``cparam`` common block filled from ``state.aux_global`` (src/pyclaw/state.py:142-162).
Here a solver is named on the Solver object (``solver.rp = riemann.rp_euler_5wave_2d`` or
the string ``'euler_5wave_2d'``); ``cparam`` lists the aux_global keys in common-block order.
A solver of the user's own is a ``CellRiemann`` (1-D, 2-D) or a ``CellRiemann3D``: C++ text compiled at ``setup()``,
outside the table of built-in solvers.
"""
import numpy as np


class RiemannSolver(object):
    def __init__(self, name, rp_id, ndim, meqn, mwaves, cparam, has_transverse=False, grid_params=False):
        self.name = name
        self.grid_params = grid_params     # append the grid spacings (the reference app sets comxyt.dxcom/dycom)
        self.id = rp_id
        self.ndim = ndim
        self.meqn = meqn
        self.mwaves = mwaves
        self.cparam = tuple(cparam)
        self.has_transverse = has_transverse

    def params(self, aux_global):
        """cparam values from aux_global; same check as State.set_cparam (state.py:156-160)."""
        if not set(self.cparam) <= set(aux_global.keys()):
            raise Exception("""Some required value(s) in the cparam common 
                                   block in the Riemann solver have not been 
                                   set in aux_global.""")
        return [float(aux_global[k]) for k in self.cparam]

    def all_params(self, state):
        """cparam values, then dx, dy(, dz) for solvers that read common /comxyt/ (set by the reference app:
        apps/shallow-sphere/shallow_4_Rossby_Haurwitz_wave.py:449-451)."""
        p = self.params(state.aux_global)
        if self.grid_params:
            p = p + [float(d) for d in state.grid.d]
        return p

    def __repr__(self):
        return "<RiemannSolver %s>" % self.name


rp_advection_1d = RiemannSolver("advection_1d", 1, 1, 1, 1, ["u"])
rp_acoustics_1d = RiemannSolver("acoustics_1d", 2, 1, 2, 2, ["rho", "bulk", "cc", "zz"])
rp_advection_color_1d = RiemannSolver("advection_color_1d", 6, 1, 1, 1, [])        # aux(1) = velocity at the left edge
rp_burgers_1d = RiemannSolver("burgers_1d", 3, 1, 1, 1, [])
rp_euler_1d = RiemannSolver("euler_1d", 4, 1, 3, 3, ["gamma", "gamma1"])            # rp1_euler_with_efix
rp_shallow_1d = RiemannSolver("shallow_1d", 5, 1, 2, 2, ["g"])                       # rp1_shallow_roe_with_efix
# f-wave solvers (solver.fwave = True, the reference's classic1fw / classic2fw): aux(1)=rho, aux(2)=K, aux(3)=1 for the
# linear stress law, anything else for sigma = exp(K eps) - 1; the p-system's transverse solver reads aux(4) = eps
rp_elasticity_fwave_1d = RiemannSolver("elasticity_fwave_1d", 7, 1, 2, 2, [])
rp_psystem_fwave_2d = RiemannSolver("psystem_fwave_2d", 17, 2, 3, 2, [], True)
rp_advection_2d = RiemannSolver("advection_2d", 12, 2, 1, 1, ["u", "v"], True)
rp_shallow_2d = RiemannSolver("shallow_2d", 13, 2, 3, 3, ["g"], True)             # rpn2/rpt2_shallow_roe_with_efix
rp_vc_acoustics_2d = RiemannSolver("vc_acoustics_2d", 14, 2, 3, 2, [], True)     # aux(1)=Z, aux(2)=c
rp_vc_advection_2d = RiemannSolver("vc_advection_2d", 15, 2, 1, 1, [], True)     # aux(1)=u at left edge, aux(2)=v at bottom edge
rp_acoustics_2d = RiemannSolver("acoustics_2d", 10, 2, 3, 2, ["rho", "bulk", "cc", "zz"], True)
rp_euler_5wave_2d = RiemannSolver("euler_5wave_2d", 11, 2, 5, 5, ["gamma", "gamma1"], True)
# rpn2/rpt2_shallow_sphere (apps/shallow-sphere/Makefile:7): common /sw/ g; the 16 aux components of setaux.f; the
# unsplit step is the app's step2qcor.f
rp_shallow_sphere_2d = RiemannSolver("shallow_sphere_2d", 16, 2, 4, 3, ["g"], True, grid_params=True)

# 3-D acoustics, impedance and sound speed per cell in aux(1), aux(2) (test/acoustics/3d/Makefile:
# rpn3_vc_acoustics.f; dimension-split, and unsplit with rpt3/rptt3_vc_acoustics.f where there is no capacity function)
rp_vc_acoustics_3d = RiemannSolver("vc_acoustics_3d", 20, 3, 4, 2, [])

_ALL = [rp_elasticity_fwave_1d, rp_psystem_fwave_2d, rp_advection_1d, rp_acoustics_1d, rp_advection_color_1d, rp_burgers_1d, rp_euler_1d, rp_shallow_1d, rp_advection_2d, rp_shallow_2d, rp_vc_acoustics_2d, rp_vc_advection_2d, rp_acoustics_2d, rp_euler_5wave_2d, rp_shallow_sphere_2d, rp_vc_acoustics_3d]
BY_NAME = dict((r.name, r) for r in _ALL)


PCL_RP_CELL = 100      # include/pyclaw_amd.h: not a built-in id, outside _ALL


class CellRiemann(RiemannSolver):
    """A user-written NORMAL Riemann solver (Clawpack's rp1 / rpn2, one interface at a time) as the text of a C++
    function body: ``solver.rp = CellRiemann(body, meqn, mwaves, ndim, params)`` on ``ClawSolver1D`` / ``ClawSolver2D``.
    It is compiled at ``setup()`` into the library's own sweep kernel and runs in the classic 1-D step and in the two
    passes of the dimension-split 2-D step with the tiles, limiter and Courant reduction of the built-in solvers; with
    ``sharpclaw=True`` (below) into the SharpClaw kernels instead.

    The body sees ``ql[MEQN]``, ``qr[MEQN]`` (the cells left and right of the interface), ``p[8]`` (``params``;
    reassigning them between steps compiles nothing), the compile-time constant ``ixy`` (1 = x, always in 1-D; 2 = y)
    and assigns ``wave[MWAVES][MEQN]``, ``s[MWAVES]``, ``amdq[MEQN]``, ``apdq[MEQN]``, all zero on entry.  The helpers
    of the built-in solvers (``dmax``, ``dmin``, ``dsqrt``, ``fdiv``, ``Recip``) are in scope; ``preamble`` holds helper
    functions.  For bitwise-equal ``ql`` and ``qr`` the waves and fluctuations must be zero (the wave form's contract;
    an f-wave body, below, is not held to it).

    A solver with cell-wise coefficients names the components of ``state.aux`` its body reads: ``aux=(0, 1)``
    (0-based).  The sweep stages those planes next to q in its tile, and the body also sees ``auxl[NAUX]`` and
    ``auxr[NAUX]``, the listed components in list order of the cell left and of the cell right of the interface
    (Clawpack's "aux(1) is the value at the left edge of cell i" is ``auxr[0]``).  One list serves both sweeps; a body
    that reads another component per direction branches on ``ixy``.  With aux the contract reads: for bitwise-equal
    ``ql`` and ``qr`` the waves and fluctuations are zero *whatever aux holds* -- a wavefront without a jump in q takes
    the speeds alone, each interface with its own ``auxl`` / ``auxr``.  A flux-difference form over varying coefficients
    breaks this; that is an f-wave solver: ``fwave=True``, below.  The tile holds ``meqn + len(aux)`` planes in a
    workgroup's 64 KB, which comes to at most 8 (``MAX_PLANES``; the library derives it from its tile shapes and
    refuses with its own figure).  ``setup()`` needs ``state.aux`` with ``maux > max(aux)``; aux upload, aux ghost
    cells and aux boundary conditions then run as for a built-in solver with aux, and a ``CellStartStep`` with
    ``writes_aux=True`` is seen by the body in the same step.

    ``transverse`` (2-D only) is a second text, the inside of Clawpack's ``rpt2`` for one interface, and opens
    ``ClawSolver2D(dim_split=False)`` with ``order_trans`` 0, 1 and 2 to the solver: the library then also compiles its
    unsplit x and y kernels around the two bodies.  Without ``aux`` it sees ``ql[MEQN]``, ``qr[MEQN]`` (the cells left
    and right of the interface whose fluctuation is split; the same pair for A-dq and A+dq, there is no ``imp``),
    ``asdq[MEQN]``, ``p[8]`` and ``ixy`` (the direction of the *normal* solve; the split is across it) and assigns
    ``bmasdq[MEQN]``, ``bpasdq[MEQN]``, zero on entry.  With ``aux`` it sees instead of the two cells ``q1[MEQN]``,
    ``aux1[NAUX]`` (the cell the fluctuation belongs to: left of the interface for A-dq, right of it for A+dq) and
    ``aux_below[NAUX]``, ``aux_above[NAUX]`` (the listed components of its neighbours at the lower and upper transverse
    index, Clawpack's aux1 / aux3 rows).  For ``asdq`` all zero the results must be zero: a wavefront without a jump
    never calls the body.  Its diagnostics read ``transverse:<n>``.  The dimension-split step of a solver that carries
    a transverse body is unchanged.

    ``fwave=True`` is an f-wave solver (``solver.fwave = True``; Clawpack's classic1fw / classic2fw): the array the body
    assigns is named ``fwave[MWAVES][MEQN]`` in place of ``wave``, as in Clawpack's f-wave solvers, and holds the pieces
    of the flux difference; ``s``, ``amdq``, ``apdq`` and everything the body reads are unchanged, all results zero on
    entry, and the transverse body's interface is the same in either form.  The "equal q, zero waves" contract does
    *not* apply to an f-wave body: every interface is solved, no wavefront is skipped, so the f-waves between two equal
    cells over different coefficients (well-balanced shallow water over bathymetry, conservative variable-coefficient
    advection, layered elasticity) are what the body says they are.  ``capa=True`` compiles the sweeps with a capacity
    function, ``state.mcapa`` (any component; it is a run-time value): the body does not change, the sweeps divide
    dt/dx by it per cell.  The tile then holds one more plane: ``meqn + 1 + len(aux) <= MAX_PLANES``.  Both are part
    of the compile key and readable as attributes; the solver and the state must say the same as the ``CellRiemann``
    (``setup()`` refuses each mismatch with its reason).

    ``sharpclaw=True`` compiles the solver for ``SharpClawSolver1D`` / ``SharpClawSolver2D`` and for nothing else (a
    classic solver refuses it; together with ``transverse`` it is a ``ValueError``).  ``setup()`` compiles the library's
    SharpClaw kernels around the body for the solver's own ``lim_type``, ``weno_order`` and ``char_decomp``, which are
    part of the compile key: ``lim_type`` 1, 2, 3 at ``weno_order`` 5 and ``weno_order`` 7..17 with ``lim_type`` 2 for
    any system, the built-in solvers that lack those orders included once they are restated as bodies; ``char_decomp =
    1`` as for the built-in solvers (1-D, ``lim_type`` 1 or 2, order 5, wave form).  The body, ``preamble``, ``params``,
    ``aux``, ``fwave`` and ``capa`` mean what they mean above (an f-wave body assigns ``fwave``; SharpClaw reads ``s``,
    ``amdq`` and ``apdq`` alone).  The "equal q, zero waves" contract is not relied on here: SharpClaw solves every
    interface and the problem inside every cell, both edge states of a cell with the cell's own aux values.  Euler,
    SSP33 and SSP104 run with the fused stage calls of the built-in solvers.  The tile holds ``meqn + capa`` planes in
    the x pass and ``meqn + capa + len(aux)`` in the 2-D y pass, at most ``MAX_PLANES`` each (the y planes are half as
    large from six aux components on, so the x pass then sets the limit).  A ``dq_src`` -- a ``CellDqSource`` or a
    Python callable -- runs as its own pass: nothing is fused into the stage.

    ``one_kernel=True`` (2-D, classic) also compiles the library's one-kernel form of the dimension-split 2-D step
    around the body: both sweeps on one tile in LDS, q through memory once per step.  ``ClawSolver2D(dim_split=True)``
    then chooses between that step and the two passes exactly as it does for a built-in solver, and
    ``solver.status["step_forms"]`` reports what ran.  A wave-form body without ``aux`` and ``capa`` gets everything the
    built-in solvers get there -- tiles whose update is the identity are skipped, only the tiles that compute are
    launched, timed trials pick the faster form, and resident mode enqueues the next step ahead -- all of which rest on
    the contract above ("bitwise-equal ``ql`` and ``qr`` give zero waves") and on nothing else.  A body with ``aux`` or
    ``capa=True`` runs the one-kernel step over the whole block; an f-wave body its f-wave form, in which every interface
    is solved.  It is a ``ValueError`` with ``ndim != 2``, with ``sharpclaw=True`` and with ``meqn > 5`` (the tile of the
    one-kernel step holds up to five equations, for every solver).  It is part of the compile key and readable as an
    attribute; the default is ``False``, which compiles what it always did.  A solver that carries a transverse body and
    runs ``dim_split=False`` keeps its unsplit kernels and never uses the extra one.

    The dimension-split 3-D step takes a ``CellRiemann3D`` (below); ``CellRiemann(..., ndim=3)`` is a ``ValueError``.

    Not served: a transverse body that needs both cells and aux, a conservation fix in the unsplit step (the sphere
    solver's ``qcor``), f-waves in 3-D, the unsplit 3-D step with a capacity function, ``mbc > 2`` in 3-D, more than one
    block (decomposed runs); under SharpClaw ``char_decomp`` 2 / 3, ``tfluct_solver`` and a fused dq source.  The unsplit y
    phase always runs in its tile form (the marching y kernel stays with the built-in solvers)."""

    MAX_PARAMS = 8
    MAX_PLANES = 8
    ONE_KERNEL_MAX_MEQN = 5
    _NDIMS = (1, 2)
    rpt3 = None             # the 3-D transverse bodies: a CellRiemann3D's alone
    rptt3 = None

    def __init__(self, body, meqn, mwaves, ndim, params=(), preamble="", name="user", aux=(), transverse=None, fwave=False,
                 capa=False, sharpclaw=False, one_kernel=False):
        RiemannSolver.__init__(self, name, PCL_RP_CELL, int(ndim), int(meqn), int(mwaves), (),
                               has_transverse=transverse is not None)
        if not 1 <= self.meqn <= 8 or not 1 <= self.mwaves <= 8:
            raise ValueError("CellRiemann: 1 <= meqn <= 8 and 1 <= mwaves <= 8, got meqn=%d mwaves=%d" % (self.meqn, self.mwaves))
        if self.ndim not in self._NDIMS:
            raise ValueError("CellRiemann: ndim must be 1 or 2 (the classic 1-D and dimension-split 2-D sweeps), got %d; the "
                             "dimension-split 3-D sweeps take a CellRiemann3D" % self.ndim)
        self.sharpclaw = bool(sharpclaw)
        if self.sharpclaw and transverse is not None:
            raise ValueError("CellRiemann: sharpclaw=True with a transverse body: SharpClaw has no transverse solve, and a "
                             "solver compiled for it serves SharpClawSolver1D / SharpClawSolver2D alone")
        self.one_kernel = bool(one_kernel)
        self._check_one_kernel()
        self.aux = tuple(int(k) for k in aux)
        if any(k < 0 for k in self.aux):
            raise ValueError("CellRiemann: aux lists 0-based components of state.aux, got a negative index in %r" % (self.aux,))
        if len(set(self.aux)) != len(self.aux):
            raise ValueError("CellRiemann: aux lists a component twice: %r" % (self.aux,))
        self.fwave = bool(fwave)
        self.capa = bool(capa)
        if self.sharpclaw:
            # the SharpClaw tiles (the library has the rule and refuses with its own figures): q and the capacity function in
            # the x pass, the listed aux components too in the y pass, whose planes are half as large from six components on
            planes = self.meqn + int(self.capa) + (len(self.aux) if self.ndim == 2 and len(self.aux) < 6 else 0)
            if planes > self.MAX_PLANES:
                raise ValueError("CellRiemann: meqn + capa + len(aux) = %d with sharpclaw=True, the SharpClaw tile holds at most "
                                 "%d planes (q components, the capacity function and, in the 2-D y pass, listed aux components)"
                                 % (planes, self.MAX_PLANES))
        elif self.aux and self.meqn + len(self.aux) > self.MAX_PLANES:
            raise ValueError("CellRiemann: meqn + len(aux) = %d, the sweep's tile holds at most %d planes (q components and "
                             "listed aux components)" % (self.meqn + len(self.aux), self.MAX_PLANES))
        if not self.sharpclaw and self.capa and self.meqn + 1 + len(self.aux) > self.MAX_PLANES:
            raise ValueError("CellRiemann: meqn + 1 + len(aux) = %d with capa=True, the sweep's tile holds at most %d planes "
                             "(q components, the capacity function and listed aux components)"
                             % (self.meqn + 1 + len(self.aux), self.MAX_PLANES))
        if transverse is not None and self.ndim != 2:
            raise ValueError("CellRiemann: a transverse body belongs to the unsplit 2-D step, got ndim=%d" % self.ndim)
        self.body = str(body)
        self.transverse = None if transverse is None else str(transverse)
        self.preamble = str(preamble)
        self.params = params
        self._rp = None            # pcl_cellrp handle and what it was compiled for
        self._key = None
        self.code_size = 0

    def _check_one_kernel(self):
        """What one_kernel=True cannot go with, each with its reason: at construction, and again in compile(), since the
        attribute can be assigned afterwards."""
        if not self.one_kernel:
            return
        if self.ndim != 2:
            raise ValueError("CellRiemann: one_kernel=True with ndim=%d: the one-kernel step is the dimension-split 2-D "
                             "step (ndim must be 2)" % self.ndim)
        if self.sharpclaw:
            raise ValueError("CellRiemann: one_kernel=True with sharpclaw=True: the one-kernel step is a classic step, "
                             "and a solver compiled for SharpClaw holds the SharpClaw kernels alone")
        if self.meqn > self.ONE_KERNEL_MAX_MEQN:
            raise ValueError("CellRiemann: one_kernel=True with meqn=%d: the tile of the one-kernel step holds up to %d "
                             "equations (meqn > %d)" % (self.meqn, self.ONE_KERNEL_MAX_MEQN, self.ONE_KERNEL_MAX_MEQN))

    @property
    def params(self):
        return self._params

    @params.setter
    def params(self, values):
        values = np.array(values, dtype=np.float64).reshape(-1)
        if len(values) > self.MAX_PARAMS:
            raise ValueError("a Riemann solver body takes at most %d parameters, got %d" % (self.MAX_PARAMS, len(values)))
        self._params = values

    def all_params(self, state):
        return [float(v) for v in self._params]

    def compile(self, math='exact', sharp=None):
        """Compile (no device needed; cached per process).  Raises with the compiler's log, whose line numbers are the
        body's ("riemann:<n>"), the transverse body's ("transverse:<n>") or the preamble's ("preamble:<n>").
        ``sharp=(lim_type, weno_order, char_decomp)``, for a solver written with ``sharpclaw=True`` and only for one:
        the SharpClaw kernels of that one reconstruction; the three are part of the key."""
        import ctypes
        from . import _lib
        if math not in ('exact', 'fast', 'strict'):
            raise Exception("math must be 'exact', 'fast' or 'strict'")
        if (sharp is not None) != self.sharpclaw:
            raise ValueError("CellRiemann: compile(sharp=(lim_type, weno_order, char_decomp)) belongs to a solver written with "
                             "sharpclaw=True, and such a solver is compiled in no other way")
        self._check_one_kernel()
        sharp = None if sharp is None else tuple(int(v) for v in sharp)
        form = (1 if self.fwave else 0) | (2 if self.capa else 0)      # PCL_CELLRP_FORM_FWAVE, PCL_CELLRP_FORM_CAPA
        key = (self.meqn, self.mwaves, self.ndim, math, self.body, self.preamble, self.aux, self.transverse, form, sharp,
               bool(self.one_kernel), self.rpt3, self.rptt3)
        if self._rp is not None and self._key == key:
            return self
        rp, size = ctypes.c_void_p(), ctypes.c_long(0)
        mode = {'exact': 0, 'fast': 1, 'strict': 2}[math]
        aux = (ctypes.c_int * len(self.aux))(*self.aux) if self.aux else None
        if self.ndim == 3 and sharp is not None:        # a SharpCellRiemann3D: (lim_type, weno_order), char_decomp 0
            _lib.check(_lib.lib().pcl_cellrp_compile3_sharp(self.body.encode(), self.preamble.encode(), self.meqn, self.mwaves,
                                                            mode, aux, len(self.aux), form, sharp[0], sharp[1], ctypes.byref(rp)))
        elif self.ndim == 3 and self.rpt3 is not None:
            _lib.check(_lib.lib().pcl_cellrp_compile3t(self.body.encode(), self.rpt3.encode(),
                                                       None if self.rptt3 is None else self.rptt3.encode(),
                                                       self.preamble.encode(), self.meqn, self.mwaves, mode,
                                                       aux, len(self.aux), form, ctypes.byref(rp), ctypes.byref(size)))
        elif self.ndim == 3:
            _lib.check(_lib.lib().pcl_cellrp_compile3(self.body.encode(), self.preamble.encode(), self.meqn, self.mwaves, mode,
                                                      aux, len(self.aux), form, ctypes.byref(rp), ctypes.byref(size)))
        elif sharp is not None:
            _lib.check(_lib.lib().pcl_cellrp_compile_sharp(self.body.encode(), self.preamble.encode(), self.meqn, self.mwaves,
                                                           self.ndim, mode, aux, len(self.aux), form, sharp[0], sharp[1], sharp[2],
                                                           ctypes.byref(rp), ctypes.byref(size)))
        elif self.one_kernel:           # (2-D, classic, meqn <= 5: _check_one_kernel)
            _lib.check(_lib.lib().pcl_cellrp_compile_onek(self.body.encode(),
                                                          None if self.transverse is None else self.transverse.encode(),
                                                          self.preamble.encode(), self.meqn, self.mwaves, mode,
                                                          aux, len(self.aux), form, ctypes.byref(rp), ctypes.byref(size)))
        else:
            _lib.check(_lib.lib().pcl_cellrp_compile_form(self.body.encode(),
                                                          None if self.transverse is None else self.transverse.encode(),
                                                          self.preamble.encode(), self.meqn, self.mwaves, self.ndim, mode,
                                                          aux, len(self.aux), form, ctypes.byref(rp), ctypes.byref(size)))
        self.release()
        self._rp, self._key, self.code_size = rp, key, int(size.value)
        return self

    def check_solver(self, solver, state):
        """What the classic and the SharpClaw solvers alike refuse of a user-written solver, each with its reason: the
        form (compiled into the kernels, so the solver and the state must say the same), more than one rank, the aux list."""
        from . import parallel
        passes, into, unit = ("stages", "", "stage") if self.sharpclaw else ("sweeps", " into the sweep", "step")
        if solver.fwave and not self.fwave:
            raise NotImplementedError("CellRiemann: fwave = True is not served by this solver: its body returns waves; an "
                                      "f-wave body is compiled with CellRiemann(..., fwave=True)")
        if self.fwave and not solver.fwave:
            raise ValueError("CellRiemann: the solver was written with fwave=True (its body assigns f-waves) and "
                             "solver.fwave is False: set solver.fwave = True")
        if state.mcapa >= 0 and not self.capa:
            raise NotImplementedError("CellRiemann: state.mcapa (a capacity function) is not served by this solver: it is "
                                      "compiled%s without one (CellRiemann(..., capa=True) compiles it with one)" % into)
        if self.capa and state.mcapa < 0:
            raise ValueError("CellRiemann: the solver was written with capa=True (%s with a capacity function) and "
                             "state.mcapa is not set: name the aux component in state.mcapa" % passes)
        if state.decomp is not None and parallel.world_size() > 1:
            raise NotImplementedError("CellRiemann: more than one rank is not served: a user-written solver runs on one "
                                      "block (the decomposed %s's plans know the built-in solvers only)" % unit)
        if self.aux:
            # (an index past maux would be a read outside the aux allocation: the library refuses it again at attach)
            if state.aux is None:
                raise ValueError("CellRiemann: the body reads aux components %r and state.aux is None" % (self.aux,))
            if max(self.aux) >= state.maux:
                raise ValueError("CellRiemann: the body reads aux component %d (0-based) and state.maux = %d"
                                 % (max(self.aux), state.maux))

    def send_params(self, solver):
        """params reassigned since the solver's last step: they travel by value with its next kernels, no compile."""
        from . import _lib
        p = self._params
        if len(p) != len(solver._user_rp_sent) or not np.array_equal(p, solver._user_rp_sent):
            _lib.check(_lib.lib().pcl_cellrp_params(solver._h, _lib.d(p) if len(p) else None, len(p)))
            solver._user_rp_sent = p.copy()

    def release(self):
        if self._rp is not None:
            from . import _lib
            _lib.lib().pcl_cellrp_release(self._rp)
            self._rp = None
            self._key = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class CellRiemann3D(CellRiemann):
    """A user-written Riemann solver for ``ClawSolver3D``: ``solver.rp = CellRiemann3D(body, meqn, mwaves, params)``.  The body
    is Clawpack's rpn3 for one interface, written as for a ``CellRiemann``: it sees ``ql``, ``qr``, ``p[8]``, with
    ``aux=(...)`` also ``auxl`` / ``auxr``, and the compile-time constant ``ixy``, here 1, 2 or 3; it assigns ``wave``,
    ``s``, ``amdq``, ``apdq``, zero on entry, and for bitwise-equal ``ql`` and ``qr`` the waves and fluctuations must be
    zero whatever aux holds.  ``setup()`` compiles the x, y and z passes of the library's 3-D sweep kernel around it
    (``dim_split=True``).  ``capa=True`` compiles the passes with a capacity function (``state.mcapa``).  ``params`` can be
    reassigned between steps without a compile.

    ``rpt3=text`` and ``rptt3=text`` are the insides of Clawpack's ``rpt3`` and ``rptt3`` for one interface and give the
    solver the unsplit step, ``ClawSolver3D(dim_split=False)``: the library compiles the pieces kernel of its general
    unsplit 3-D step around the three texts, for every ``order_trans`` of the reference (0, 10, 11, 20, 21, 22); with
    ``rpt3`` alone for 0, 10 and 20, and ``setup()`` refuses the others with the reason.  Both texts see the compile-time
    constants ``ixyz`` (alias ``ixy``: the direction of the normal solve, 1..3) and ``icoor`` (2: the split is in the y-like
    direction ``ixyz+1``, 3: in the z-like direction ``ixyz+2``, cyclic), and ``p[8]``.  Without an aux list they see
    ``ql[MEQN]``, ``qr[MEQN]``, the cells left and right of the interface (the same pair for A-dq, A+dq and the
    correction wave: there is no ``imp``); with one they see ``imp`` (1, 2), ``q1[MEQN]``, the cell ``i-2+imp`` the
    fluctuation belongs to, and ``auxb[3][3][NAUX]``, ``auxb[a][b][k]`` being the k-th listed component of that cell's
    neighbour at y-like offset ``a-1`` and z-like offset ``b-1``.  ``rpt3`` reads ``asdq[MEQN]`` and assigns
    ``bmasdq[MEQN]``, ``bpasdq[MEQN]``; ``rptt3`` also sees ``impt`` (1: its input came out of a split that went down
    in the other transverse direction, 2: up), reads ``bsasdq[MEQN]`` and assigns ``cmbsasdq[MEQN]``,
    ``cpbsasdq[MEQN]`` -- the new split lies inside the neighbouring row the input went to.  Outputs are zero on entry,
    and for an all-zero input they must stay zero.  Diagnostics carry ``rpt3:<n>`` and ``rptt3:<n>``.  ``rptt3``
    without ``rpt3`` and ``capa=True`` with ``rpt3`` are a ``ValueError``.  The unsplit step holds 14 * meqn doubles of
    scratch per cell (ghost cells included) on the device, released by ``teardown()``.

    The three dimension-split passes stage q, the listed aux components and the capacity function in one tile:
    ``meqn + len(aux) + capa <= MAX_PLANES`` (7; the library derives it from its tile shapes and refuses with its own
    figure).  A solver with ``rpt3`` may exceed it and then serves ``dim_split=False`` alone.

    Not served in 3-D, so there is no keyword for them: f-waves and SharpClaw (``SharpClawSolver3D`` takes a
    ``SharpCellRiemann3D``, a class of its own, below).  Nor: the unsplit step with a capacity
    function, a transverse body with both cells and aux, ``mbc`` other than 2, more than one block."""

    MAX_PLANES = 7
    _NDIMS = (3,)

    def __init__(self, body, meqn, mwaves, params=(), preamble="", name="user", aux=(), capa=False, rpt3=None, rptt3=None):
        aux = tuple(aux)
        if rptt3 is not None and rpt3 is None:
            raise ValueError("CellRiemann3D: rptt3 without rpt3: the double-transverse solver splits what the transverse "
                             "solver returned")
        if rpt3 is not None and capa:
            raise ValueError("CellRiemann3D: capa=True with rpt3: the unsplit 3-D step (step3) with a capacity function is "
                             "not built for any solver")
        planes = int(meqn) + len(aux) + int(bool(capa))
        if planes > self.MAX_PLANES:
            if rpt3 is None:
                raise ValueError("CellRiemann3D: meqn + len(aux) + capa = %d, the tile of the 3-D sweeps holds at most %d planes "
                                 "(q components, listed aux components and the capacity function)" % (planes, self.MAX_PLANES))
            self.MAX_PLANES = 16        # the unsplit step alone: its kernels have no tile
        CellRiemann.__init__(self, body, meqn, mwaves, 3, params=params, preamble=preamble, name=name, aux=aux, capa=capa)
        self.rpt3 = None if rpt3 is None else str(rpt3)
        self.rptt3 = None if rptt3 is None else str(rptt3)
        self.has_transverse = self.rpt3 is not None


class SharpCellRiemann3D(CellRiemann):
    """A user-written Riemann solver for ``SharpClawSolver3D``:
    ``solver.rp = SharpCellRiemann3D(body, meqn, mwaves, params=(), aux=(), capa=False, preamble="", name=None)``.  The body is
    Clawpack's rpn3 for one interface under the contract of a ``CellRiemann3D``: it sees ``ql``, ``qr``, ``p[8]``, with
    ``aux=(...)`` also ``auxl`` / ``auxr``, and the compile-time constant ``ixy``, 1, 2 or 3, and assigns ``wave``, ``s``,
    ``amdq``, ``apdq``, zero on entry (SharpClaw reads ``s``, ``amdq`` and ``apdq`` alone, solves every interface and the
    problem inside every cell, both edge states of a cell with the cell's own aux values).  ``setup()`` compiles the x, y and
    z passes of the library's 3-D SharpClaw kernel around it for the solver's own ``lim_type`` and ``weno_order``
    (``compile(math, sharp=(lim_type, weno_order))``; both are part of the key): ``lim_type`` 1, 2, 3 at order 5 and orders
    7..17 with ``lim_type`` 2, for any system.  It is the only way SharpClaw runs in 3-D -- the library's own 3-D solver runs
    as ``apps.problems.VC_ACOUSTICS_3D_RP`` with ``aux=(0, 1)``.  ``capa=True`` compiles the passes with a capacity function
    (``state.mcapa``).  The tile of a pass holds ``meqn + capa + len(aux) <= MAX_PLANES`` (8) planes.  ``params`` can be
    reassigned between steps without a compile.  ``code_size`` is not reported for this class.

    Not served, so there is no keyword for them: f-waves, ``char_decomp``, transverse bodies.  Nor: ``tfluct_solver``, a fused
    dq source (a ``dq_src`` runs as its own pass), more than one block.  It serves ``SharpClawSolver3D`` and nothing else."""

    MAX_PLANES = 8
    _NDIMS = (3,)

    def __init__(self, body, meqn, mwaves, params=(), aux=(), capa=False, preamble="", name=None):
        aux = tuple(aux)
        planes = int(meqn) + int(bool(capa)) + len(aux)
        if planes > self.MAX_PLANES:
            raise ValueError("SharpCellRiemann3D: meqn + capa + len(aux) = %d, the tile of the 3-D SharpClaw passes holds at most "
                             "%d planes (q components, the capacity function and listed aux components)"
                             % (planes, self.MAX_PLANES))
        CellRiemann.__init__(self, body, meqn, mwaves, 3, params=params, preamble=preamble,
                             name="user" if name is None else name, aux=(), capa=capa, sharpclaw=True)
        # (the list goes in behind the 1-D / 2-D plane rule of the base class: this class has its own, above)
        self.aux = tuple(int(k) for k in aux)
        if any(k < 0 for k in self.aux):
            raise ValueError("SharpCellRiemann3D: aux lists 0-based components of state.aux, got a negative index in %r" % (self.aux,))
        if len(set(self.aux)) != len(self.aux):
            raise ValueError("SharpCellRiemann3D: aux lists a component twice: %r" % (self.aux,))

    def compile(self, math='exact', sharp=None):
        """``sharp=(lim_type, weno_order)``; a third entry, ``char_decomp``, must be 0."""
        if sharp is not None:
            sharp = tuple(int(v) for v in sharp)
            if len(sharp) not in (2, 3) or (len(sharp) == 3 and sharp[2] != 0):
                raise NotImplementedError("SharpCellRiemann3D: compile(sharp=(lim_type, weno_order)): char_decomp must be 0 in 3-D, "
                                          "got %r" % (sharp,))
            sharp = sharp[:2]
        return CellRiemann.compile(self, math, sharp=sharp)


def get(rp):
    if isinstance(rp, RiemannSolver):
        return rp
    if isinstance(rp, str):
        key = rp[3:] if rp.startswith("rp_") else rp
        if key in BY_NAME:
            return BY_NAME[key]
    raise Exception("Unknown Riemann solver %r; available: %s" % (rp, sorted(BY_NAME)))
