r"""
Solver base class: the plugin surface of the reference (src/pyclaw/solver.py).

``evolve_to_time`` / ``step`` / ``setup`` / ``teardown`` keep the reference's semantics
(adaptive dt with CFL accept/reject and retake, solver.py:602-717; status dict; error
messages).  What differs is where the state lives: between the first and last line of
``evolve_to_time`` the authoritative ``q`` is the solver's resident copy in HBM; ``state.q`` on
the host is refreshed when control returns to the caller (and around user callbacks that
are plain Python).  The reference's ``q_backup = state.q.copy('F')`` (solver.py:660) becomes
a pointer swap on the device (``pcl_undo_step``) -- no copy at all in the common case.
"""
import logging

import numpy as np

from . import _lib, parallel
from .cfl import CFL


def default_compute_gauge_values(q, aux):
    r"""By default, record values of q at gauges (solver.py:26-29)."""
    return q


class BC():
    """Boundary condition types (solver.py:17-23)."""
    custom = 0
    outflow = 1
    periodic = 2
    reflecting = 3


class DeviceBC(object):
    """A user boundary condition that libpyclaw_amd applies on the device.

    Assign an instance to ``solver.user_bc_lower`` / ``user_bc_upper`` (with the matching
    ``bc_lower[idim] = BC.custom``) instead of a Python function to avoid moving ghost cells
    through the host every step.
    """

    def apply(self, solver, idim, side):
        raise NotImplementedError


class ConstantStateBC(DeviceBC):
    """Ghost cells of one side := a fixed state vector (e.g. the post-shock inflow state of
    test/euler/2d/shockbubble.py:41-57).  ``dims`` restricts it to some dimensions."""

    def __init__(self, state, dims=None):
        self.state = np.ascontiguousarray(state, dtype=np.float64)
        self.dims = dims

    def apply(self, solver, idim, side):
        if self.dims is not None and idim not in self.dims:
            return
        _lib.check(_lib.lib().pcl_bc_const(solver._h, idim, side, _lib.d(self.state)))


class SphereMirrorBC(DeviceBC):
    """The custom y boundary of the shallow-water-on-the-sphere app (``qbc_lower_y`` / ``qbc_upper_y``,
    apps/shallow-sphere/shallow_4_Rossby_Haurwitz_wave.py:295-313): ghost row j takes interior row 2*mbc-1-j with
    the x index reversed over the whole ghosted width, on the device."""

    def apply(self, solver, idim, side):
        if idim != 1:
            raise Exception("SphereMirrorBC is the y boundary of a 2-D grid")
        dec = getattr(solver, '_state', None) and solver._state.decomp
        if dec is not None and dec.dims[0] != 1:
            raise Exception("SphereMirrorBC reverses whole rows: decompose the grid in y only (PCL_PROC_GRID=1xN)")
        _lib.check(_lib.lib().pcl_bc(solver._h, idim, side, 4))


class CellFunction(object):
    """Per-cell arithmetic written by the user as the text of a C++ function body, compiled at ``setup()`` for the
    library's architecture and run on the resident arrays as one pointwise pass over the interior cells: what a Python
    ``step_src`` / ``dq_src`` / ``start_step`` does with numpy on the host, without the device->host->device round trip.

    The body sees ``q[MEQN]``, ``aux[MAUX]`` (const), ``c.t``, ``c.dt``, the GLOBAL 0-based interior indices
    ``c.i[NDIM]``, the cell centre ``c.x[NDIM]`` (``lower + (i + 0.5) * d``, as ``grid.x.center`` computes it), the cell
    sizes ``c.d[NDIM]`` and ``p[]``, up to 16 doubles taken from ``params`` at every launch (reassigning ``params``
    between steps never recompiles).  ``preamble`` holds helper functions.
    ``solver.math`` is part of the compile: 'exact' and 'strict' evaluate the body without FMA contraction and with IEEE
    division and square root, 'fast' allows contraction.  A body that does not compile raises at ``setup()`` with the
    compiler's log, whose line numbers are the body's own.

    Neighbour cells (``CellSource``, ``CellDqSource``, ``CellStartStep``; a ``CellBC`` has ``qin`` / ``auxin`` instead):
    ``reach``, an integer 0..8, is the largest index offset, in any dimension, at which the body reads other cells.  With
    ``reach > 0`` the body also sees ``qn(m, di)`` (1-D), ``qn(m, di, dj)`` (2-D), ``qn(m, di, dj, dk)`` (3-D; trailing
    offsets default to 0): component ``m`` of the cell at that index offset from the lane's own cell, and
    ``auxn(m, di, dj, dk)``, the same for ``aux`` (when ``MAUX > 0``).

    * Snapshot: every ``qn`` read returns the value the cell had when the launch began, the lane's own cell included
      (``qn(m, 0, 0)`` is the old ``q[m]``) -- what a numpy callback computes when it forms the right-hand side from the
      old array and then assigns.  No lane sees a value another lane of the same launch stored.  ``q[m]`` is initialised
      with the old value and writable as before, and a component is still stored only where its bits changed.
    * Ghost cells are valid: a read may land in a ghost cell, up to ``reach`` layers.  At the launch they hold what
      ``apply_q_bcs`` gives for the state being read -- halo exchange, then the boundary conditions per dimension, lower
      then upper, corners included, ``CellBC`` and Python callbacks too.  The solver runs that fill in front of a
      ``step_src`` or ``start_step`` launch with ``reach > 0`` (the frame a hyperbolic step leaves behind is stale); a
      ``dq_src`` reads the stage's register, which the stage's own ``apply_q_bcs`` has just filled.  The aux ghost cells
      are the resident ones: uploaded with ``auxbc``, refreshed behind a ``start_step`` that writes aux.
    * No read outside the allocation, whatever the body passes: the accessors clamp every offset to ``[-reach, reach]``
      (a compile-time constant) and ``m`` to ``[0, MEQN - 1]`` (``MAUX - 1``); for literal arguments both clamps fold
      away.  ``reach <= solver.mbc`` is required (2 for the classic solvers, ``(weno_order + 1) // 2`` for SharpClaw)
      and checked at ``setup()``, at the first ``step()`` for a function assigned later, and by the library.
    * ``writes_aux=True`` with ``reach > 0`` is refused: neighbours reading aux while it is written would need a second
      snapshot.  ``qn`` in a ``reach=0`` body is a compile error that says so."""

    kind = 0
    MAX_PARAMS = 16
    MAX_REACH = 8               # the largest mbc the library takes

    def __init__(self, body, params=(), preamble="", writes_aux=False, reach=0):
        self.body = str(body)
        self.preamble = str(preamble)
        self.writes_aux = bool(writes_aux)
        if int(reach) != reach:
            raise ValueError("reach must be an integer, got %r" % (reach,))
        self.reach = int(reach)
        if self.reach < 0:
            raise ValueError("reach must be >= 0 (the largest index offset at which the body reads other cells), got %d"
                             % self.reach)
        if self.reach > self.MAX_REACH:
            raise ValueError("reach must be <= %d, the largest mbc the library takes, got %d" % (self.MAX_REACH, self.reach))
        if self.reach > 0 and self.writes_aux:
            raise ValueError("writes_aux=True together with reach=%d is not built: a body that writes aux while neighbours "
                             "read it would need a second snapshot" % self.reach)
        self.params = params
        self._fn = None            # pcl_cellfn handle and the constants it was compiled for
        self._key = None
        self.code_size = 0

    @property
    def params(self):
        return self._params

    @params.setter
    def params(self, values):
        values = np.array(values, dtype=np.float64).reshape(-1)
        if len(values) > self.MAX_PARAMS:
            raise ValueError("a cell function takes at most %d parameters, got %d" % (self.MAX_PARAMS, len(values)))
        self._params = values

    def compile(self, meqn, maux, ndim, math='exact'):
        """Compile for these shape constants (no device needed; cached per process).  Raises with the compiler's log."""
        import ctypes
        if math not in ('exact', 'fast', 'strict'):
            raise Exception("math must be 'exact', 'fast' or 'strict'")
        key = (int(meqn), int(maux), int(ndim), math, self.body, self.preamble, self.writes_aux, self.reach)
        if self._fn is not None and self._key == key:
            return self
        if self.writes_aux and maux == 0:
            raise ValueError("writes_aux needs an aux array: the state has maux == 0")
        L = _lib.lib()
        fn, size = ctypes.c_void_p(), ctypes.c_long(0)
        rc = L.pcl_cellfn_compile_reach(self.kind, self.body.encode(), self.preamble.encode(), key[0], key[1], key[2],
                                        {'exact': 0, 'fast': 1, 'strict': 2}[math], int(self.writes_aux), self.reach,
                                        ctypes.byref(fn), ctypes.byref(size))
        _lib.check(rc)
        self.release()
        self._fn, self._key, self.code_size = fn, key, int(size.value)
        return self

    def release(self):
        if self._fn is not None:
            _lib.lib().pcl_cellfn_release(self._fn)
            self._fn = None
            self._key = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def _compile_for(self, solver, state):
        self._check_reach(solver)
        return self.compile(state.meqn, state.maux, solver.ndim, solver.math)

    def _check_reach(self, solver):
        """Host only, before any device call: qn() may read ``reach`` ghost layers, the solver has ``mbc``."""
        if self.reach > solver.mbc:
            raise ValueError("%s: reach=%d, but the solver has mbc=%d ghost layers: a neighbour read could leave the "
                             "block (reach <= solver.mbc is required)" % (type(self).__name__, self.reach, solver.mbc))

    def launch(self, solver, t, dt):
        """One pass over the interior cells of the solver's selected register.  With ``reach > 0`` the caller has filled
        the ghost cells of that register (``apply``)."""
        # compiled here when the object was assigned after setup() or its text was changed since (a cache look-up otherwise)
        self._compile_for(solver, solver._state)
        p = self._params
        _lib.check(_lib.lib().pcl_cellfn_apply(solver._h, self._fn, float(t), float(dt), _lib.d(p) if len(p) else None,
                                               len(p)))
        solver._host_stale = True


class CellStartStep(CellFunction):
    """A before-step hook (``solver.start_step``) as a cell function: ``q`` is read/write, ``c.t`` is the time at the
    start of the step.  Accepted by the classic and the SharpClaw solvers in place of a Python
    ``start_step(solver, solution)``, and treated like one everywhere else: the step keeps a copied backup of q, and a
    rejected step restores it.  With ``reach > 0`` the body reads neighbour cells through ``qn`` / ``auxn`` (see
    ``CellFunction``): the solver fills the ghost cells of the current state (``apply_q_bcs``) in front of the launch.

    ``writes_aux=True`` makes ``aux[MAUX]`` writable as well (time-dependent aux, e.g. ``aux[3] = q[0];`` for the
    p-system's strain copy).  After the launch the solver fills the aux ghost cells again on the device -- halo exchange
    in a decomposed run, then the aux boundary conditions per dimension and side -- and ``state.aux`` on the host is
    refreshed when control returns to the caller or a Python callback is about to see the state.  A Python
    ``user_aux_bc_lower`` / ``user_aux_bc_upper`` cannot follow a changing aux (it is evaluated once, on the host) and is
    refused at ``setup()``."""

    kind = 3

    def apply(self, solver, state):
        if self.reach > 0:
            self._check_reach(solver)
            solver.apply_q_bcs(state)          # the frame left behind the last step is stale
        self.launch(solver, state.t, solver.dt)
        if self.writes_aux:
            solver._refresh_aux_ghosts(state)
            solver._aux_host_stale = True


class CellBC(CellFunction, DeviceBC):
    """A custom boundary condition as a cell function (see ``CellFunction``): assigned to ``solver.user_bc_lower`` and /
    or ``user_bc_upper`` (with ``bc_lower[idim] = BC.custom``) in place of a Python ``bc(state, dim, t, qbc, mbc)``.  The
    body is compiled at ``setup()`` and run as one launch per custom side over the ghost cells of that side, on the
    resident arrays -- nothing goes through the host.

    One lane is one ghost cell.  A launch covers ``mbc`` layers times the whole ghosted extent of the transverse
    dimensions, corner cells included, at the place ``apply_q_bcs`` gives a callback: behind the halo exchange, per
    dimension, lower then upper, on the blocks that own that boundary (so the y fill sees x-filled ghosts).  The body sees

    * ``q[MEQN]``, writable, initialised with the ghost cell's current contents; ``aux[MAUX]`` (const), the ghost
      cell's own aux; ``p[]`` as for every cell function;
    * ``c.t``, the time of the state being filled (the stage time in a SharpClaw stage); ``c.idim``, ``c.side``
      (0 lower, 1 upper); ``c.g``, the layer, 0 next to the boundary face up to ``mbc - 1``;
    * ``c.i[NDIM]``, the GLOBAL 0-based indices of the ghost cell -- negative on a lower side, >= n on an upper side,
      in the normal and in the transverse directions --, ``c.x[NDIM] = lower + (i + 0.5) * d`` and ``c.d[NDIM]``;
    * ``qin(m, r)`` and ``auxin(m, r)``: component ``m`` of the cell ``r`` cells inward from the boundary face on this
      ghost cell's own line along the normal, ``r = 0`` the first interior cell.  ``r`` is clamped to
      ``[0, n[idim] - 1]``; ``m`` is the caller's responsibility, like ``q[m]``.  These are the only neighbour reads:
      no launch reads a cell it writes.

    ``c.idim`` and ``c.side`` are run-time fields, so one object (and one compiled kernel) serves every dimension and
    both sides; ``dims`` restricts it to some dimensions, as on ``ConstantStateBC``.  A component is stored only where
    its bits changed.  ``SphereMirrorBC`` cannot be written this way (it reads across the transverse direction).

    ``_device_bc_spec`` is ``None`` for a solver with a ``CellBC``: every step runs ``apply_q_bcs`` followed by
    ``pcl_step_hyperbolic`` (``pcl_sharp_stage`` / ``pcl_sharp_dq``), with step-ahead and exchange-ahead off -- the
    fused ``pcl_bc_step`` knows the built-in fills only."""

    kind = 4

    def __init__(self, body, params=(), preamble="", dims=None):
        CellFunction.__init__(self, body, params, preamble)
        self.dims = dims

    def apply(self, solver, idim, side, state=None):
        """Fill the ghost cells of side (idim, side) of the solver's selected register; ``state.t`` is the body's c.t."""
        if self.dims is not None and idim not in self.dims:
            return
        if state is None:
            state = solver._state
        self._compile_for(solver, solver._state)       # (a cache look-up unless assigned or changed after setup())
        p = self._params
        _lib.check(_lib.lib().pcl_cellbc_apply(solver._h, self._fn, int(idim), int(side), float(state.t),
                                               _lib.d(p) if len(p) else None, len(p)))
        solver._host_stale = True


class CellFunctional(CellFunction):
    """Per-cell integrands reduced over the whole state on the device: what ``np.sum(f(state.q))`` or a Python
    ``compute_F`` followed by ``np.sum(np.abs(state.F[i]))`` computes on a downloaded ``q``, as one pass over the resident
    arrays that returns ``nout`` numbers.

    The body (see ``CellFunction``) reads ``q[MEQN]`` and ``aux[MAUX]``, both const, ``c.t``, ``c.i``, ``c.x``, ``c.d``
    and ``p[]`` -- with ``reach > 0`` also ``qn`` / ``auxn``, which read the register itself -- and assigns ``f[NOUT]``,
    zero on entry; ``c.dt`` is 0.  It writes nothing else: assigning ``q[...]`` or ``aux[...]`` is a compile error.  Cell
    volumes are the body's business (``c.d[]``).

    ``reduce`` is one name or a sequence of ``nout`` names out of ``'sum'``, ``'abs_sum'`` (the reference's
    ``sum|F_i|``), ``'max'`` and ``'min'``.  ``max`` / ``min`` pass over a NaN integrand (``fmax`` / ``fmin``); the sums
    propagate it.  The reduction runs over the interior cells of the block, never over ghost cells, in an order fixed by
    the block's shape: the same state gives the same bits on every call.

    ``evaluate(solver, state)`` works after ``setup()`` on every solver, in and out of resident mode, and in a
    decomposed run returns the same array on every rank.  ``claw.compute_F = CellFunctional(...)`` makes
    ``Controller.write_F`` write these values."""

    kind = 5                    # internal: compiled through pcl_cellfn_compile_reduce alone
    MAX_NOUT = 8
    OPS = {'sum': 0, 'abs_sum': 1, 'max': 2, 'min': 3}

    def __init__(self, body, nout, reduce='sum', params=(), preamble="", reach=0):
        CellFunction.__init__(self, body, params, preamble, reach=reach)
        if int(nout) != nout or not 1 <= nout <= self.MAX_NOUT:
            raise ValueError("nout must be an integer 1..%d, got %r" % (self.MAX_NOUT, nout))
        self.nout = int(nout)
        names = [reduce] * self.nout if isinstance(reduce, str) else list(reduce)
        for name in names:
            if name not in self.OPS:
                raise ValueError("reduce must be 'sum', 'abs_sum', 'max' or 'min', got %r" % (name,))
        if len(names) != self.nout:
            raise ValueError("reduce names %d operations, but nout=%d" % (len(names), self.nout))
        self.reduce = tuple(names)

    def compile(self, meqn, maux, ndim, math='exact'):
        """Compile for these shape constants (no device needed; cached per process).  Raises with the compiler's log."""
        import ctypes
        if math not in ('exact', 'fast', 'strict'):
            raise Exception("math must be 'exact', 'fast' or 'strict'")
        key = (int(meqn), int(maux), int(ndim), math, self.body, self.preamble, self.reach, self.nout, self.reduce)
        if self._fn is not None and self._key == key:
            return self
        ops = np.array([self.OPS[name] for name in self.reduce], dtype=np.int32)
        fn, size = ctypes.c_void_p(), ctypes.c_long(0)
        rc = _lib.lib().pcl_cellfn_compile_reduce(self.body.encode(), self.preamble.encode(), key[0], key[1], key[2],
                                                  {'exact': 0, 'fast': 1, 'strict': 2}[math], self.reach, self.nout,
                                                  _lib.i(ops), ctypes.byref(fn), ctypes.byref(size))
        _lib.check(rc)
        self.release()
        self._fn, self._key, self.code_size = fn, key, int(size.value)
        return self

    def launch(self, solver, t, dt):
        raise NotImplementedError("a CellFunctional stores nothing into the state: use evaluate(solver, state)")

    def evaluate(self, solver, state):
        """The ``nout`` values of the state ``pcl_get_q`` would return now, as a float64 array; the same on every rank.

        Out of resident mode the host copy is the newer one and is uploaded first, by the rule of ``step()``.  In
        resident mode the call reads the resident state and leaves a step enqueued ahead in place: it sees the accepted
        state.  With ``reach > 0`` the ghost cells are filled first (``apply_q_bcs``)."""
        from . import parallel
        self._check_reach(solver)                       # host only, before any device call
        if solver._h is None:
            raise Exception("solver.setup(solution) must be called before CellFunctional.evaluate")
        self.compile(state.meqn, state.maux, solver.ndim, solver.math)
        if not solver._pinned:
            resident = solver._resident
            solver._push(state)
            solver._resident = resident
        if self.reach > 0:
            solver.apply_q_bcs(state)
        p = self._params
        out = np.zeros(self.nout)
        _lib.check(_lib.lib().pcl_cellfn_reduce(solver._h, self._fn, float(state.t), _lib.d(p) if len(p) else None,
                                                len(p), _lib.d(out)))
        summed = parallel.allreduce_sum_host(out)
        largest = [name == 'max' for name in self.reduce]
        extreme = parallel.allreduce_minmax_host(out, largest)
        return np.array([e if name in ('max', 'min') else s for name, s, e in zip(self.reduce, summed, extreme)])


class Solver(object):
    r"""Pyclaw solver superclass; see the reference docstring (solver.py:25-125)."""

    _required_attrs = ['dt_initial', 'dt_max', 'cfl_max', 'cfl_desired', 'max_steps', 'dt_variable',
                       'mbc']
    # gauge_log / gauge_log_capacity: the device gauge log of evolve_to_time(tend), see write_gauge_values
    _default_attr_values = {'dt_initial': 0.1, 'dt_max': 1e99, 'max_steps': 1000, 'dt_variable': True,
                            'gauge_log': True, 'gauge_log_capacity': 1024}

    def __init__(self, data=None):
        self.logger = logging.getLogger('evolve')
        # class-level defaults may be extended by subclasses before calling this
        for (k, v) in self._default_attr_values.items():
            self.__dict__.setdefault(k, v)
        if data is not None:
            for attr in self._required_attrs:
                if hasattr(data, attr):
                    setattr(self, attr, getattr(data, attr))

        self.dt = self._default_attr_values['dt_initial']
        self.cfl = CFL(self._default_attr_values['cfl_desired'])
        self.status = {'cflmax': self.cfl.get_cached_max(), 'dtmin': self.dt, 'dtmax': self.dt,
                       'numsteps': 0}
        self.bc_lower = [None] * self.ndim
        self.bc_upper = [None] * self.ndim
        self.aux_bc_lower = [None] * self.ndim
        self.aux_bc_upper = [None] * self.ndim
        self.user_bc_lower = None
        self.user_bc_upper = None
        self.user_aux_bc_lower = None
        self.user_aux_bc_upper = None
        self.compute_gauge_values = None
        self.qbc = None
        self.auxbc = None
        # device handle (libpyclaw_amd) and bookkeeping
        self._h = None
        self._resident = False       # True while the HBM copy is the authoritative q
        self._pinned = False         # begin_resident()/end_resident(): keep q in HBM across calls
        self._host_stale = False
        self._aux_host_stale = False  # a start_step cell function wrote aux on the device since the last download
        self._state = None
        # device gauge log: what the handle's log was armed with (gauge cells, capacity), whether write_gauge_values
        # is on the logged path, and the times of the records the device holds
        self._glog_key = None
        self._glog_on = False
        self._glog_times = []
        self._glog_call = None       # (solution, tend is not None) of the evolve_to_time call in progress

    # ------------------------------------------------------------------ validation
    def is_valid(self):
        valid = True
        for key in self._required_attrs:
            if key not in self.__dict__:
                self.logger.info('%s is not present.' % key)
                valid = False
        if any(b == BC.custom for b in self.bc_lower) and self.user_bc_lower is None:
            valid = False
        if any(b == BC.custom for b in self.bc_upper) and self.user_bc_upper is None:
            valid = False
        return valid

    def setup(self, solution):
        pass

    def teardown(self):
        # bookkeeping that dies with the handle: how many steps ran in each form of the dimension-split 2-D step
        # (one kernel / two passes; identical results, the library runs the faster one -- pcl_step_form_stats)
        if self._h is not None and hasattr(self, "status"):
            import ctypes
            ms, n, s1, s0 = ctypes.c_double(), ctypes.c_long(), ctypes.c_long(), ctypes.c_long()
            if _lib.lib().pcl_step_form_stats(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(s1),
                                              ctypes.byref(s0)) == 0:
                self.status["step_forms"] = {"one_kernel": int(s1.value), "two_pass": int(s0.value)}
        self._gauge_log_disarm()
        self._release()

    def _release(self):
        if self._h is not None:
            _lib.lib().pcl_destroy(self._h)      # (frees an armed gauge log with the rest: no library call of its own here,
            self._h = None                       # this also runs from __del__)
        self._glog_key, self._glog_on, self._glog_times = None, False, []
        self._step_ahead_sent = None         # (what the handle was last told: pcl_step_ahead)
        self._resident = False

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def __str__(self):
        output = "Solver Status:\n"
        for (k, v) in self.status.items():
            output = "\n".join((output, "%s = %s" % (k.rjust(25), v)))
        return output

    # ------------------------------------------------------------------ host <-> device
    def _push(self, state):
        """state.q (host) -> HBM; the device copy becomes authoritative."""
        q = _lib.fortran64(state.q)
        _lib.check(_lib.lib().pcl_put_q(self._h, _lib.d(q), 0))
        self._resident = True
        self._host_stale = False
        self._state = state

    def _pull(self, state):
        """HBM -> state.q (host), if the host copy is stale."""
        if self._resident and self._host_stale:
            if not (state.q.flags.f_contiguous and state.q.dtype == np.float64 and state.q.flags.writeable):
                state.q = np.empty(state.q.shape, order='F')
            _lib.check(_lib.lib().pcl_get_q(self._h, _lib.d(state.q), 0))
            self._host_stale = False
        self._pull_aux(state)

    def _pull_aux(self, state):
        """HBM -> state.aux (host) and the solver's auxbc, if a start_step cell function has written aux on the device
        since the last download (CellStartStep(writes_aux=True)).  Runs wherever Python code is about to see the state:
        with _pull, and in front of a Python custom-BC callback."""
        if self._aux_host_stale and self._h is not None:
            _lib.check(_lib.lib().pcl_get_aux(self._h, _lib.d(self.auxbc)))
            interior = (slice(None),) + (slice(self.mbc, -self.mbc),) * self.ndim
            state.aux[...] = self.auxbc[interior]
            self._aux_host_stale = False

    # ------------------------------------------------------------------ cell functions
    def _cell_functions(self):
        fns = [getattr(self, name, None) for name in ('start_step', 'step_src', 'dq_src', 'user_bc_lower', 'user_bc_upper')]
        return [f for f in fns if isinstance(f, CellFunction)]

    def _check_cell_functions(self, state):
        """What the cell functions among start_step / step_src / dq_src cannot be given, refused before the device
        handle exists (setup(), next to the check of a user-written Riemann solver)."""
        for fn in self._cell_functions():
            fn._check_reach(self)

    def _setup_cell_functions(self, state):
        """Called by setup() once the device handle exists: tell the library where this block sits in the global grid
        (a body's c.i and c.x are global) and compile the cell functions among start_step / step_src / dq_src and the
        custom boundary conditions."""
        dims = state.grid.dimensions
        lower = np.array([dim.lower for dim in dims], dtype=np.float64)
        nstart = np.array([dim.nstart for dim in dims], dtype=np.int32)
        _lib.check(_lib.lib().pcl_cellfn_geometry(self._h, _lib.d(lower), _lib.i(nstart)))
        self._state = state
        self._aux_host_stale = False
        for fn in self._cell_functions():
            if fn.writes_aux and (self.user_aux_bc_lower is not None or self.user_aux_bc_upper is not None):
                raise NotImplementedError("a start_step that writes aux cannot be combined with a Python user_aux_bc_lower / "
                                          "user_aux_bc_upper: the callback is evaluated once on the host and cannot "
                                          "follow a changing aux")
            fn._compile_for(self, state)

    # ------------------------------------------------------------------ boundary conditions
    def allocate_bc_arrays(self, state):
        r"""qbc/auxbc host arrays with ghost cells (solver.py:297-313).  qbc is only a staging
        area for Python custom-BC callbacks here; auxbc is filled once and uploaded."""
        qbc_dim = [n + 2 * self.mbc for n in state.grid.ng]
        qbc_dim.insert(0, state.meqn)
        self.qbc = np.zeros(qbc_dim, order='F')
        if state.maux > 0:
            auxbc_dim = [n + 2 * self.mbc for n in state.grid.ng]
            auxbc_dim.insert(0, state.maux)
            self.auxbc = np.empty(auxbc_dim, order='F')
            self.apply_aux_bcs(state)
        else:
            self.auxbc = None

    def _at_lower(self, dim):
        return dim.nstart == 0

    def _at_upper(self, dim):
        return dim.nend == dim.n

    def apply_q_bcs(self, state):
        r"""Fill the ghost cells of the resident q (solver.py:315-381), same order: per
        dimension, lower then upper; only on blocks that touch the physical boundary.  In a
        decomposed run the halo exchange comes first (petclaw: globalToLocal inside
        get_qbc_from_q, src/petclaw/state.py:254-262)."""
        L = _lib.lib()
        if self._halo_active:
            _lib.check(L.pcl_halo_exchange(self._h))
        grid = state.grid
        for idim, dim in enumerate(grid.dimensions):
            whole = self._at_lower(dim) and self._at_upper(dim)
            if self._at_lower(dim):
                bc = self.bc_lower[idim]
                if bc == BC.custom:
                    self._custom_bc(state, dim, idim, 0, self.user_bc_lower)
                elif bc == BC.periodic:
                    if whole:
                        _lib.check(L.pcl_bc(self._h, idim, 0, bc))
                elif bc in (BC.outflow, BC.reflecting):
                    _lib.check(L.pcl_bc(self._h, idim, 0, bc))
                else:
                    raise NotImplementedError("Boundary condition %s not implemented" % bc)
            if self._at_upper(dim):
                bc = self.bc_upper[idim]
                if bc == BC.custom:
                    self._custom_bc(state, dim, idim, 1, self.user_bc_upper)
                elif bc == BC.periodic:
                    if whole:
                        _lib.check(L.pcl_bc(self._h, idim, 1, bc))
                elif bc in (BC.outflow, BC.reflecting):
                    _lib.check(L.pcl_bc(self._h, idim, 1, bc))
                else:
                    raise NotImplementedError("Boundary condition %s not implemented" % bc)

    def _device_bc_spec(self, state):
        """(types[2*ndim], constant states) for pcl_bc_step when every ghost fill of apply_q_bcs can
        run on the device (no plain-Python callback), else None.  Cached per solver setup."""
        key = (tuple(self.bc_lower), tuple(self.bc_upper), id(self.user_bc_lower), id(self.user_bc_upper))
        cached = getattr(self, '_bc_spec_cache', None)
        if cached is not None and cached[0] == key:
            return cached[1]
        types = np.full(2 * self.ndim, -1, dtype=np.int32)
        consts = np.zeros(2 * self.ndim * _lib.MAX_RP_PARAMS)
        spec = (types, consts)
        for idim, dim in enumerate(state.grid.dimensions):
            whole = self._at_lower(dim) and self._at_upper(dim)
            for side, at_edge, bcs, fn in ((0, self._at_lower(dim), self.bc_lower, self.user_bc_lower),
                                           (1, self._at_upper(dim), self.bc_upper, self.user_bc_upper)):
                if not at_edge:
                    continue
                bc = bcs[idim]
                k = 2 * idim + side
                if bc == BC.custom:
                    if isinstance(fn, ConstantStateBC) and state.meqn <= _lib.MAX_RP_PARAMS:
                        if fn.dims is None or idim in fn.dims:
                            types[k] = BC.custom
                            consts[k * _lib.MAX_RP_PARAMS:k * _lib.MAX_RP_PARAMS + state.meqn] = fn.state
                    elif (isinstance(fn, SphereMirrorBC) and self.ndim == 2 and idim == 1 and self._mirror_in_spec()
                          and (state.decomp is None or state.decomp.dims[0] == 1)):
                        types[k] = 4                       # PCL_BC_SPHERE_MIRROR
                    else:
                        spec = None
                elif bc == BC.periodic:
                    if whole:
                        types[k] = bc
                elif bc in (BC.outflow, BC.reflecting):
                    types[k] = bc
                else:
                    spec = None
        if spec is not None:
            # (types, consts, their ctypes pointers): the pointers are built once, not on every step
            spec = (types, consts, _lib.i(types), _lib.d(consts))
        self._bc_spec_cache = (key, spec)
        return spec

    def _mirror_in_spec(self):
        """the library takes the sphere app's pole boundary inside pcl_bc_step (unsplit classic step) and inside the
        SharpClaw stage calls; the dimension-split classic step evaluates its BCs in the x pass and does not"""
        return getattr(self, 'lim_type', None) is not None or not getattr(self, 'dim_split', True)

    def _custom_bc(self, state, dim, idim, side, fn):
        if fn is None:
            raise Exception("Custom BC requested but user_bc_%s is not set" % ("lower", "upper")[side])
        if isinstance(fn, CellBC):
            fn.apply(self, idim, side, state)       # the state carries the time (a stage's, in SharpClaw)
            return
        if isinstance(fn, DeviceBC):
            fn.apply(self, idim, side)
            return
        # Plain Python callback (state,dim,t,qbc,mbc): give it the reference's full qbc array
        # (solver.py:404-405), then send back only the ghost layers of this side.
        L = _lib.lib()
        self._pull_aux(state)          # a stage's _StageState shares the aux array of the solver's state
        _lib.check(L.pcl_get_q(self._h, _lib.d(self.qbc), 1))
        fn(state, dim, state.t, self.qbc, self.mbc)
        idx = [slice(None)] * self.qbc.ndim
        idx[idim + 1] = slice(0, self.mbc) if side == 0 else slice(self.qbc.shape[idim + 1] - self.mbc, None)
        strip = np.asfortranarray(self.qbc[tuple(idx)])
        _lib.check(L.pcl_put_strip(self._h, idim, side, self.mbc, _lib.d(strip)))

    def apply_aux_bcs(self, state):
        r"""Host-side aux ghost fill, once at setup (solver.py:456-596)."""
        self.auxbc = state.get_qbc_from_q(self.mbc, 'aux', self.auxbc)
        grid = state.grid
        mbc = self.mbc
        for idim, dim in enumerate(grid.dimensions):
            whole = self._at_lower(dim) and self._at_upper(dim)
            if self._at_lower(dim):
                bc = self.aux_bc_lower[idim]
                if bc == BC.custom:
                    self.user_aux_bc_lower(state, dim, state.t, self.auxbc, mbc)
                elif bc == BC.periodic and not whole:
                    pass
                else:
                    a = np.rollaxis(self.auxbc, idim + 1, 1)
                    if bc == BC.outflow:
                        for i in range(mbc):
                            a[:, i, ...] = a[:, mbc, ...]
                    elif bc == BC.periodic:
                        a[:, :mbc, ...] = a[:, -2 * mbc:-mbc, ...]
                    elif bc == BC.reflecting:
                        for i in range(mbc):
                            a[:, i, ...] = a[:, 2 * mbc - 1 - i, ...]
                    elif bc is None:
                        raise Exception("One or more of the aux boundary conditions aux_bc_upper has not been specified.")
                    else:
                        raise NotImplementedError("Boundary condition %s not implemented" % bc)
            if self._at_upper(dim):
                bc = self.aux_bc_upper[idim]
                if bc == BC.custom:
                    self.user_aux_bc_upper(state, dim, state.t, self.auxbc, mbc)
                elif bc == BC.periodic and not whole:
                    pass
                else:
                    a = np.rollaxis(self.auxbc, idim + 1, 1)
                    if bc == BC.outflow:
                        for i in range(mbc):
                            a[:, -i - 1, ...] = a[:, -mbc - 1, ...]
                    elif bc == BC.periodic:
                        a[:, -mbc:, ...] = a[:, mbc:2 * mbc, ...]
                    elif bc == BC.reflecting:
                        for i in range(mbc):
                            a[:, -i - 1, ...] = a[:, -2 * mbc + i, ...]
                    elif bc is None:
                        raise Exception("One or more of the aux boundary conditions aux_bc_lower has not been specified.")
                    else:
                        raise NotImplementedError("Boundary condition %s not implemented" % bc)

    def _upload_aux(self, state):
        """auxbc -> HBM.  Decomposed runs: exchange the aux halo, then redo the physical aux BCs on
        the device so that corner ghost cells next to a neighbour face are right (the reference
        order: globalToLocal, then auxbc_lower/upper; solver.py:492-523)."""
        if self.auxbc is None:
            return
        L = _lib.lib()
        _lib.check(L.pcl_put_aux(self._h, _lib.d(_lib.fortran64(self.auxbc))))
        if not self._halo_active:
            return
        self._refresh_aux_ghosts(state)

    def _refresh_aux_ghosts(self, state):
        """Ghost cells of the resident aux from its interior, on the device, in the reference's order: halo exchange in a
        decomposed run, then the physical aux BCs per dimension, lower then upper (solver.py:492-523).  Runs behind the
        upload of a decomposed run and behind every start_step cell function that writes aux."""
        L = _lib.lib()
        if self._halo_active:
            _lib.check(L.pcl_halo_exchange_aux(self._h))
        for idim, dim in enumerate(state.grid.dimensions):
            whole = self._at_lower(dim) and self._at_upper(dim)
            for side, at_edge, bcs in ((0, self._at_lower(dim), self.aux_bc_lower),
                                       (1, self._at_upper(dim), self.aux_bc_upper)):
                if not at_edge:
                    continue
                bc = bcs[idim]
                if bc == BC.custom:
                    # the callback filled these ghost layers of the host auxbc (apply_aux_bcs), over the whole
                    # ghosted width of the block; they go onto the device at the callback's place in the reference
                    # order (exchange, then per dimension lower / upper).  Right as long as the callback computes
                    # them from positions alone, like the sphere app's setaux rows: one that copies interior values
                    # would miss the exchanged cells next to a neighbour face.
                    idx = [slice(None)] * self.auxbc.ndim
                    idx[idim + 1] = (slice(0, self.mbc) if side == 0
                                     else slice(self.auxbc.shape[idim + 1] - self.mbc, None))
                    strip = np.asfortranarray(self.auxbc[tuple(idx)])
                    _lib.check(L.pcl_put_aux_strip(self._h, idim, side, self.mbc, _lib.d(strip)))
                    continue
                if bc == BC.periodic and not whole:
                    continue
                _lib.check(L.pcl_bc_aux(self._h, idim, side, bc))

    # ------------------------------------------------------------------ multi-GPU glue
    _halo_active = False

    def _setup_halo(self, state):
        """Join the RCCL communicator if the state's grid is decomposed over several GPUs."""
        dec = state.decomp
        if dec is None:
            self._halo_active = False
            return
        L = _lib.lib()
        import ctypes as C
        import os
        # PetClaw's DMDA is periodic in every direction and the physical BCs overwrite the ghost cells of the sides
        # that are not (petclaw/state.py:205-208): a dimension wraps around as soon as EITHER of its sides is periodic
        # (the reference's 3-D heterogeneous test has reflecting lower and periodic upper sides)
        periodic = [self.bc_lower[k] == BC.periodic or self.bc_upper[k] == BC.periodic for k in range(state.grid.ndim)]
        nbr = np.array(dec.neighbors(periodic), dtype=np.int32)
        def host_wire():
            # host-staged wire: same device path, this module's TCP group instead of RCCL
            self._host_transport = parallel.host_transport()
            xfn, rfn = self._host_transport
            _lib.check(L.pcl_comm_init_host(self._h, parallel.world_size(), parallel.rank(), _lib.i(nbr),
                                            C.cast(xfn, C.c_void_p), C.cast(rfn, C.c_void_p), None))
            self._halo_active = True
            self.cfl._reduce = None

        if os.environ.get("PCL_HALO_TRANSPORT", "rccl") == "host":     # diagnostics; several ranks on ONE device
            self.halo_transport = "host"
            return host_wire()
        # RCCL.  Every rank learns whether EVERY rank got its communicator (a failure on one rank -- librccl missing,
        # ncclCommInitRank refusing -- must not leave the others waiting inside a collective).
        err = None
        uid = C.create_string_buffer(128)
        try:                                  # on every rank: loads librccl (rank 0's id is the one that is used)
            _lib.check(L.pcl_comm_unique_id(uid))
        except _lib.PclError as e:
            err = str(e)
        loaded = [e for e in parallel.allgather(err) if e]      # nobody enters ncclCommInitRank unless all can
        raw = parallel.broadcast_bytes((uid.raw if not loaded else b"") if parallel.rank() == 0 else None, src=0)
        if len(raw) != 128:
            err = err or loaded[0]
        else:
            try:
                _lib.check(L.pcl_comm_init(self._h, parallel.world_size(), parallel.rank(),
                                           C.create_string_buffer(raw, 128), _lib.i(nbr)))
            except _lib.PclError as e:
                err = str(e)
        errs = [e for e in parallel.allgather(err) if e]
        if errs:
            if os.environ.get("PCL_HALO_FALLBACK", "") != "host":
                raise Exception("RCCL communicator set-up failed on %d rank(s): %s  (PCL_HALO_FALLBACK=host would "
                                "run the same device path over the host-staged wire)" % (len(errs), errs[0]))
            self.logger.warning("RCCL set-up failed (%s): falling back to the host-staged halo wire" % errs[0])
            self.halo_transport = "host (fallback: RCCL set-up failed: %s)" % errs[0]
            return host_wire()
        self.halo_transport = "rccl"
        self._halo_active = True
        # the CFL all-reduce (petclaw/cfl.py:29-31) happens inside pcl_step_hyperbolic /
        # pcl_sharp_dq on the device: the value they return is already the global maximum
        self.cfl._reduce = None

    # ------------------------------------------------------------------ evolution
    def evolve_to_time(self, solution, tend=None):
        r"""Evolve solution from solution.t to tend (one step if tend is None); returns the
        status dict.  Line-for-line semantics of solver.py:602-717."""
        if self._h is None:
            raise Exception("solver.setup(solution) must be called before evolve_to_time")
        take_one_step = tend is None
        retake_step = False
        tstart = solution.t

        self.status['cflmax'] = self.cfl.get_cached_max()
        self.status['dtmin'] = self.dt
        self.status['dtmax'] = self.dt
        self.status['numsteps'] = 0

        if not self.dt_variable:
            if take_one_step:
                self.max_steps = 1
            else:
                self.max_steps = int((tend - tstart + 1e-10) / self.dt)
                if abs(self.max_steps * self.dt - (tend - tstart)) > 1e-5 * (tend - tstart):
                    raise Exception('dt does not divide (tend-tstart) and dt is fixed!')
        if self.dt_variable == 1 and self.cfl_desired > self.cfl_max:
            raise Exception('Variable time-stepping and desired CFL > maximum CFL')
        if (not take_one_step) and tend <= tstart:
            self.logger.info("Already at or beyond end time: no evolution required.")
            self.max_steps = 0

        state = solution.state
        if not self._pinned:
            self._push(state)
        self._arm_step_ahead(state, take_one_step)
        self._glog_call = (solution, not take_one_step)
        failed = True                # until the loop has ended without an exception
        try:
            self._gauge_log_decide()
            for n in range(self.max_steps):
                state = solution.state
                if (not take_one_step) and solution.t + self.dt > tend and tstart < tend:
                    self.dt = tend - solution.t

                if self.dt_variable:
                    self._backup(state)          # q_backup = state.q.copy('F')
                    told = solution.t
                retake_step = False

                self.step(solution)

                cfl = self.cfl.get_cached_max()
                if cfl <= self.cfl_max:
                    self.status['cflmax'] = max(cfl, self.status['cflmax'])
                    if self.dt_variable == True:
                        solution.t += self.dt
                    else:
                        solution.t = tstart + (n + 1) * self.dt
                    if self.logger.isEnabledFor(logging.DEBUG):
                        self.logger.debug("Step %i  CFL = %f   dt = %f   t = %f" % (n, cfl, self.dt, solution.t))
                    self.write_gauge_values(solution)
                    self.status['numsteps'] += 1
                    if take_one_step or solution.t >= tend:
                        break
                else:
                    self.logger.debug("Rejecting time step, CFL number too large")
                    if self.dt_variable:
                        self._restore(state)     # state.q = q_backup
                        solution.t = told
                        retake_step = True
                    else:
                        self.status['cflmax'] = max(cfl, self.status['cflmax'])
                        raise Exception('CFL too large, giving up!')

                if self.dt_variable:
                    if cfl > 0.0:
                        self.dt = min(self.dt_max, self.dt * self.cfl_desired / cfl)
                        self.status['dtmin'] = min(self.dt, self.status['dtmin'])
                        self.status['dtmax'] = max(self.dt, self.status['dtmax'])
                    else:
                        self.dt = self.dt_max
            failed = False
        finally:
            # the gauge files are complete whenever evolve_to_time has returned.  (Behind an exception of the loop the
            # device may hold the record of a step that was never accepted: what was accepted is written, and one record
            # more is not an error of its own.)
            try:
                if self._glog_key is not None:
                    self._gauge_log_flush(strict=not failed)
            finally:
                self._glog_on = False
                self._glog_call = None
                if not self._pinned:
                    self._pull(solution.state)
                    self._resident = False

        if self.dt_variable and (not take_one_step) and solution.t < tend \
                and self.status['numsteps'] == self.max_steps:
            raise Exception("Maximum number of timesteps have been taken")
        return self.status

    def step(self, solution):
        raise NotImplementedError("No stepping routine has been defined!")

    # Extension of the reference surface: keep q resident in HBM across several
    # evolve_to_time calls (the reference's state.q is host memory, so every call would
    # otherwise upload at entry and download at exit).  state.q on the host is stale in
    # between; end_resident() refreshes it.
    def begin_resident(self, solution):
        self._push(solution.state)
        self._pinned = True

    def end_resident(self, solution):
        self._pull(solution.state)
        self._pinned = False
        self._resident = False
        self._arm_step_ahead(solution.state)         # no longer pinned: disarms

    # Resident mode runs one step ahead where the library can (pcl_step_ahead; ClawSolver decides): nothing here
    def _arm_step_ahead(self, state, one_step=False):
        pass

    # backup/restore of the resident state; subclasses pick the cheap form when legal
    def _backup(self, state):
        _lib.check(_lib.lib().pcl_backup(self._h))

    def _restore(self, state):
        _lib.check(_lib.lib().pcl_restore(self._h))
        self._host_stale = True

    # ------------------------------------------------------------------ gauges
    def _gauge_log_eligible(self):
        """Whether the steps of this solver can record their gauge cells themselves (ClawSolver decides)."""
        return False

    def _gauge_log_decide(self):
        """Put write_gauge_values on the logged or on the direct path.  At the entry of evolve_to_time, and again by
        ClawSolver.step when it has decided the source fusion afresh.  Before any switch the records held are written, so
        the lines of a file stay in the order of the steps."""
        solution, has_tend = self._glog_call if self._glog_call is not None else (None, False)
        gauges = solution.state.grid.gauges if solution is not None else []
        if not gauges and self._glog_key is None:        # (the common case, every call of a run without gauges)
            self._glog_on = False
            return
        import os
        on = bool(has_tend and gauges and self.gauge_log and os.environ.get("PCL_GAUGE_LOG", "1") != "0"
                  and self._h is not None and self._resident and self._gauge_log_eligible()
                  and hasattr(_lib.lib(), "pcl_gauge_log"))        # (an older build of the library, PCL_LIB_OVERRIDE)
        if not on:
            if self._glog_key is not None:
                self._gauge_log_flush()
                self._gauge_log_disarm()      # the direct path: the steps stop recording
            self._glog_on = False
            return
        capacity = max(1, int(self.gauge_log_capacity))
        key = (tuple(tuple(int(i) for i in g) for g in gauges), capacity)
        if key != self._glog_key:
            self._gauge_log_flush()
            ij = np.zeros((len(gauges), 3 if self.ndim > 2 else 2), dtype=np.int32)      # (i, j) pairs; (i, j, k) in 3-D
            for c, g in enumerate(gauges):
                ij[c, :len(g)] = g
            self._glog_key = None            # (a failed arming has freed the log that was there)
            _lib.check(_lib.lib().pcl_gauge_log(self._h, len(gauges), _lib.i(ij), capacity))
            self._glog_key = key
        self._glog_on = True

    def _gauge_log_disarm(self):
        if self._glog_key is not None and self._h is not None:
            _lib.check(_lib.lib().pcl_gauge_log(self._h, 0, None, 0))
        self._glog_key = None
        self._glog_on = False
        self._glog_times = []

    def _gauge_log_flush(self, strict=True):
        """Read the records the device holds -- one per accepted step since the last flush -- and write their lines."""
        import ctypes
        times = self._glog_times
        if self._glog_key is None or self._h is None or self._glog_call is None:
            return
        solution = self._glog_call[0]
        state, grid = solution.state, solution.state.grid
        ncell, capacity = len(self._glog_key[0]), self._glog_key[1]
        per = state.meqn + state.maux
        nmax = min(capacity, len(times) + 1)         # (room for one record too many: reported below, not by the library)
        out = np.empty((nmax, ncell, per))
        nrec = ctypes.c_int(0)
        _lib.check(_lib.lib().pcl_gauge_log_read(self._h, nmax, _lib.d(out), ctypes.byref(nrec)))
        self._glog_times = []
        if nrec.value != len(times) and (strict or nrec.value < len(times)):
            raise Exception("gauge log: the device holds %d records for %d accepted steps" % (nrec.value, len(times)))
        compute = self.compute_gauge_values or default_compute_gauge_values
        for r, t in enumerate(times):
            for i in range(ncell):
                p = compute(out[r, i, :state.meqn], out[r, i, state.meqn:])
                grid.gauge_files[i].write(str(t) + ' ' + ' '.join(str(j) for j in p) + '\n')

    def write_gauge_values(self, solution):
        r"""solver.py:731-741.  While the state is resident the gauge cells are gathered on the device
        (pcl_get_cells: ngauges*(meqn+maux) doubles over PCIe) instead of pulling the whole q.

        Inside ``evolve_to_time(tend)`` of a classic solver whose steps end with the hyperbolic step (no source, or the
        fused one) nothing is gathered here at all: every step has recorded its gauge cells into a log on the device
        (``pcl_gauge_log``), this method notes the time, and the lines are written when the log is read -- at
        ``gauge_log_capacity`` records, and before ``evolve_to_time`` returns.  Same lines, same bytes;
        ``compute_gauge_values(q, aux)`` is called then, not after each step, so it must be a function of its arguments
        alone.  ``solver.gauge_log = False`` (or PCL_GAUGE_LOG=0) keeps the gather after every step."""
        grid = solution.state.grid
        gauges = grid.gauges
        if not gauges:
            return
        if self._glog_on:
            self._glog_times.append(solution.t)
            if len(self._glog_times) >= self._glog_key[1]:
                self._gauge_log_flush()
            return
        state = solution.state
        compute = self.compute_gauge_values or default_compute_gauge_values
        if self._resident and self._h is not None:
            n = len(gauges)
            ij = np.zeros((n, 3 if state.grid.ndim > 2 else 2), dtype=np.int32)      # (i, j) pairs; (i, j, k) in 3-D
            for c, g in enumerate(gauges):
                ij[c, :len(g)] = g
            qv = np.empty((n, state.meqn))
            av = np.empty((n, max(state.maux, 1)))
            _lib.check(_lib.lib().pcl_get_cells(self._h, n, _lib.i(ij), _lib.d(qv),
                                                _lib.d(av) if state.maux > 0 else None))
            cells = [(qv[c], av[c, :state.maux]) for c in range(n)]
        else:
            cells = [(state.q[(slice(None),) + tuple(g)],
                      state.aux[(slice(None),) + tuple(g)] if state.aux is not None else None) for g in gauges]
        for i, (q, aux) in enumerate(cells):
            p = compute(q, aux)
            grid.gauge_files[i].write(str(solution.t) + ' ' + ' '.join(str(j) for j in p) + '\n')
