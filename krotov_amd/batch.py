"""``optimize_pulses_batch``: many independent small optimisations as one batch on the device.

A *replica* is one complete :func:`~krotov_amd.optimize.optimize_pulses` problem -- its own objectives,
``pulse_options`` and ``tlist``.  B replicas of the same shape (objectives per replica, dimension, number of
controls, grid length, kind) run on ONE replica engine (``kh_engine_create_replicas``, kernel family
``"replica16/wave"``): per Krotov iteration of the whole batch one ``kh_tau``, one ``kh_chi_boundary``, one backward
sweep and one update sweep, where a Python loop over ``optimize_pulses`` creates B engines and pays three launches per
replica and iteration.  Replicas stop on their own (``check_convergence``, ``iter_stop``): a finished one is frozen
through the engine's active mask.  With ``sigma`` (one ``Sigma`` per problem) the update sweep is the second-order
one, every replica under its own sigma(t) (``kh_set_second_order_replicas``).  Whatever does not fit one batch runs
the replicas one after another through ``optimize_pulses``, with the same results.
"""
import copy
import logging
import time

import numpy as np

from . import functionals as _functionals
from . import optimize as _opt
from ._run import RunRecord, chained_hook, default_norm, host_costates
from .mixed import layout_of
from .mu import derivative_wrt_pulse
from .propagators import HipExpm, expm

__all__ = ['optimize_pulses_batch']

# the limits of the replica kernels (defined next to the checks that use them)
REPLICA_NMAX, REPLICA_KMAX, REPLICA_LMAX = _opt.REPLICA_NMAX, _opt.REPLICA_KMAX, _opt.REPLICA_LMAX


def _free_device_bytes():
    """Free memory of the current device, or None where there is none to ask (engine doubles on the host)."""
    import torch

    if not torch.cuda.is_available():
        return None
    return int(torch.cuda.mem_get_info()[0])


class _Replica(RunRecord):
    """One problem of the batch: its run record, what ``optimize_pulses`` keeps in local variables next to its own, and
    what only a batch needs (``active``, ``li_values``, ``midpoints``; the backend adds ``likes`` and ``weights``)."""

    def __init__(self, problem, propagator, chi_constructor, iter_stop, store_all_pulses, continue_from, sigma=None,
                 info_hook=None, check_convergence=None):
        self.objectives = problem['objectives']
        self.pulse_options = problem['pulse_options']
        self.tlist = problem['tlist']
        self.adjoint_objectives = [obj.adjoint() for obj in self.objectives]
        (self.guess_controls, self.guess_pulses, self.pulses_mapping, self.lambda_vals,
         self.shape_arrays) = _opt._initialize_krotov_controls(self.objectives, self.pulse_options, self.tlist)
        if continue_from is not None:
            self.guess_controls, self.guess_pulses = _opt._restore_from_previous_result(
                continue_from, self.objectives, self.tlist, store_all_pulses)
        self.L = len(self.guess_pulses)
        self.g_a_integrals = np.zeros(self.L)
        static_args = dict(
            objectives=self.objectives, adjoint_objectives=self.adjoint_objectives, lambda_vals=self.lambda_vals,
            shape_arrays=self.shape_arrays, tlist=self.tlist, propagator=propagator, chi_constructor=chi_constructor,
            mu=derivative_wrt_pulse, sigma=sigma, iter_start=0, iter_stop=iter_stop,
        )
        super().__init__(static_args, continue_from, store_all_pulses, info_hook, check_convergence)
        self.sigma = sigma
        self.midpoints = None  # (second order: the interval mid-points sigma is evaluated at)
        self.optimized_pulses = copy.deepcopy(self.guess_pulses)
        self.tau_vals = None
        self.fw_states_T = None
        self.forward_states0 = None  # second order: this replica's view of the trajectory under its guess pulses
        self.active = True
        self.iteration = 0
        self.li_values = None  # PerfectEntanglerChi / LocalInvariantsChi: the J per gate of this problem's last co-states

    def stop(self):
        """The run is over: the Result is finished and this replica holds no device reference any more."""
        self.active = False
        self.forward_states0 = None
        self.finish(self.optimized_pulses)


def _batch_obstacle(problems, reps, propagator):
    """Why these problems cannot run as one batch (a short reason), or None."""
    if isinstance(propagator, list) or not (propagator is expm or isinstance(propagator, HipExpm)):
        return "the propagator is not expm / HipExpm"
    if any(_opt._parametrizations(r.objectives, r.pulse_options) is not None for r in reps):
        return "a pulse parametrization ('parametrization' in pulse_options)"
    if any(_opt.has_control_function(r.objectives) for r in reps):
        return "non-linear controls (a ControlFunction in H)"
    for r in reps:  # (what a single problem must be: shared with optimize_pulses' own use of a one-replica engine)
        reason = _opt._replica_kind_obstacle(r.objectives, propagator)
        if reason is not None:
            return reason
    layouts = [layout_of(r.objectives, propagator) for r in reps]
    shapes = {(len(r.objectives), lay.stride, lay.kinds[0], r.L, len(r.tlist)) for r, lay in zip(reps, layouts)}
    if len(shapes) > 1:
        return "the problems differ in shape"
    Kr, N, _, L, _ = next(iter(shapes))
    return _opt._replica_size_obstacle(N, Kr, L)


class _ReplicaBackend:
    """The B replicas of one (sub-)batch resident on one replica engine; every buffer a sweep writes is persistent, so
    that a frozen replica's slices keep their last values."""

    def __init__(self, reps, propagator, second_order=False):
        import torch

        from .engine import HipKrotovEngine

        self.torch = t = torch
        self.reps = reps
        self.B, self.Kr, self.L = len(reps), len(reps[0].objectives), reps[0].L
        self.K = self.B * self.Kr
        layout = layout_of(reps[0].objectives, propagator)
        self.N, self.is_super = layout.stride, layout.kinds[0]
        self.nt = len(reps[0].tlist)
        ops = []
        for r in reps:
            ops += _opt._operator_rows(r.objectives, r.pulses_mapping, self.L, _opt.to_dense)[0]
        dts = np.array([np.diff(np.asarray(r.tlist, dtype=np.float64)) for r in reps])
        self.engine = eng = HipKrotovEngine(ops, dts, is_super=self.is_super, replicas=self.B)
        init, targets = [], []
        for r in reps:
            lay = layout_of(r.objectives, propagator)
            r.likes = [obj.initial_state for obj in r.objectives]
            vecs = [lay.vector(obj.initial_state, k) for k, obj in enumerate(r.objectives)]
            if any(v is None for v in vecs):
                raise ValueError("initial states do not match the operator dimension %s" % self.N)
            init += vecs
            targets += [lay.vector(obj.target, k) for k, obj in enumerate(r.objectives)]
            w = [getattr(obj, 'weight', None) for obj in r.objectives]
            r.weights = None if all(x is None for x in w) else np.array([1.0 if x is None else x for x in w])
        self.init = eng.dev(np.array(init), t.complex128)
        self.targets = None if any(v is None for v in targets) else eng.dev(np.array(targets), t.complex128)
        c128, f64, dev = t.complex128, t.float64, eng.device
        self.psi_T = t.zeros((self.K, self.N), dtype=c128, device=dev)
        self.chi_store = t.zeros((self.K, self.nt, self.N), dtype=c128, device=dev)
        self.opt = t.zeros((self.B, self.L, self.nt - 1), dtype=f64, device=dev)
        self.g_a = t.zeros((self.B, self.L), dtype=f64, device=dev)
        # second order: phi(t_n) of the last / the running iteration, swapped once per pass for the whole batch (a
        # frozen replica's slices of either are never read again)
        self.second_order = second_order
        self.fw_prev = self.fw_next = None
        if second_order:
            self.fw_prev = t.zeros((self.K, self.nt, self.N), dtype=c128, device=dev)
            self.fw_next = t.zeros((self.K, self.nt, self.N), dtype=c128, device=dev)
            self.sigma_host = np.zeros((self.B, self.nt - 1))
        self.last_chi = None
        self.propagator = propagator
        self.li_out = self.li_J = None  # kh_chi_local_invariants: (chi_T, chi_norms, J) of the batch; J alone
        self._uploads = _opt._UploadCache(eng, t.float64)
        self._mask = None

    def _pulses(self, key, which):
        host = np.array([np.array(getattr(r, which), dtype=np.float64).reshape(self.L, self.nt - 1) for r in self.reps])
        return self._uploads.get(key, host)

    def set_active(self):
        mask = [1 if r.active else 0 for r in self.reps]
        if mask != self._mask:
            self.engine.set_active_replicas(None if all(mask) else mask)
            self._mask = mask

    def initial_forward(self):
        pulses = self._pulses('pulses', 'guess_pulses')
        if self.second_order:  # (the trajectory under the guess: forward_states0 of iteration 1)
            self.engine.forward(pulses, self.init, store=True, out=(self.psi_T, self.fw_prev))
        else:
            self.engine.forward(pulses, self.init, out=self.psi_T)
        return self.psi_T.cpu().numpy()

    def trajectories(self, store, b, likes, final):
        """Replica b's slices of a (K, nt, N) store, for ``info_hook`` and ``sigma.refresh`` (views: they follow the
        buffer through ``advance_second_order``).  ``final``: the states at T of all objectives on the host -- what
        ``numerical_estimate_A`` reads, B K_r times per pass, without a device copy each (a copy of the rows: the
        sweeps write ``psi_T`` in place)."""
        rows = slice(b * self.Kr, (b + 1) * self.Kr)
        return _opt._DeviceTrajectories(store[rows], likes, final=np.array(final[rows]))

    def chi_host(self):
        """Normalised chi_k(T) and their norms of the last iteration, (K, N) and (K,), on the host."""
        chi, norms = self.last_chi
        return chi.cpu().numpy(), norms.cpu().numpy()

    def advance_second_order(self):
        """The trajectory of the finished iteration becomes ``forward_states0`` of the next one (optimize.py:577): one
        swap for the whole batch."""
        self.fw_prev, self.fw_next = self.fw_next, self.fw_prev

    def tau_vals(self):
        """(B, K_r) on the host from one kh_tau over all objectives, or None without state targets."""
        if self.targets is None:
            return None
        return self.engine.tau(self.targets, self.psi_T).cpu().numpy().reshape(self.B, self.Kr)

    def local_invariants_route(self, constructor):
        """The arguments of ``kh_chi_local_invariants`` for ``constructor`` (a ``PerfectEntanglerChi`` /
        ``LocalInvariantsChi``) when the batch forms its co-states on the device -- Hilbert space, one gate (K_r = 4) per
        replica --, else None with the reason logged: the object is then called on the host, replica by replica."""
        reason = args = None
        if self.is_super:
            reason = "super-operators"
        elif self.Kr != 4:
            reason = "%d objectives per problem, not one gate of 4" % self.Kr
        else:
            for r in self.reps:
                constructor.check_objectives(self.Kr, r.objectives)  # (ValueError, as the host call would raise)
            layout = layout_of(self.reps[0].objectives, self.propagator)
            args = constructor.device_arguments(lambda state: layout.vector(state, 0))
            if args is None:
                reason = "the canonical basis does not match the state dimension %d" % self.N
        if reason is not None:
            logging.getLogger('krotov').info("%s: co-states on the host (%s)", type(constructor).__name__, reason)
        return args

    def iterate(self, chi_T, chi_norms, chi_coef, chi_li=None):
        """One backward and one update sweep over the active replicas.  chi_coef = (c, d), (K,) each: the boundary
        co-states are formed on the device (kh_chi_boundary); chi_li: what :meth:`local_invariants_route` returned
        (kh_chi_local_invariants, one gate per replica; the J per replica is left in ``self.li_J``); else chi_T (K, N)
        normalised, chi_norms (K,), host."""
        t, eng = self.torch, self.engine
        guess = self._pulses('pulses', 'guess_pulses')
        shapes = self._pulses('shapes', 'shape_arrays')
        lambdas = self._uploads.get('lambdas', np.array([np.asarray(r.lambda_vals, dtype=np.float64) for r in self.reps]))
        if chi_li is not None:
            mode, bell, invariants, weight = chi_li
            if self.li_out is None:  # (persistent: a frozen replica's slices keep their last values)
                self.li_out = (t.zeros((self.K, self.N), dtype=t.complex128, device=eng.device),
                               t.zeros((self.K,), dtype=t.float64, device=eng.device),
                               t.zeros((self.B,), dtype=t.float64, device=eng.device))
            self.set_active()
            chi_loc, norms_loc, self.li_J = eng.chi_local_invariants(
                self.psi_T, self._uploads.get('li_bell', bell, t.complex128), mode,
                self._uploads.get('li_invariants', invariants), weight, 1.0, out=self.li_out)
        elif chi_coef is not None:
            c_dev = self._uploads.get('chi_c', np.ascontiguousarray(chi_coef[0], dtype=np.complex128), t.complex128)
            d_dev = self._uploads.get('chi_d', np.ascontiguousarray(chi_coef[1], dtype=np.complex128), t.complex128)
            chi_loc, norms_loc = eng.chi_boundary(self.targets, self.psi_T, c_dev, d_dev)
        else:
            chi_loc = eng.dev(chi_T, t.complex128)
            norms_loc = eng.dev(np.asarray(chi_norms, dtype=np.float64), t.float64)
        if self.second_order:
            # sigma_b at replica b's own interval mid-points (optimize.py:451-452), the active replicas, one upload
            # (the mid-points once per replica, as an array: the same values as the scalar expression, element by element)
            for b, r in enumerate(self.reps):
                if r.active:
                    if r.midpoints is None:
                        tl = np.asarray(r.tlist)
                        r.midpoints = tl[:-1] + 0.5 * (tl[1:] - tl[:-1])
                    self.sigma_host[b] = [r.sigma(t) for t in r.midpoints]
            eng.set_second_order_replicas(self.fw_prev, self.fw_next, self.sigma_host)
        self.last_chi = (chi_loc, norms_loc)
        self.set_active()
        eng.backward(chi_loc, guess, out=self.chi_store)
        # (the update sweep reads init and the boundary states' buffer is its own: psi_T may be written in place)
        eng.forward_update(self.chi_store, norms_loc, self.init, guess, shapes, lambdas, out=(self.opt, self.psi_T, self.g_a))
        eng.check()
        opt_host = self.opt.cpu().numpy()
        self._uploads.record('pulses', opt_host, self.opt.clone())  # (the next guess of the replicas that go on)
        return opt_host, self.psi_T.cpu().numpy(), self.g_a.cpu().numpy()


def _run_batch(reps, propagator, chi_constructor, first=0):
    """One (sub-)batch on one replica engine; ``first``: the index of ``reps[0]`` among the caller's problems."""
    logger = logging.getLogger('krotov')
    li_object = isinstance(chi_constructor, _functionals._LocalInvariantsFunctional)
    second_order = reps[0].sigma is not None
    backend = _ReplicaBackend(reps, propagator, second_order=second_order)
    Kr = backend.Kr

    def states_of(psi_host, b):
        return _opt._LazyStates(psi_host[b * Kr:(b + 1) * Kr], reps[b].likes)

    def taus_of(tau, b):
        return np.array([None] * Kr) if tau is None else tau[b]

    # ---- iteration 0: forward propagation under the guess (optimize.py:295-322), all replicas in one sweep
    tic = time.time()
    psi_host = backend.initial_forward()
    tau = backend.tau_vals()
    toc = time.time()
    for b, r in enumerate(reps):
        r.fw_states_T = states_of(psi_host, b)
        r.tau_vals = taus_of(tau, b)
        if second_order:  # (in iteration 0 the states under "optimized" and guess pulses coincide)
            r.forward_states0 = backend.trajectories(backend.fw_prev, b, r.likes, psi_host)
        r.record_initial(r.guess_controls, r.pulses_mapping, r.guess_pulses, r.optimized_pulses, r.g_a_integrals,
                         r.fw_states_T, r.tau_vals, r.forward_states0, tic, toc)
        r.iteration = r.iter_start
        if not r.verdict(r.iteration):  # (an empty loop)
            r.stop()

    # the perfect-entangler / local-invariants functional itself (not a function wrapping it): co-states on the device
    chi_li = None
    if li_object:
        chi_li = backend.local_invariants_route(chi_constructor)

    # ---- main loop (optimize.py:392-581): one iteration of every active replica per pass
    while any(r.active for r in reps):
        tic = time.time()
        coefs = None
        if chi_li is None and backend.targets is not None:
            coefs = [_functionals.chi_coefficients(chi_constructor, r.weights, r.tau_vals, Kr) for r in reps]
            if any(c is None for c in coefs):
                coefs = None
        chi_T = chi_norms = chi_coef = None
        host_chis = {}  # (second order, a user's chi_constructor: what sigma.refresh gets, per replica)
        if chi_li is not None:
            pass
        elif coefs is not None:
            chi_coef = (np.concatenate([c[0] for c in coefs]), np.concatenate([c[1] for c in coefs]))
        else:  # a user's chi_constructor: on the host, per replica, as optimize_pulses does
            chi_T = np.zeros((backend.K, backend.N), dtype=np.complex128)
            chi_norms = np.ones(backend.K)
            layout = layout_of(reps[0].objectives, propagator)
            for b, r in enumerate(reps):
                if not r.active:
                    continue
                chis, norms, vecs = host_costates(chi_constructor, default_norm, layout.vector, fw_states_T=r.fw_states_T,
                                                  objectives=r.objectives, tau_vals=r.tau_vals)
                if li_object:  # (the object itself on the host: it has just left this problem's J in .values)
                    r.li_values = np.array(chi_constructor.values, dtype=np.float64)
                chi_T[b * Kr:(b + 1) * Kr] = np.array(vecs)
                chi_norms[b * Kr:(b + 1) * Kr] = norms
                host_chis[b] = (chis, norms)
        opt_host, psi_host, g_a = backend.iterate(chi_T, chi_norms, chi_coef, chi_li=chi_li)
        if chi_li is not None:  # (a singular U_B of an active replica: ValueError)
            chi_constructor.set_device_values(backend.li_J.cpu().numpy(), active=[r.active for r in reps])
            for b, r in enumerate(reps):  # (one gate per replica; a frozen one keeps the J of its last co-states)
                if r.active:
                    r.li_values = chi_constructor.values[b:b + 1].copy()
        tau = backend.tau_vals()
        toc = time.time()
        chi_fetched = None

        for b, r in enumerate(reps):
            if not r.active:
                continue
            r.iteration += 1
            logger.info("Finished Krotov iteration %d of problem %d", r.iteration, first + b)
            r.optimized_pulses = [opt_host[b, l].copy() for l in range(r.L)]
            r.fw_states_T = states_of(psi_host, b)
            r.g_a_integrals[:] = g_a[b]
            r.tau_vals = taus_of(tau, b)
            forward_states = None
            if second_order:
                forward_states = backend.trajectories(backend.fw_next, b, r.likes, psi_host)
            backward_states = None
            if r.info_hook is not None:
                backward_states = _opt._DeviceTrajectories(backend.chi_store[b * Kr:(b + 1) * Kr], r.likes)
            r.record_iteration(r.iteration, backward_states, forward_states, r.forward_states0, r.fw_states_T,
                               r.guess_pulses, r.optimized_pulses, r.g_a_integrals, r.tau_vals, tic, toc)
            if not r.verdict(r.iteration, r.convergence()):
                r.stop()
                continue
            r.guess_pulses = r.optimized_pulses
            if second_order:  # (optimize.py:566-577, for the replicas that go on)
                if b in host_chis:
                    chi_states, norms = host_chis[b]
                else:  # co-states formed on the device, in the caller's state type
                    if chi_fetched is None:
                        chi_fetched = backend.chi_host()
                    rows = slice(b * Kr, (b + 1) * Kr)
                    chi_states, norms = _opt._LazyStates(chi_fetched[0][rows], r.likes), chi_fetched[1][rows]
                r.sigma.refresh(
                    forward_states=forward_states, forward_states0=r.forward_states0, chi_states=chi_states,
                    chi_norms=norms, optimized_pulses=r.optimized_pulses, guess_pulses=r.guess_pulses,
                    objectives=r.objectives, result=r.result,
                )
                r.forward_states0 = forward_states
        if second_order:
            backend.advance_second_order()
    backend.engine.close()


def optimize_pulses_batch(problems, *, propagator, chi_constructor, iter_stop=5000, check_convergence=None,
                          info_hook=None, modify_params_after_iter=None, store_all_pulses=False, continue_from=None,
                          sigma=None):
    """Optimise B independent problems (*replicas*) as one batch on the device.

    ``problems``: a sequence of B mappings with the keys ``objectives``, ``pulse_options`` and ``tlist`` -- the first
    three arguments of :func:`~krotov_amd.optimize.optimize_pulses`; the keywords are shared by all of them
    (``continue_from``: None or a list of B ``Result`` s).  Returns a list of B ``Result`` s: ``results[b]`` is what
    ``optimize_pulses(**problems[b], <the shared keywords>)`` returns (``iters``, ``tau_vals``, ``info_vals``,
    ``all_pulses``, ``optimized_controls``, ``guess_controls``, ``controls_mapping``, ``states``, ``message``; the
    wall-clock fields aside), and ``info_hook`` / ``modify_params_after_iter`` are called once per replica and
    iteration with that replica's own keyword arguments (its ``lambda_vals``, ``shape_arrays`` and ``iter_stop`` may be
    changed in place, as today).

    Replicas of one shape -- the same number of objectives (at most 8), dimension (N <= 16), number of controls (1..4),
    grid length and kind, dense operators, ``propagator`` :func:`~krotov_amd.propagators.expm` /
    :class:`~krotov_amd.propagators.HipExpm` -- run on one replica engine (``"replica16/wave"``): one ``kh_tau``, one
    ``kh_chi_boundary``, one backward and one update sweep per iteration of the whole batch.  ``check_convergence`` and
    each replica's ``iter_stop`` decide per replica; a finished replica is frozen (the engine's active mask) and its
    ``Result`` is not touched again; the batch ends when no replica is active.  ``sigma``: None, or a sequence of B
    :class:`~krotov_amd.second_order.Sigma` objects -- the second-order update, replica b under ``sigma[b]``
    (``static_args['sigma']`` of its hooks), which is refreshed after every iteration that replica goes on from;
    ``info_hook`` then gets ``forward_states`` / ``forward_states0`` of its replica.  ``chi_constructor``: one of the four
    built-in functionals, a :class:`~krotov_amd.functionals.PerfectEntanglerChi` /
    :class:`~krotov_amd.functionals.LocalInvariantsChi` object (problems of one gate, 4 objectives: the co-states of the
    whole batch in one ``kh_chi_local_invariants`` launch, ``.values[b]`` the functional of problem b) -- or any callable,
    which is called on the host, problem by problem.  Under such an object, AFTER THE CALL RETURNS ``.values`` holds the
    J of every gate of every problem in problem order -- of each problem's last construction of the co-states, a problem
    that stopped early included (NaN for one that ran no iteration) --, whichever way the batch ran: as one batch, in
    sub-batches or one problem after another; entry b is what ``optimize_pulses`` on problem b alone leaves.  WHILE A
    SPLIT OR SEQUENTIAL BATCH IS STILL RUNNING, a hook sees in ``.values`` the running part only: the sub-batch's
    problems, or the one problem of the sequential loop.  A batch whose co-state store
    (B K_r nt N 16 bytes; with ``sigma`` three such stores: chi and the two forward trajectories) exceeds a quarter of
    the free device memory is split into consecutive sub-batches of equal size.  Everything else runs the replicas one
    after another through ``optimize_pulses`` (logged once as ``"optimize_pulses_batch: sequential (<reason>)"`` on the
    ``krotov`` logger)."""
    logger = logging.getLogger('krotov')
    problems = [dict(p) for p in problems]
    B = len(problems)
    if continue_from is not None and len(continue_from) != B:
        raise ValueError("continue_from must be None or a list of one Result per problem")
    previous = [None] * B if continue_from is None else list(continue_from)
    if sigma is not None:
        sigma = list(sigma)
        if len(sigma) != B or any(s is None for s in sigma):
            raise ValueError("sigma must be None or a sequence of one Sigma per problem")
    sigmas = [None] * B if sigma is None else sigma
    if B == 0:
        return []

    li_object = isinstance(chi_constructor, _functionals._LocalInvariantsFunctional)

    def publish_values(per_problem):
        """``.values`` of a ``PerfectEntanglerChi`` / ``LocalInvariantsChi`` object over the whole batch: every
        problem's J per gate in problem order (NaN for a problem that formed no co-states)."""
        if li_object and any(v is not None for v in per_problem):
            chi_constructor.values = np.concatenate([
                np.full(len(p['objectives']) // 4, np.nan) if v is None else np.asarray(v, dtype=np.float64)
                for p, v in zip(problems, per_problem)])

    def sequential(reason):
        logger.info("optimize_pulses_batch: sequential (%s)", reason)
        results, values = [], []
        before = chi_constructor.values if li_object else None
        for p, prev, sig in zip(problems, previous, sigmas):
            if li_object:  # (every call leaves its own problem's J there: collected, published together at the end)
                chi_constructor.values = None
            results.append(_opt.optimize_pulses(
                p['objectives'], p['pulse_options'], p['tlist'], propagator=propagator, chi_constructor=chi_constructor,
                iter_stop=iter_stop, check_convergence=check_convergence, info_hook=info_hook,
                modify_params_after_iter=modify_params_after_iter, store_all_pulses=store_all_pulses, continue_from=prev,
                sigma=sig))
            values.append(None if not li_object or chi_constructor.values is None else np.array(chi_constructor.values))
        if li_object:
            chi_constructor.values = before  # (it stays what it was where no problem formed co-states)
        publish_values(values)
        return results

    if isinstance(propagator, list) or not (propagator is expm or isinstance(propagator, HipExpm)):
        return sequential("the propagator is not expm / HipExpm")
    hook = chained_hook(modify_params_after_iter, info_hook)
    reps = [_Replica(p, propagator, chi_constructor, iter_stop, store_all_pulses, prev, sigma=sig, info_hook=hook,
                     check_convergence=check_convergence)
            for p, prev, sig in zip(problems, previous, sigmas)]
    reason = _batch_obstacle(problems, reps, propagator)
    if reason is not None:
        return sequential(reason)
    logger.info("optimize_pulses_batch: %d problems of %d objectives in one batch", B, len(reps[0].objectives))

    # the co-state store of the whole batch (second order: and the two forward trajectories) against a quarter of the
    # free device memory
    size = B
    free = _free_device_bytes()
    if free is not None:
        per_replica = len(reps[0].objectives) * len(reps[0].tlist) * layout_of(reps[0].objectives, propagator).stride * 16
        if sigma is not None:
            per_replica *= 3  # chi, phi_prev, phi_next
        while size > 1 and (B % size != 0 or size * per_replica > free // 4):
            size -= 1
        if size < B:
            logger.info("optimize_pulses_batch: %d sub-batches of %d problems (the co-state store of all %d would take "
                        "%d bytes, a quarter of the free device memory is %d)", B // size, size, B, B * per_replica, free // 4)
    for i in range(0, B, size):
        _run_batch(reps[i:i + size], propagator, chi_constructor, first=i)
    publish_values([r.li_values for r in reps])
    return [r.result for r in reps]
