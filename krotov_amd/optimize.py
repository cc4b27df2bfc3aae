"""``optimize_pulses``: Krotov's method behind the reference's plugin surface.

Same signature, keyword semantics, error behaviour and ``Result`` as
``krotov.optimize_pulses`` (reference src/krotov/optimize.py:33-590).  Two
execution paths share all bookkeeping:

* **device path** -- taken when ``propagator`` is this package's
  :func:`krotov_amd.propagators.expm` / :class:`~krotov_amd.propagators.HipExpm`
  and ``mu``, ``overlap``, ``storage`` are the defaults (first- or second-order
  update).  Per
  iteration the three objective-parallel dispatches of the reference
  (optimize.py:302-313, 413-425, 449-501) become three calls into
  ``libkrotov_hip.so``: all objectives are batched in one launch per sweep,
  the co-states never leave HBM, and the K*L*(nt-1) Python ``mu``/``overlap``
  calls of optimize.py:454-470 disappear into the kernel.  Objectives can be
  sharded over the GPUs of a node with ``process_group=`` (one rank per GPU,
  one all-reduce of the L update sums per interval).

* **plugin path** -- any other ``propagator`` (a user's own callable, in
  whatever arithmetic it implements) runs through a host loop with the
  reference's call structure, so custom ``propagator`` / ``mu`` / ``overlap`` /
  ``norm`` / ``parallel_map`` / ``storage`` plugins keep working.  This path
  does no arithmetic of its own.

There is no CPU fallback for the device path: without a GPU or without the
built library, requesting it raises.
"""
import copy
import inspect
import logging
import os
import time
from functools import partial

import numpy as np

from . import _run
from . import functionals as _functionals
from ._ingest import state_to_vector, to_dense, to_sparse, vector_to_state
from .constraints import QuadraticStateConstraint, StateDependentConstraint
from .conversions import (
    control_onto_interval,
    discretize,
    extract_controls,
    extract_controls_mapping,
    plug_in_pulse_values,
    pulse_onto_tlist,
    pulse_options_dict_to_list,
)
from ._lib import KrotovHipError as _KrotovHipError
from ._lib import KH_ERR_TIMEOUT as _KH_ERR_TIMEOUT
from ._update_ladder import UpdateLadder as _UpdateLadder, leave_row_split as _leave_row_split

_KH_MAX_CONTROLS = 32  # KH_GEN_MAX_L of krotov_amd/csrc/kh_common.h (the register-resident kernel families: 8)
from .mixed import Layout, LindbladLayout, layout_of, lindblad_layout_of
from .mu import derivative_wrt_pulse
from .nonlinear import has_control_function, term_plan
from .parallelization import serial_map
from .parametrization import Parametrization, PulseParameters
from .propagators import HipExpm, LindbladExpm, Propagator, expm
from .result import Result
from .second_order import _overlap
from .shapes import one_shape, zero_shape
from .sharding import gather_rows, shard_range

__all__ = ['optimize_pulses']


# ---------------------------------------------------------------------------
# control initialisation (reference optimize.py:593-704)
# ---------------------------------------------------------------------------


def _shape_callable(val):
    if callable(val):
        return val
    if val == 1:
        return one_shape
    if val == 0:
        return zero_shape
    raise ValueError("update_shape must be a callable")


def _checked_shape(arr):
    """Shapes must lie in [0, 1] up to the rounding of the un-averaging; then
    clip (reference optimize.py:605-620)."""
    lo, hi = np.min(arr), np.max(arr)
    if lo < -0.01 or hi > 1.01:
        raise ValueError(
            "Update shapes ('update_shape' in pulse options-dict) must have "
            "values in the range [0, 1], not [%s, %s]" % (lo, hi)
        )
    return np.clip(arr, a_min=0.0, a_max=1.0)


def _initialize_krotov_controls(objectives, pulse_options, tlist):
    guess_controls = extract_controls(objectives)
    pulses_mapping = extract_controls_mapping(objectives, guess_controls)
    options_list = pulse_options_dict_to_list(pulse_options, guess_controls)
    try:
        guess_controls = [
            discretize(c, tlist, args=(options_list[i].get('args', None),), via_midpoints=True)
            for i, c in enumerate(guess_controls)
        ]
    except TypeError as exc:
        raise ValueError(
            "Cannot discretize controls: %s. Note that "
            "all controls must be real-valued. Complex controls must be "
            "split into an independent real and imaginary part in the "
            "objectives before passing them to the optimization" % exc
        )
    guess_pulses = [control_onto_interval(c) for c in guess_controls]
    try:
        lambda_vals = np.array([float(o['lambda_a']) for o in options_list])
    except KeyError:
        raise ValueError("Each value in pulse_options must be a dict that contains the key 'lambda_a'.")
    shape_arrays = []
    for o in options_list:
        try:
            S = discretize(_shape_callable(o['update_shape']), tlist, args=(), via_midpoints=True)
        except KeyError:
            raise ValueError("Each value in pulse_options must be a dict that contains the key 'update_shape'.")
        except TypeError as exc:
            raise ValueError(
                "Update shapes ('update_shape' in pulse options-dict) must be real-valued: %s" % exc
            )
        shape_arrays.append(_checked_shape(control_onto_interval(S)))
    return guess_controls, guess_pulses, pulses_mapping, lambda_vals, shape_arrays


def _parametrizations(objectives, pulse_options):
    """``pulse_options[ctrl]['parametrization']`` per control, in the controls' order (None: the control is its own
    parameter), or None when no control has one."""
    options_list = pulse_options_dict_to_list(pulse_options, extract_controls(objectives))
    params = [o.get('parametrization', None) for o in options_list]
    for l, par in enumerate(params):
        if par is not None and not isinstance(par, Parametrization):
            raise ValueError("control %d: 'parametrization' in pulse_options must be a krotov_amd.parametrization."
                             "Parametrization, not %r" % (l, par))
    return params if any(par is not None for par in params) else None


def _restore_from_previous_result(result, objectives, tlist, store_all_pulses):
    """Guess controls/pulses of a continued optimisation (reference
    optimize.py:707-774), with the same compatibility checks."""
    if not isinstance(result, Result):
        raise ValueError("Continuation is only possible from a Result object")
    if len(objectives) != len(result.objectives):
        raise ValueError("When continuing from a previous Result, the number of objectives must be the same")
    for a, b in zip(objectives, result.objectives):
        if a != b:
            raise ValueError("When continuing from a previous Result, the objectives must remain unchanged")
    if store_all_pulses and len(result.all_pulses) == 0:
        raise ValueError(
            "The store_all_pulses parameter cannot be changed when continuing from a previous Result. "
            "Pass it as False."
        )
    if not store_all_pulses and len(result.all_pulses) > 0:
        raise ValueError(
            "The store_all_pulses parameter cannot be changed when continuing from a previous Result. "
            "Pass it as True."
        )
    same_grid = len(tlist) == len(result.tlist) and np.max(np.abs(np.array(tlist) - np.array(result.tlist))) <= 1e-5
    if not same_grid:
        raise ValueError("When continuing from a previous Result, the controls must be defined on the same time grid")
    nt = len(tlist)
    guess_controls = []
    for control in result.optimized_controls:
        if len(control) == nt - 1:  # dumped mid-optimisation: these are pulses
            guess_controls.append(pulse_onto_tlist(control))
        elif len(control) == nt:
            guess_controls.append(control)
        else:
            raise ValueError("Invalid Result: optimized_controls and tlist are incongruent")
    return guess_controls, [control_onto_interval(c) for c in guess_controls]


def _check_propagators_interface(propagators, logger):
    """Warn about propagators whose signature is neither ``expm``'s nor
    ``Propagator.__call__``'s (reference optimize.py:623-638)."""
    ok = (inspect.getfullargspec(expm), inspect.getfullargspec(Propagator.__call__))
    for p in propagators:
        try:
            spec = inspect.getfullargspec(p)
        except TypeError:
            spec = None
        if spec not in ok:
            logger.warning("The propagator %s does not have the expected interface.", p)


# ---------------------------------------------------------------------------
# plugin path: the reference's call structure around user callables
# ---------------------------------------------------------------------------


def _forward_propagation(i_objective, objectives, pulses, pulses_mapping, tlist, propagators, storage,
                         store_all=True):
    """Task for ``parallel_map[0]`` (reference optimize.py:806-846)."""
    obj = objectives[i_objective]
    state = obj.initial_state
    mapping = pulses_mapping[i_objective]
    out = None
    if store_all:
        out = storage(len(tlist))
        out[0] = state
    for n in range(len(tlist) - 1):
        H = plug_in_pulse_values(obj.H, pulses, mapping[0], n)
        c_ops = [plug_in_pulse_values(c, pulses, mapping[ic + 1], n) for ic, c in enumerate(obj.c_ops)]
        state = propagators[i_objective](H, state, tlist[n + 1] - tlist[n], c_ops, initialize=(n == 0))
        if store_all:
            out[n + 1] = state
    return out if store_all else state


def _backward_propagation(i_state, chi_states, adjoint_objectives, pulses, pulses_mapping, tlist, propagators,
                          storage):
    """Task for ``parallel_map[1]`` (reference optimize.py:849-886)."""
    state = chi_states[i_state]
    obj = adjoint_objectives[i_state]
    mapping = pulses_mapping[i_state]
    nt = len(tlist)
    out = storage(nt)
    out[-1] = state
    for n in range(nt - 2, -1, -1):
        H = plug_in_pulse_values(obj.H, pulses, mapping[0], n, conjugate=True)
        c_ops = [plug_in_pulse_values(c, pulses, mapping[ic + 1], n) for ic, c in enumerate(obj.c_ops)]
        state = propagators[i_state](
            H, state, tlist[n + 1] - tlist[n], c_ops, backwards=True, initialize=(n == nt - 2)
        )
        out[n] = state
    return out


def _backward_propagation_source(i_state, chi_states, adjoint_objectives, pulses, pulses_mapping, tlist, propagators,
                                 storage, source, chi_norms):
    """:func:`_backward_propagation` with a source term (state-dependent constraints, krotov_amd.constraints):
    ``chi[n] = V_n (chi[n+1] + h W[n+1]) + h W[n]`` with ``h = dt_n / 2 / ||chi(T)||``, V_n the propagator's own step."""
    state = chi_states[i_state]
    obj = adjoint_objectives[i_state]
    mapping = pulses_mapping[i_state]
    nt = len(tlist)
    out = storage(nt)
    out[-1] = state
    for n in range(nt - 2, -1, -1):
        dt = tlist[n + 1] - tlist[n]
        h = 0.5 * dt / chi_norms[i_state]
        H = plug_in_pulse_values(obj.H, pulses, mapping[0], n, conjugate=True)
        c_ops = [plug_in_pulse_values(c, pulses, mapping[ic + 1], n) for ic, c in enumerate(obj.c_ops)]
        state = state + h * vector_to_state(source[i_state, n + 1], state)
        state = propagators[i_state](H, state, dt, c_ops, backwards=True, initialize=(n == nt - 2))
        state = state + h * vector_to_state(source[i_state, n], state)
        out[n] = state
    return out


def _forward_propagation_step(i_state, states, objectives, pulses, pulses_mapping, tlist, time_index, propagators):
    """Task for ``parallel_map[2]`` (reference optimize.py:889-911)."""
    obj = objectives[i_state]
    mapping = pulses_mapping[i_state]
    H = plug_in_pulse_values(obj.H, pulses, mapping[0], time_index)
    c_ops = [plug_in_pulse_values(c, pulses, mapping[ic + 1], time_index) for ic, c in enumerate(obj.c_ops)]
    dt = tlist[time_index + 1] - tlist[time_index]
    return propagators[i_state](H, states[i_state], dt, c_ops, initialize=(time_index == 0))


class _PluginBackend:
    """Host loop over user callables, call-for-call like the reference."""

    def __init__(self, objectives, adjoint_objectives, pulses_mapping, tlist, propagators, storage, parallel_map,
                 mu, overlap):
        self.objectives = objectives
        self.adjoint_objectives = adjoint_objectives
        self.mapping = pulses_mapping
        self.tlist = tlist
        self.propagators = propagators
        self.storage = storage
        self.pmap = parallel_map
        self.mu = mu
        self.overlap = overlap

    def initial_forward(self, pulses, store=False):
        """(``store``: the trajectories are kept whether or not the caller goes on to use them.)"""
        K = len(self.objectives)
        forward_states = self.pmap[0](
            _forward_propagation, list(range(K)),
            (self.objectives, pulses, self.mapping, self.tlist, self.propagators, self.storage),
        )
        return [s[-1] for s in forward_states], forward_states

    def tau_vals(self, fw_states_T):
        return np.array([self.overlap(obj.target, s) for s, obj in zip(fw_states_T, self.objectives)])

    def state_vector(self, state, k):
        """The user's callables take the states as they are."""
        return state

    def advance_second_order(self):
        """``forward_states0`` is the caller's here: nothing to swap."""

    def iterate(self, chi_states, chi_norms, guess_pulses, lambda_vals, shape_arrays, sigma=None, forward_states0=None,
                chi_coef=None, par=None, constraint=None, chi_li=None):
        """``_HipBackend.iterate``'s signature; ``chi_coef`` / ``chi_li`` (co-states formed on the device) never come here."""
        objectives, tlist = self.objectives, self.tlist
        K, nt = len(objectives), len(tlist)
        if constraint is not None:
            # state-dependent constraint: the source on the states under the guess pulses drives the co-states
            source = np.asarray(constraint.source(forward_states0, tlist), dtype=np.complex128)
            backward_states = self.pmap[1](
                _backward_propagation_source, list(range(K)),
                (chi_states, self.adjoint_objectives, guess_pulses, self.mapping, tlist, self.propagators, self.storage,
                 source, chi_norms),
            )
        else:
            backward_states = self.pmap[1](
                _backward_propagation, list(range(K)),
                (chi_states, self.adjoint_objectives, guess_pulses, self.mapping, tlist, self.propagators, self.storage),
            )
        g_a = np.zeros(len(guess_pulses))
        optimized = copy.deepcopy(guess_pulses)
        if par is not None:  # pulse parametrizations: u is updated, the interval is propagated with f(u)
            dfdu = par.dfdu()
            u_new = [np.array(u, dtype=np.float64) for u in par.u]
        fw_states = [obj.initial_state for obj in objectives]
        forward_states = moved = None
        if sigma is not None or constraint is not None:
            # second order: keep phi(t_n) and phi(t_n) - phi_prev(t_n) (optimize.py:429-442); a state-dependent
            # constraint needs phi(t_n) for the next iteration's source
            forward_states = [self.storage(nt) for _ in range(K)]
            for k in range(K):
                forward_states[k][0] = objectives[k].initial_state
        if sigma is not None:
            moved = [fw_states[k] - forward_states0[k][0] for k in range(K)]  # zero at t=0
        for n in range(nt - 1):
            dt = tlist[n + 1] - tlist[n]
            if sigma is not None:
                half_sigma = 0.5 * sigma(tlist[n] + 0.5 * dt)
            for l in range(len(guess_pulses)):
                total = 0j
                for k in range(K):  # optimize.py:455-470
                    mu_op = self.mu(objectives, k, guess_pulses, self.mapping, l, n)
                    mu_phi = mu_op(fw_states[k])
                    update = self.overlap(backward_states[k][n], mu_phi)
                    update *= chi_norms[k]
                    if sigma is not None:
                        update += half_sigma * self.overlap(moved[k], mu_phi)
                    total += update
                step = shape_arrays[l][n] / lambda_vals[l]
                d1 = total.imag
                if par is not None:
                    d1 = dfdu[l][n] * d1  # dH/du = f'(u_guess) dH/d eps
                    u_new[l][n] = par.u[l][n] + step * d1
                    g_a[l] += step * abs(d1) ** 2 * dt
                    optimized[l][n] = par.eps(l, u_new[l][n])
                    continue
                g_a[l] += step * abs(d1) ** 2 * dt
                optimized[l][n] += step * d1
            fw_states = self.pmap[2](
                _forward_propagation_step, list(range(K)),
                (fw_states, objectives, optimized, self.mapping, tlist, n, self.propagators),
            )
            if sigma is not None:
                moved = [fw_states[k] - forward_states0[k][n + 1] for k in range(K)]
            if forward_states is not None:
                for k in range(K):
                    forward_states[k][n + 1] = fw_states[k]
        if par is not None:
            par.commit(u_new, optimized)
        return backward_states, optimized, fw_states, g_a, forward_states


# ---------------------------------------------------------------------------
# device path
# ---------------------------------------------------------------------------


class _LazyStates:
    """List-like view of per-objective states held as one (K, N) array -- on the
    host, or still on the device and fetched on first access (``fetch``);
    elements are converted to the caller's state type on access."""

    def __init__(self, array, likes, fetch=None, layout=None):
        self._host = array
        self._fetch = fetch
        self._likes = likes
        self._layout = layout  # (mixed objective lists: rows at the stride, sliced back to N_k)

    @property
    def _array(self):
        if self._host is None:
            self._host = self._fetch()
            self._fetch = None
        return self._host

    def __len__(self):
        return len(self._likes)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        if self._layout is not None:
            return self._layout.state(self._array[k], k, self._likes[k])
        return vector_to_state(self._array[k], self._likes[k])

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def __reduce__(self):
        # pickled (Result.dump from a check_convergence hook, copy.deepcopy) as the plain list of states
        # it stands for: the fetch closure holds device tensors and must not travel
        return (list, (list(self),))


class _DeviceTrajectory:
    """States of one objective on the time grid, one device row per access."""

    def __init__(self, owner, k):
        self._o, self._k = owner, k

    def __len__(self):
        return self._o._t.shape[1]

    def __getitem__(self, n):
        o, k = self._o, self._k
        nt = len(self)
        if isinstance(n, slice):
            return [self[i] for i in range(*n.indices(nt))]
        if not -nt <= n < nt:
            raise IndexError("time index %d out of range" % n)
        n %= nt
        like = o._likes[k]
        if n == nt - 1 and o._final is not None:
            return o._state(o._final[k], k, like)
        if not o._k0 <= k < o._k0 + o._t.shape[0]:
            raise IndexError("objective %d lives on another rank; only its final state is available here" % k)
        return o._state(o._t[k - o._k0, n].cpu().numpy(), k, like)

    def __iter__(self):
        return (self[n] for n in range(len(self)))


class _DeviceTrajectories:
    """``backward_states[k][n]`` / ``forward_states[k][n]`` for ``info_hook`` and
    ``sigma.refresh``: (K_loc, nt, N) in HBM, fetched on access.  ``final``: the
    states at T of all objectives of all ranks on the host, if known."""

    def __init__(self, tensor, likes, k0=0, final=None, layout=None, engine=None):
        self._t, self._likes, self._k0, self._final = tensor, likes, k0, final
        self._layout = layout  # (mixed objective lists: rows at the stride, sliced back to N_k)
        self._engine = engine  # (krotov_amd.constraints: expectation values of the trajectory on the device)

    def _state(self, row, k, like):
        if self._layout is not None:
            return self._layout.state(row, k, like)
        return vector_to_state(row, like)

    def __len__(self):
        return len(self._likes) if self._final is not None else self._t.shape[0]

    def __getitem__(self, k):
        if self._final is None:
            k += self._k0  # local numbering (backward states of this rank)
        if not 0 <= k < len(self._likes):
            raise IndexError("objective index out of range")
        return _DeviceTrajectory(self, k)

    def __iter__(self):
        return (self[k] for k in range(len(self)))


def _use_device_path(propagator, mu, overlap, sigma, storage, objectives):
    if isinstance(propagator, list):
        if not propagator or any(not (p is expm or isinstance(p, HipExpm)) for p in propagator):
            return False
    elif not (propagator is expm or isinstance(propagator, HipExpm)):
        return False
    if mu is not None and mu is not derivative_wrt_pulse:
        return False
    if overlap is not None and overlap is not _overlap:
        return False
    if storage != 'array':
        return False
    if all(len(obj.c_ops) == 0 for obj in objectives):
        return True
    # objectives in Lindblad form (H + c_ops): only with the propagator that opts in
    props = propagator if isinstance(propagator, list) else [propagator]
    return all(isinstance(p, LindbladExpm) for p in props)


def _operator_rows(objectives, pulses_mapping, L, convert, k0=0, k1=None):
    """The engine's operator rows ``[H0, H_1 .. H_L]`` (``None``: the control does not occur) and Lindblad operators of
    objectives k0 .. k1 - 1, every distinct operator converted once: objectives sharing an operator share its copy."""
    dense = {}

    def dense_of(op):
        key = id(op)
        if key not in dense:
            dense[key] = (convert(op), op)
        return dense[key][0]

    sums = {}

    def summed(terms):
        """Dense sum of several operators, cached on their identities so
        objectives sharing the same nested list share one device copy."""
        if len(terms) == 1:
            return dense_of(terms[0])
        key = tuple(id(t) for t in terms)
        if key not in sums:
            total = dense_of(terms[0]).copy()
            for t in terms[1:]:
                total = total + dense_of(t)
            sums[key] = (total, terms)
        return sums[key][0]

    ops, c_rows = [], []
    for k in range(k0, len(objectives) if k1 is None else k1):
        obj = objectives[k]
        H = obj.H if isinstance(obj.H, list) else [obj.H]
        drift = [t for t in H if not isinstance(t, list)]
        row = [summed(drift)]
        for l in range(L):
            where = pulses_mapping[k][0][l]
            row.append(summed([H[i][0] for i in where]) if len(where) else None)
        ops.append(row)
        c_rows.append([dense_of(c) for c in obj.c_ops])
    return ops, c_rows


# the limits of the replica kernels (krotov_amd/csrc/kh_mini.h: KH_MINI_N, KH_MINI_MAXK; kh_replica.h: 1..4 controls)
REPLICA_NMAX, REPLICA_KMAX, REPLICA_LMAX = 16, 8, 4


def _replica_kind_obstacle(objectives, propagator):
    """Why the KIND of one problem does not fit a replica engine (a short reason), or None.  With
    ``_replica_size_obstacle``: what ``optimize_pulses_batch`` asks of every problem of a batch."""
    if isinstance(propagator, list) or not (propagator is expm or isinstance(propagator, HipExpm)):
        return "the propagator is not expm / HipExpm"
    if isinstance(propagator, LindbladExpm) or any(len(o.c_ops) > 0 for o in objectives):
        return "objectives with c_ops"
    if isinstance(propagator, HipExpm) and getattr(propagator, 'sparse', False):
        return "sparse propagator"
    if layout_of(objectives, propagator).mixed:
        return "objectives of mixed dimension or kind"
    return None


def _replica_size_obstacle(N, Kr, L):
    """Why a problem of dimension N with Kr objectives and L controls exceeds the replica kernels, or None."""
    if N > REPLICA_NMAX:
        return "N = %d > %d" % (N, REPLICA_NMAX)
    if Kr > REPLICA_KMAX:
        return "%d objectives per problem > %d" % (Kr, REPLICA_KMAX)
    if L < 1 or L > REPLICA_LMAX:
        return "%d controls (1..%d)" % (L, REPLICA_LMAX)
    return None


def _one_gate_replica_form(objectives, propagator, n_controls, chi_constructor, process_group, other_features):
    """Whether ``optimize_pulses`` runs this problem as a batch of one on a replica engine: one gate (4 Hilbert-space
    objectives) under a ``PerfectEntanglerChi`` / ``LocalInvariantsChi`` object, of a kind and size a replica engine
    takes, without parametrization, constraint, sharding or a skipped forward sweep
    (``other_features``).  These are the problems run from many guesses at once; on the same kernels a batch's
    ``results[b]`` is ``optimize_pulses(**problems[b])`` bit for bit (the one-wave kernels a problem of this size gets
    under any other constructor round differently in the last bit).  The price: the replica kernels are somewhat slower
    on a single problem."""
    if not isinstance(chi_constructor, _functionals._LocalInvariantsFunctional) or len(objectives) != 4:
        return False
    if process_group is not None or other_features or _replica_kind_obstacle(objectives, propagator) is not None:
        return False
    layout = layout_of(objectives, propagator)
    if layout.kinds[0]:  # (Liouville space: the co-states are not formed on the device)
        return False
    return _replica_size_obstacle(layout.stride, len(objectives), n_controls) is None


class _UploadCache:
    """Device copies of small host arrays that are usually the same from one iteration to the next (every upload from
    pageable memory blocks the host for ~30 us with the GPU idle)."""

    def __init__(self, engine, dtype):
        self.engine, self.dtype = engine, dtype  # (dtype: the one of an upload that names none)
        self._held = {}  # key -> (host array as uploaded, its device copy)

    def get(self, key, host, dtype=None):
        hit = self._held.get(key)
        if hit is not None and hit[0].shape == host.shape and np.array_equal(hit[0], host):
            return hit[1]
        dev = self.engine.dev(host, dtype if dtype is not None else self.dtype)
        self._held[key] = (host.copy(), dev)
        return dev

    def record(self, key, host, dev):
        """``dev`` is already the device copy of ``host`` (a sweep's output that was fetched): no upload if the caller
        comes back with the same values."""
        self._held[key] = (host.copy(), dev)


class _HipBackend:
    """All objectives of this rank resident on one GPU."""

    def __init__(self, objectives, pulses_mapping, tlist, n_controls, propagator, process_group=None,
                 second_order=False, parametrized=False, replica_form=False):
        import torch

        from .engine import HipKrotovEngine

        self.torch = torch
        self.group = process_group
        # replica_form: the problem as a batch of ONE on a replica engine (``_one_gate_replica_form``) -- the kernels
        # ``optimize_pulses_batch`` runs it on, so that a batch is, bit for bit, the loop over its problems
        self.replica_form = replica_form
        self.objectives = objectives
        K_total = len(objectives)
        self.rank, self.world = 0, 1
        if process_group is not None:
            import torch.distributed as dist

            self.dist = dist
            self.rank = dist.get_rank(process_group)
            self.world = dist.get_world_size(process_group)
        # contiguous shard of objectives for this rank
        self.k0, self.k1 = shard_range(K_total, self.world, self.rank)
        if K_total < self.world:
            # the same error on EVERY rank, before any collective (a lone raising rank would leave the
            # others hanging in the first all-gather)
            raise ValueError("%d objectives cannot be sharded over %d ranks" % (K_total, self.world))
        # every objective's dimension and kind (Hilbert / Liouville), decided per objective over the whole list (the
        # same on every rank)
        # objectives in Lindblad form (H + c_ops): the matrix-form engine, or -- outside its limits -- the Liouvillian
        # built on the host and today's engines (host-only decision)
        self.lindblad = None
        nonlinear = has_control_function(objectives, c_ops_too=False)
        if nonlinear and process_group is not None:
            raise ValueError("non-linear controls (ControlFunction) run on one GPU: process_group= (sharding) is not "
                             "supported with them")
        if any(len(obj.c_ops) > 0 for obj in objectives):
            lind = lindblad_layout_of(objectives, propagator, n_controls, second_order, parametrized, nonlinear)
            if lind.matrix:
                if process_group is not None:
                    raise ValueError("objectives in Lindblad form run on one GPU: process_group= (sharding) is not "
                                     "supported for the matrix-form engine")
                self.lindblad = lind
                logging.getLogger('krotov').info(
                    "Lindblad-form objectives: matrix-form engine (d = %d, up to %d Lindblad operators)", lind.d, lind.n_c)
            else:
                logging.getLogger('krotov').info("Lindblad-form objectives: Liouvillian fallback (%s)", lind.reason)
                objectives = LindbladLayout.liouvillian_objectives(objectives)
                self.objectives = objectives
        if self.lindblad is not None:
            layout = Layout([self.lindblad.d ** 2] * K_total, [True] * K_total)
        else:
            layout = layout_of(objectives, propagator)
        self.layout = layout if layout.mixed else None
        self.K_total = K_total
        L = n_controls
        # non-linear controls (krotov_amd.nonlinear): one operator slot per distinct (control, power) -- the engine's
        # plain, backward and source sweeps take the J rows of term coefficients eps_c^p, its update sweep the L rows
        # of eps and the weights p eps_guess^(p-1) (kh_set_nonlinear)
        self.nl = term_plan(objectives, pulses_mapping, n_controls) if nonlinear else None
        if self.nl is False:
            raise ValueError("a ControlFunction that is no integer power (power None) runs the host loop, not the "
                             "device's sweeps")
        op_mapping, n_slots = (pulses_mapping, L) if self.nl is None else (self.nl.mapping, self.nl.J)
        props = propagator if isinstance(propagator, list) else [propagator]
        # operators stay in CSR form on the device when the propagator asks for it
        # (DensityMatrixODEPropagator / HipExpm(sparse=True): large sparse Liouvillians)
        self.sparse = any(isinstance(p, HipExpm) and getattr(p, 'sparse', False) for p in props)
        ops, c_rows = _operator_rows(objectives, op_mapping, n_slots, to_sparse if self.sparse else to_dense,
                                     self.k0, self.k1)
        N = layout.stride
        self.is_super = layout.kinds[self.k0:self.k1] if layout.mixed else layout.kinds[self.k0]
        self.N, self.L = N, L
        tlist = np.asarray(tlist, dtype=np.float64)
        # (HipExpm(sparse=True, row_split=...) / DensityMatrixODEPropagator(row_split=...): an objective's rows on several workgroups)
        row_split = next((p.row_split for p in props if isinstance(p, HipExpm) and getattr(p, 'sparse', False)
                          and getattr(p, 'row_split', None) is not None), None)
        if self.lindblad is not None:
            self.engine = HipKrotovEngine(ops, np.diff(tlist), c_ops=c_rows)
        elif replica_form:
            self.engine = HipKrotovEngine(ops, np.diff(tlist)[None, :], is_super=self.is_super, replicas=1)
        elif row_split is not None:
            self.engine = HipKrotovEngine(ops, np.diff(tlist), is_super=self.is_super, row_split=row_split)
        else:
            self.engine = HipKrotovEngine(ops, np.diff(tlist), is_super=self.is_super)
        self.nt = len(tlist)
        self.tlist_host = tlist
        self.likes = [obj.initial_state for obj in objectives]
        init = [layout.vector(objectives[k].initial_state, k) for k in range(self.k0, self.k1)]
        if any(v is None for v in init):
            raise ValueError("initial states do not match the operator dimension %s" % (
                N if not layout.mixed else "of their objective (%s)" % layout.dims))
        self.init_host = np.array(init)
        self.init = self.engine.dev(self.init_host, torch.complex128)
        tg = [layout.vector(obj.target, k) for k, obj in enumerate(objectives)]
        self.targets_host = None if any(v is None for v in tg) else np.array(tg)
        self.targets = (
            None if self.targets_host is None
            else self.engine.dev(self.targets_host[self.k0:self.k1], torch.complex128)
        )
        w = [getattr(obj, 'weight', None) for obj in objectives]
        self.weights = None if all(x is None for x in w) else np.array([1.0 if x is None else x for x in w])
        self.chi_store = None
        self.fw_T_dev = None
        self.fw_prev = self.fw_next = None  # second order: phi(t_n) of the last / the running iteration
        self.last_chi = None
        self._uploads = _UploadCache(self.engine, torch.float64)
        if self.nl is not None:
            self._nl_rows = self.engine.dev(self.nl.term_control.astype(np.int64), torch.int64)
            self._nl_pow = self.engine.dev(self.nl.term_power.astype(np.float64)[:, None], torch.float64)
        self._src_store = None  # W_k(t_n) of a state-dependent constraint (_constraint_source)
        self._li_route = None  # (constructor, its device arguments or None): local_invariants_route, decided once
        self._ladder = _UpdateLadder(self.engine)  # (one GPU) the single-launch update sweep's retries
        # device-side exchange over peer-mapped windows (xGMI) when every rank can set it up;
        # otherwise (or after a failed sweep) one RCCL all-reduce per interval
        self._p2p_synced = False  # until the ranks have been lined up before the first peer-window sweep
        self.p2p = False
        self.engine.p2p_why = "KH_P2P=0" if self.world > 1 else None
        if self.world > 1 and os.environ.get('KH_P2P', '1') != '0':
            self.p2p = self.engine.enable_p2p(self.group)
            logging.getLogger('krotov').info(
                "cross-GPU exchange: %s", "peer windows" if self.p2p else "RCCL all-reduce per interval")

    # -- helpers -----------------------------------------------------------
    def _per_control(self):
        """Shape of the pulse-like arrays the engine takes: (L, nt - 1), on a replica engine (1, L, nt - 1)."""
        return (1, self.L, self.nt - 1) if self.replica_form else (self.L, self.nt - 1)

    def _pulses(self, pulses, cached=False):
        host = np.array(pulses, dtype=np.float64).reshape(self._per_control())
        if cached:  # (the guess of an iteration is normally the optimized pulse of the one before: still on the device)
            return self._uploads.get('pulses', host)
        return self.engine.dev(host, self.torch.float64)

    def _terms(self, pulses):
        """What the plain, backward and source sweeps propagate with: the (L, nt-1) device tensor ``pulses`` itself,
        or -- non-linear controls -- the (J, nt-1) term coefficients eps_c^p, formed on the device by repeated
        products (as the update kernels form them)."""
        if self.nl is None:
            return pulses
        t = self.torch
        rows = pulses.index_select(0, self._nl_rows)
        coef = rows
        for q in range(1, 4):
            coef = t.where(self._nl_pow > q, coef * rows, coef)
        return coef.contiguous()

    def _set_nonlinear(self, guess):
        """Non-linear controls: the weights w_j = p_j eps_guess^(p_j - 1) of the update sweep, formed on the device
        (kh_set_nonlinear); returns the term coefficients under the guess pulses for the backward sweep."""
        t = self.torch
        rows = guess.index_select(0, self._nl_rows)
        dcde = self._nl_pow.expand_as(rows)
        for q in range(1, 4):
            dcde = t.where(self._nl_pow - 1 >= q, dcde * rows, dcde)
        self.engine.set_nonlinear(self.nl.term_control, self.nl.term_power, dcde.contiguous())
        return self._terms(guess)

    def state_vector(self, state, k):
        """``state`` of objective k as the engine's row (zero-padded to the stride on mixed lists), or None."""
        if self.layout is not None:
            return self.layout.vector(state, k)
        return state_to_vector(state, self.N, self.is_super)

    def _split_guarded(self, sweep, what):
        """``sweep()`` on an engine that spreads an objective's rows over several workgroups (``row_split`` > 1): its
        workgroups wait for each other inside BOTH kinds of sweep, so each is checked when it is done, and one that
        reports KH_ERR_TIMEOUT (its workgroups were not all resident) is redone with one workgroup per objective -- the
        form the engine then keeps for the rest of the optimisation.  Any other engine: just ``sweep()``."""
        eng = self.engine
        if getattr(eng, 'row_split', 1) <= 1:
            return sweep()
        try:
            out = sweep()
            eng.check()
            return out
        except _KrotovHipError as exc:
            if exc.code != _KH_ERR_TIMEOUT:
                raise
            _leave_row_split(eng, what, exc)
            return sweep()

    def _gather_rows(self, local):
        """(K_loc, ...) host array on every rank -> (K_total, ...) on every rank."""
        return gather_rows(local, self.K_total, self.world, self.group, self.engine.device)

    def initial_forward(self, pulses, store=False):
        forward_states = None
        if store:
            self.fw_T_dev, self.fw_prev = self._split_guarded(
                lambda: self.engine.forward(self._terms(self._pulses(pulses)), self.init, store=True), 'forward')
        else:
            self.fw_T_dev = self._split_guarded(
                lambda: self.engine.forward(self._terms(self._pulses(pulses)), self.init), 'forward')
        fw_states_T = self._final_states(self.fw_T_dev)
        if store:
            forward_states = _DeviceTrajectories(self.fw_prev, self.likes, self.k0, final=fw_states_T._array,
                                                 layout=self.layout, engine=self.engine)
        return fw_states_T, forward_states

    def tau_vals(self, fw_states_T):
        if self.targets is None:
            return np.array([None] * self.K_total)
        tau = self.engine.tau(self.targets, self.fw_T_dev).cpu().numpy()
        return self._gather_rows(tau)

    def _final_states(self, psi_T):
        """phi_k(T) of all objectives for the caller: gathered now when sharded (a
        collective), else left on the device until somebody looks at them."""
        if self.world > 1:
            return _LazyStates(self._gather_rows(psi_T.cpu().numpy()), self.likes)
        return _LazyStates(None, self.likes, fetch=lambda: psi_T.cpu().numpy(), layout=self.layout)

    def chi_host(self):
        """Normalised chi_k(T) and their norms of the last iteration, all objectives, on
        the host (only the second-order ``sigma.refresh`` needs them)."""
        chi, norms = self.last_chi
        return self._gather_rows(chi.cpu().numpy()), self._gather_rows(norms.cpu().numpy())

    def _constraint_source(self, constraint):
        """W_k(t_n) of a state-dependent constraint on the stored states under the guess pulses, a (K, nt, N) device
        tensor: formed on the device (kh_apply_store) for the built-in quadratic cost, on the host from the fetched
        trajectory for a ``source()`` of the user's own."""
        t, eng = self.torch, self.engine
        if self._src_store is None:
            self._src_store = t.empty_like(self.fw_prev)
        if isinstance(constraint, QuadraticStateConstraint) and type(constraint).source is QuadraticStateConstraint.source:
            ops = constraint.operators(self.objectives)
            for k, op in enumerate(ops):
                if op is not None and op.shape != (self.N, self.N):
                    raise ValueError("state_dependent_constraint: D of objective %d has shape %s, the states have "
                                     "dimension %d" % (k, op.shape, self.N))
            factors = self._uploads.get('sdc_factors', np.asarray(constraint.factors(self.tlist_host), dtype=np.float64))
            return eng.apply_store(ops, factors, self.fw_prev, out=self._src_store)
        W = np.asarray(constraint.source(self.fw_prev.cpu().numpy(), self.tlist_host), dtype=np.complex128)
        if W.shape != tuple(self.fw_prev.shape):
            raise ValueError("state_dependent_constraint.source returned shape %s, expected %s" % (
                W.shape, tuple(self.fw_prev.shape)))
        self._src_store.copy_(eng.dev(W, t.complex128))
        return self._src_store

    def local_invariants_route(self, constructor):
        """``constructor`` (a ``PerfectEntanglerChi`` / ``LocalInvariantsChi``) when this backend forms its co-states on
        the device (kh_chi_local_invariants: Hilbert space, one GPU, a dense or CSR engine), else None -- the object is
        then called on the host like any user constructor; the reason is logged once."""
        cached = self._li_route
        if cached is not None and cached[0] is constructor:
            return constructor if cached[1] else None
        reason = args = None
        if self.group is not None:
            reason = "process_group= (objectives sharded over GPUs)"
        elif self.lindblad is not None or self.layout is not None or self.is_super:
            reason = "super-operators or objectives of different dimension or kind"
        elif self.fw_T_dev is None:
            reason = "no forward propagation on the device (skip_initial_forward_propagation)"
        else:
            constructor.check_objectives(self.K_total, self.objectives)  # (ValueError, as the host call would raise)
            args = constructor.device_arguments(lambda state: self.state_vector(state, 0))
            if args is None:
                reason = "the canonical basis does not match the state dimension %d" % self.N
        if reason is not None:
            logging.getLogger('krotov').info("%s: co-states on the host (%s)", type(constructor).__name__, reason)
        self._li_route = (constructor, args)
        return constructor if args is not None else None

    def iterate(self, chi_T, chi_norms, guess_pulses, lambda_vals, shape_arrays, sigma=None, forward_states0=None,
                chi_coef=None, par=None, constraint=None, chi_li=None):
        """chi_T: the K_total normalised co-states as :meth:`state_vector` rows (host); chi_norms (K_total,) -- or
        ``chi_coef = (c, d)``, (K_total,) each: chi_k(T) = c_k target_k + d_k phi_k(T) is
        then formed and normalised on the device (kh_chi_boundary) -- or ``chi_li``: what
        :meth:`local_invariants_route` returned (kh_chi_local_invariants).  ``forward_states0``: here ``self.fw_prev``."""
        second_order = sigma is not None or constraint is not None
        guess = self._pulses(guess_pulses, cached=True)
        # every upload of the iteration BEFORE the first sweep is launched: a host-to-device copy from pageable memory
        # is ordered behind the kernels already in the stream and blocks the host until it is done -- issued between the
        # two sweeps it kept the update sweep's launch back until the backward sweep had finished (the GPU idled for
        # two copies and a launch per iteration).  Shapes and step widths rarely change: uploaded when they do.
        shapes = self._uploads.get('shapes', np.array(shape_arrays, dtype=np.float64).reshape(self._per_control()))
        lambdas = self._uploads.get('lambdas', np.asarray(lambda_vals, dtype=np.float64).reshape(
            (1, self.L) if self.replica_form else (self.L,)))
        if second_order:
            self._set_second_order(sigma)
        u_opt = self._set_parametrization(par) if par is not None else None
        terms = self._set_nonlinear(guess) if self.nl is not None else guess
        chi_loc, norms_loc, li_J = self._boundary_costates(chi_T, chi_norms, chi_coef, chi_li)
        self.last_chi = (chi_loc, norms_loc)
        self._backward(chi_loc, norms_loc, terms, constraint)
        opt, psi_T, g_a = self._update((self.chi_store, norms_loc, self.init, guess, shapes, lambdas))
        self.fw_T_dev = psi_T
        self.engine.check()
        if chi_li is not None:
            chi_li.set_device_values(li_J.cpu().numpy())  # (a singular U_B: ValueError)
        return self._results(opt, psi_T, g_a, par, u_opt, second_order)

    # -- the steps of an iteration, in the order ``iterate`` takes them (uploads: none after ``_backward`` has begun its sweep) --
    def _set_second_order(self, sigma):
        """sigma at the interval mid-points (optimize.py:451-452); phi under the guess pulses is the trajectory the
        previous sweep stored, the running one goes to the other buffer.  (A state-dependent constraint without sigma:
        sigma = 0 -- the second-order kernels are the ones that store phi(t_n), which the next iteration's source is
        formed from.)"""
        tl = np.asarray(self.tlist_host)
        if sigma is None:
            sig = np.zeros(self.nt - 1)
        else:
            sig = np.array([sigma(tl[n] + 0.5 * (tl[n + 1] - tl[n])) for n in range(self.nt - 1)], dtype=np.float64)
        if self.fw_next is None:
            self.fw_next = self.torch.empty_like(self.fw_prev)
        if self.replica_form:
            self.engine.set_second_order_replicas(self.fw_prev, self.fw_next, sig[None, :])
        else:
            self.engine.set_second_order(self.fw_prev, self.fw_next, sig)

    def _set_parametrization(self, par):
        """Pulse parametrizations: the update sweep reads u under the guess and f'(u) in place of the guess pulses,
        writes u_new -- the tensor returned -- next to the pulses f(u_new) it propagates with (kh_set_parametrization)."""
        t, eng = self.torch, self.engine
        kind, a, b = par.device_kinds
        u_guess = eng.dev(np.array(par.u, dtype=np.float64).reshape(self.L, self.nt - 1), t.float64)
        dfdu = eng.dev(par.dfdu().reshape(self.L, self.nt - 1), t.float64)
        u_opt = t.empty_like(u_guess)
        eng.set_parametrization(kind, a, b, u_guess, dfdu, u_opt)
        return u_opt

    def _boundary_costates(self, chi_T, chi_norms, chi_coef, chi_li):
        """This rank's normalised chi_k(T) and their norms on the device, from whichever of the three forms ``iterate``
        was given, and the functional's value J of the local-invariants form (a device tensor; else None)."""
        t, eng = self.torch, self.engine
        if chi_coef is not None:
            c, d = chi_coef
            psi = self.fw_T_dev if self.fw_T_dev is not None else self.init  # (d == 0 without phi(T))
            c_dev = self._uploads.get('chi_c', np.ascontiguousarray(c[self.k0:self.k1], dtype=np.complex128), t.complex128)
            d_dev = self._uploads.get('chi_d', np.ascontiguousarray(d[self.k0:self.k1], dtype=np.complex128), t.complex128)
            chi_loc, norms_loc = eng.chi_boundary(self.targets, psi, c_dev, d_dev)
            return chi_loc, norms_loc, None
        if chi_li is not None:
            # (J stays on the device until the sweeps are launched: fetching it here would idle the GPU for a round trip)
            mode, bell, invariants, weight = self._li_route[1]
            return eng.chi_local_invariants(
                self.fw_T_dev, self._uploads.get('li_bell', bell, t.complex128), mode,
                self._uploads.get('li_invariants', invariants), weight, 4.0 / self.K_total)
        chi_loc = eng.dev(np.array(chi_T[self.k0:self.k1]), t.complex128)
        norms_loc = eng.dev(np.asarray(chi_norms, dtype=np.float64)[self.k0:self.k1], t.float64)
        return chi_loc, norms_loc, None

    def _backward(self, chi_loc, norms_loc, guess, constraint):
        """The backward sweep into ``self.chi_store``, with the source term of a state-dependent constraint if there is
        one.  The last place of an iteration that may upload anything: see ``iterate``."""
        eng = self.engine
        if constraint is not None:
            src = self._constraint_source(constraint)
            self.chi_store = eng.backward_source(chi_loc, guess, src, norms_loc, out=self.chi_store)
        else:
            self.chi_store = self._split_guarded(lambda: eng.backward(chi_loc, guess, out=self.chi_store), 'backward')

    def _update(self, args):
        """The update sweep over ``args``, the six tensors of ``forward_update``, by the transport this backend is on;
        returns ``(opt, psi_T, g_a)``."""
        if self.replica_form:
            # a replica engine's update sweep is one workgroup per problem and waits on no other workgroup (no exchange
            # slots, no polling, no residency requirement: DESIGN.md 3.9): it cannot time out, and the retry ladder --
            # set_update_workgroups, the per-interval form -- is not written for it (the engine answers
            # KH_ERR_UNSUPPORTED to both).  Any error here is a real one.
            return self._single_launch(args)
        if self.group is None:
            # the single-launch sweep needs all its workgroups resident at once; when the GPU could not give it that, the
            # ladder redoes it on smaller grids and in the end interval by interval (_update_ladder.py)
            return self._ladder.run(lambda: self._single_launch(args), lambda: self._update_per_interval(args))
        out = self._update_peer_windows(args) if self.p2p else None
        return out if out is not None else self._update_all_reduce(args)

    def _single_launch(self, args):
        out = self.engine.forward_update(*args)
        self.engine.check()
        return out

    def _update_per_interval(self, args):
        """(One GPU) one launch per interval: nothing waits inside a kernel."""
        return self.engine.forward_update_sharded(*args, lambda x: None, graph_chunk=0)

    def _update_peer_windows(self, args):
        """One persistent launch per rank; the per-GPU sums cross the node inside the kernel.  None when the sweep failed
        on any rank: all of them then drop the peer windows together, and the caller goes on with the all-reduce."""
        t, eng = self.torch, self.engine
        if not self._p2p_synced:
            # the ranks' kernels wait for each other INSIDE the sweep (bounded by KH_TIMEOUT_MS): before the first
            # one, line the ranks up -- set-up time (imports, engine creation, operator norms) differs by more than
            # that bound between ranks; afterwards they stay within a sweep's jitter of each other
            t.cuda.synchronize(eng.device)
            self.dist.barrier(group=self.group)
            self._p2p_synced = True
        out, failed = None, 0
        try:
            out = self._single_launch(args)
        except Exception as exc:  # exchange timeout: every rank falls back together
            logging.getLogger('krotov').warning("cross-GPU exchange failed (%s)", exc)
            eng.p2p_why = "peer windows dropped after a failed sweep on this rank: %s" % exc
            failed = 1
        flag = t.tensor([failed], dtype=t.int32, device=eng.device)
        self.dist.all_reduce(flag, op=self.dist.ReduceOp.MAX, group=self.group)
        if int(flag.item()) == 0:
            eng._p2p_used = True
            return out
        self.p2p = False
        eng.disable_p2p()
        eng._p2p_fell_back = True  # (stays with the per-interval transport from here on)
        if not failed:
            eng.p2p_why = "peer windows dropped: the sweep failed on another rank"
        return None

    def _update_all_reduce(self, args):
        """One launch and one all-reduce of the L update sums per interval."""
        def all_reduce(x):
            self.dist.all_reduce(x, op=self.dist.ReduceOp.SUM, group=self.group)

        # HIP-graph replay of the interval loop needs a capturable collective (RCCL)
        chunk = None if self.dist.get_backend(self.group) == 'nccl' else 0
        return self.engine.forward_update_sharded(*args, all_reduce, graph_chunk=chunk)

    def _results(self, opt, psi_T, g_a, par, u_opt, second_order):
        """What ``iterate`` returns, fetched from the update sweep's outputs."""
        fw_states_T = self._final_states(psi_T)
        opt_host = opt.cpu().numpy()
        self._uploads.record('pulses', opt_host, opt)  # (the next iteration's guess, if unchanged)
        if self.replica_form:  # ((1, L, nt - 1) and (1, L): the one replica's rows)
            opt_host, g_a = opt_host[0], g_a[0]
        optimized = [opt_host[l].copy() for l in range(self.L)]
        if par is not None:
            par.commit(u_opt.cpu().numpy(), optimized)
        backward_states = _DeviceTrajectories(self.chi_store, self.likes, self.k0, layout=self.layout)
        forward_states = None
        if second_order:
            forward_states = _DeviceTrajectories(self.fw_next, self.likes, self.k0, final=fw_states_T._array,
                                                 layout=self.layout, engine=self.engine)
        return backward_states, optimized, fw_states_T, g_a.cpu().numpy(), forward_states

    def advance_second_order(self):
        """The stored trajectory of the finished iteration becomes ``forward_states0``
        of the next one (optimize.py:577)."""
        self.fw_prev, self.fw_next = self.fw_next, self.fw_prev


# ---------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------


def _check_arguments(objectives, pulse_options, propagator, mu, overlap, sigma, storage, process_group, constraint,
                     skip_initial_forward_propagation):
    """What ``optimize_pulses`` refuses, decided on the host before any GPU work and any collective (the same verdict on
    every rank); returns ``(device_path, params)``: whether the arguments select the device path, and
    :func:`_parametrizations`."""
    second_order = sigma is not None
    if second_order and skip_initial_forward_propagation:
        raise ValueError(
            "skip_initial_forward_propagation is incompatible with second order Krotov (sigma is not None)"
        )
    if constraint is not None:
        if not isinstance(constraint, StateDependentConstraint):
            raise ValueError("state_dependent_constraint must be a krotov_amd.constraints.StateDependentConstraint, "
                             "not %r" % (constraint,))
        if process_group is not None:
            raise ValueError("state-dependent constraints run on one GPU: process_group= (sharding) is not supported "
                             "with state_dependent_constraint")
        if any(len(obj.c_ops) > 0 for obj in objectives):
            raise NotImplementedError("state_dependent_constraint is not implemented for objectives with c_ops "
                                      "(Lindblad form)")
        if skip_initial_forward_propagation:
            raise ValueError("skip_initial_forward_propagation is incompatible with state_dependent_constraint (the "
                             "source term needs the states under the guess pulses)")
        if layout_of(objectives, propagator).mixed:
            raise ValueError("state_dependent_constraint needs objectives of one dimension and kind")
    device_path = _use_device_path(propagator, mu, overlap, sigma, storage, objectives)
    params = _parametrizations(objectives, pulse_options)
    if params is not None and process_group is not None:
        raise ValueError("pulse parametrizations run on one GPU: process_group= (sharding) is not supported with "
                         "'parametrization' in pulse_options")
    nonlinear = has_control_function(objectives)
    if nonlinear and params is not None:
        raise ValueError("a ControlFunction (non-linear control) together with 'parametrization' in pulse_options is "
                         "not supported")
    if nonlinear and process_group is not None:
        raise ValueError("non-linear controls (ControlFunction) run on one GPU: process_group= (sharding) is not "
                         "supported with them")
    if process_group is not None and not device_path:
        raise ValueError("process_group requires the device path (propagator=krotov_amd.propagators.expm)")
    if device_path and any(len(obj.c_ops) > 0 for obj in objectives):
        # (a control inside c_ops raises here)
        if (lindblad_layout_of(objectives, propagator, None, second_order, params is not None, nonlinear).matrix
                and process_group is not None):
            raise ValueError("objectives in Lindblad form run on one GPU: process_group= (sharding) is not supported "
                             "for the matrix-form engine")
    elif process_group is not None and layout_of(objectives, propagator).mixed:
        raise ValueError("objectives of different dimension or kind run on one GPU: process_group= (sharding) is "
                         "not supported for them")
    return device_path, params


def _device_costates(backend, chi_constructor, tau_vals):
    """``(chi_coef, chi_li)`` for ``_HipBackend.iterate`` where the device forms the boundary co-states itself (both
    None: ``chi_constructor`` is called on the host)."""
    if isinstance(chi_constructor, _functionals._LocalInvariantsFunctional):
        # the perfect-entangler / local-invariants functional itself (not a function wrapping it): the 4 x 4
        # algebra per gate and the co-states on the device
        return None, backend.local_invariants_route(chi_constructor)
    if backend.targets is not None and (backend.fw_T_dev is not None or chi_constructor is _functionals.chis_re):
        # built-in functionals: chi_k(T) is formed and normalised on the device from K scalars
        # (no K-long Python loop, phi_k(T) and chi_k(T) stay in HBM)
        return _functionals.chi_coefficients(chi_constructor, backend.weights, tau_vals, backend.K_total), None
    return None, None


def optimize_pulses(
    objectives,
    pulse_options,
    tlist,
    *,
    propagator,
    chi_constructor,
    mu=None,
    sigma=None,
    iter_start=0,
    iter_stop=5000,
    check_convergence=None,
    info_hook=None,
    modify_params_after_iter=None,
    storage='array',
    parallel_map=None,
    store_all_pulses=False,
    continue_from=None,
    skip_initial_forward_propagation=False,
    norm=None,
    overlap=None,
    limit_thread_pool=None,
    process_group=None,
    state_dependent_constraint=None,
):
    """Optimise all controls in ``objectives`` with Krotov's method.

    Arguments, callbacks, returned :class:`~krotov_amd.result.Result` and raised
    ``ValueError`` s are those of ``krotov.optimize_pulses`` (reference
    optimize.py:33-228).  Differences:

    * ``propagator=krotov_amd.propagators.expm`` runs on the GPU (see module
      docstring); ``parallel_map`` is then unused -- objectives are batched in
      the kernels.
    * ``process_group`` (extension): a ``torch.distributed`` group with one
      rank per GPU; every rank passes the full objective list and gets the
      full result, objectives are sharded contiguously over the ranks.
    * ``sigma`` (second order): on the device path the trajectories phi(t_n) of
      the last two iterations stay in HBM; ``forward_states`` / ``forward_states0``
      handed to ``info_hook`` and ``sigma.refresh`` fetch single states on
      access (with ``process_group``: all time points of this rank's
      objectives, the final time of every objective).
    * ``pulse_options[ctrl]['parametrization']`` (extension): a
      :class:`~krotov_amd.parametrization.Parametrization`, eps = f(u) -- the update is applied to the unconstrained
      u and the control stays inside the range of f (bounded controls).  ``Result``, hooks and dumps hold eps;
      ``g_a_integrals`` is the running cost in u.  The built-in kinds run inside the device's update sweep, a subclass
      of your own through the host loop; not with ``process_group``.
    * non-linear controls (extension): ``[H2, krotov_amd.Power(eps, 2)]`` in ``H`` is a term eps(t)^2 H2 of the SAME
      control as ``[H1, eps]`` -- one pulse, one entry of ``pulse_options`` (keyed by ``eps``), one row of ``Result``
      (:mod:`krotov_amd.nonlinear`).  dH/d eps is evaluated for the guess pulses inside the update; integer powers
      1..4 run inside the device's update sweep (``kh_set_nonlinear``), any other ``ControlFunction`` through the host
      loop.  Not with ``process_group`` or ``'parametrization'``; objectives with ``c_ops`` run as Liouvillians.
    * ``state_dependent_constraint`` (extension): a :class:`~krotov_amd.constraints.StateDependentConstraint`, a running
      cost g_b(phi(t)) -- the backward sweep then carries its source term (:mod:`krotov_amd.constraints`), on the device
      (``kh_apply_store`` + ``kh_backward_store_source``) or, with a propagator of your own, in the host loop.  The
      trajectories phi(t_n) of the last two iterations are kept as in second-order runs (``forward_states`` /
      ``forward_states0`` of ``info_hook``); without ``sigma`` the device's update sweep is the second-order one with
      sigma = 0.  Not with ``process_group``, ``c_ops``, objectives of different dimension or kind, or
      ``skip_initial_forward_propagation``.
    * ``limit_thread_pool`` is accepted and ignored (no BLAS on the hot path).
    """
    logger = logging.getLogger('krotov')
    logger.info("Initializing optimization with Krotov's method")
    second_order = sigma is not None
    constraint = state_dependent_constraint
    keeps_states = second_order or constraint is not None  # phi(t_n) of the last two iterations are kept
    device_path, params = _check_arguments(objectives, pulse_options, propagator, mu, overlap, sigma, storage,
                                           process_group, constraint, skip_initial_forward_propagation)
    if mu is None:
        mu = derivative_wrt_pulse
    default_norm = norm is None
    if norm is None:
        norm = _run.default_norm
    if overlap is None:
        overlap = _overlap
    info_hook = _run.chained_hook(modify_params_after_iter, info_hook)
    if isinstance(propagator, list):
        propagators = propagator
        assert len(propagators) == len(objectives)
    else:
        propagators = [copy.deepcopy(propagator) for _ in objectives]
    _check_propagators_interface(propagators, logger)

    adjoint_objectives = [obj.adjoint() for obj in objectives]
    if storage == 'array':
        storage = partial(np.empty, dtype=object)
    if parallel_map is None:
        parallel_map = serial_map
    if not isinstance(parallel_map, (tuple, list)):
        parallel_map = (parallel_map, parallel_map, parallel_map)

    (guess_controls, guess_pulses, pulses_mapping, lambda_vals, shape_arrays) = _initialize_krotov_controls(
        objectives, pulse_options, tlist
    )
    if continue_from is not None:
        guess_controls, guess_pulses = _restore_from_previous_result(
            continue_from, objectives, tlist, store_all_pulses
        )
    g_a_integrals = np.zeros(len(guess_pulses))
    par = None
    if params is not None:
        # u of the first guess (a value outside the range raises, naming control and interval); a continued run
        # re-derives it from the stored pulses, where rounding may have put a value on a bound
        par = PulseParameters(params, guess_pulses, pull=continue_from is not None)
    static_args = dict(
        objectives=objectives, adjoint_objectives=adjoint_objectives, lambda_vals=lambda_vals,
        shape_arrays=shape_arrays, tlist=tlist, propagator=propagator, chi_constructor=chi_constructor,
        mu=mu, sigma=sigma, iter_start=iter_start, iter_stop=iter_stop,
    )
    run = _run.RunRecord(static_args, continue_from, store_all_pulses, info_hook, check_convergence)

    # ---- the backend: all objectives in the device's sweeps, or the host loop around the user's callables
    if device_path and par is not None and par.device_kinds is None:
        logger.info("pulse parametrization: a user-defined Parametrization (kind None) is evaluated on the host; "
                    "running the host loop around single-step propagations on the GPU")
        device_path = False
    plan = term_plan(objectives, pulses_mapping, len(guess_pulses))  # (None: no ControlFunction in any H)
    if device_path and plan is False:
        logger.info("non-linear controls: a user-defined ControlFunction (power None) is evaluated on the host; "
                    "running the host loop around single-step propagations on the GPU")
        device_path = False
    if device_path and plan is not None and plan.J > _KH_MAX_CONTROLS:
        logger.warning("%d terms: the device sweeps take at most %d; running the host loop around single-step "
                       "propagations on the GPU", plan.J, _KH_MAX_CONTROLS)
        device_path = False
    if device_path and len(guess_pulses) > _KH_MAX_CONTROLS and process_group is None:
        # the sweep kernels are compiled for at most 32 controls (KH_GEN_MAX_L: the generic kernels; the register-resident
        # families take 8); the reference takes any number (optimize.py:33-55, conversions.py:140-254).  More than that
        # runs the reference's own structure: the host loop around single-interval propagations (each of them on the
        # GPU) -- correct, and slow
        logger.warning("%d controls: the device sweeps take at most %d; running the host loop around single-step "
                       "propagations on the GPU", len(guess_pulses), _KH_MAX_CONTROLS)
        device_path = False
    if device_path:
        backend = _HipBackend(objectives, pulses_mapping, tlist, len(guess_pulses), propagator, process_group,
                              second_order=second_order, parametrized=par is not None,
                              replica_form=default_norm and _one_gate_replica_form(
                                  objectives, propagator, len(guess_pulses), chi_constructor, process_group,
                                  par is not None or constraint is not None or skip_initial_forward_propagation
                                  or plan is not None))
    else:
        backend = _PluginBackend(
            objectives, adjoint_objectives, pulses_mapping, tlist, propagators, storage, parallel_map, mu, overlap
        )

    # ---- iteration 0: forward propagation under the guess (optimize.py:295-322)
    tic = time.time()
    if skip_initial_forward_propagation:
        if continue_from is not None:
            fw_states_T = list(continue_from.states)
        else:
            logger.warning(
                "You should not use `skip_initial_forward_propagation` unless you are also passing `continue_from`"
            )
            fw_states_T = [None for _ in objectives]
        forward_states = None
        tau_vals = np.array([overlap(obj.target, s) for s, obj in zip(fw_states_T, objectives)])
    else:
        fw_states_T, forward_states = backend.initial_forward(guess_pulses, store=keeps_states)
        tau_vals = backend.tau_vals(fw_states_T)
    toc = time.time()
    # the stored trajectories are only needed by the second-order update (optimize.py:324-329);
    # in iteration 0 the states under "optimized" and guess pulses coincide
    forward_states0 = forward_states = forward_states if keeps_states else None
    optimized_pulses = copy.deepcopy(guess_pulses)
    run.record_initial(guess_controls, pulses_mapping, guess_pulses, optimized_pulses, g_a_integrals, fw_states_T,
                       tau_vals, forward_states, tic, toc)

    # ---- main loop (optimize.py:392-581)
    iteration = run.iter_start
    go_on = run.verdict(iteration)
    while go_on:
        iteration += 1
        logger.info("Started Krotov iteration %d", iteration)
        tic = time.time()

        chi_coef = chi_li = None
        if device_path and default_norm:  # (the built-in functionals: co-states formed on the device)
            chi_coef, chi_li = _device_costates(backend, chi_constructor, tau_vals)
        chi_states = chi_norms = chi_T = None
        if chi_coef is None and chi_li is None:
            chi_states, chi_norms, chi_T = _run.host_costates(
                chi_constructor, norm, backend.state_vector, fw_states_T=fw_states_T, objectives=objectives, tau_vals=tau_vals)

        g_a_integrals[:] = 0.0
        if par is not None:
            # u is carried from sweep to sweep; only a pulse that a hook (modify_params_after_iter) has edited since
            # is inverted again
            redone = par.sync(guess_pulses)
            if redone:
                logger.info("pulse parametrization: controls %s were changed after the last sweep; u re-derived", redone)
        backward_states, optimized_pulses, fw_states_T, g_a, forward_states = backend.iterate(
            chi_T, chi_norms, guess_pulses, lambda_vals, shape_arrays, sigma=sigma, forward_states0=forward_states0,
            chi_coef=chi_coef, par=par, constraint=constraint, chi_li=chi_li,
        )
        g_a_integrals[:] = g_a
        tau_vals = backend.tau_vals(fw_states_T)
        toc = time.time()

        run.record_iteration(iteration, backward_states, forward_states, forward_states0, fw_states_T, guess_pulses,
                             optimized_pulses, g_a_integrals, tau_vals, tic, toc)
        logger.info("Finished Krotov iteration %d", iteration)
        go_on = run.verdict(iteration, run.convergence())
        if not go_on:
            break
        guess_pulses = optimized_pulses
        if second_order:
            if chi_states is None:  # co-states formed on the device, in the caller's state type
                chi_T, chi_norms = backend.chi_host()
                chi_states = _LazyStates(chi_T, backend.likes, layout=backend.layout)
            sigma.refresh(
                forward_states=forward_states, forward_states0=forward_states0, chi_states=chi_states,
                chi_norms=chi_norms, optimized_pulses=optimized_pulses, guess_pulses=guess_pulses,
                objectives=objectives, result=run.result,
            )
        if keeps_states:
            forward_states0 = forward_states
            backend.advance_second_order()

    # ---- finalize (optimize.py:583-590)
    run.finish(optimized_pulses)
    return run.result
