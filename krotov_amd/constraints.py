"""State-dependent constraints: running costs g_b(phi(t), t) in Krotov's functional.

The reference lists them under "not yet implemented" (its how-to "How to penalize population in a forbidden subspace"
sends the user to a non-Hermitian Hamiltonian instead): a running cost turns the co-state equation into an
inhomogeneous one,

    d chi / dt = -i H^+ chi + d g_b / d <phi|         (reference docs/07_krotovs_method.rst, eq. ``bw_eqm``)

while the pulse update itself stays as it is.  ``optimize_pulses(..., state_dependent_constraint=...)`` takes an object
of this module; with ``W_k(t_n) = -d g_b / d <phi_k|`` taken on the forward states of the previous iteration -- the sign
convention of ``chi_k(T) = -d J_T / d <phi_k|`` -- the backward sweep becomes

    chi[nt-1] = chi(T),    chi[n] = V_n (chi[n+1] + h_n W[n+1]) + h_n W[n],    h_n = dt_n / 2 / ||chi_k(T)||

(trapezoid in the source, the propagator's own backward step V_n; ``chi`` is the normalised co-state the update reads).

:class:`QuadraticStateConstraint` is the built-in cost ``g_b(t) = (lambda_b / T) s_b(t) sum_k <phi_k(t)|D_k|phi_k(t)>``.
First-order monotonic convergence needs ``lambda_b D_k <= 0`` -- e.g. ``D`` the projector onto the allowed subspace and
``lambda_b < 0`` --; anything else is combined with ``sigma=``.
"""
from abc import ABC, abstractmethod

import numpy as np

from ._ingest import state_array, to_dense

__all__ = ['StateDependentConstraint', 'QuadraticStateConstraint', 'trapezoid_weights']


def trapezoid_weights(tlist):
    """Weights omega_n of the trapezoid rule on ``tlist`` (any spacing)."""
    dt = np.diff(np.asarray(tlist, dtype=np.float64))
    w = np.zeros(len(dt) + 1)
    w[:-1] += 0.5 * dt
    w[1:] += 0.5 * dt
    return w


def _vector(state, N):
    """A state as the length-N vector the sweeps propagate (kets raveled, density matrices column-stacked)."""
    arr = state_array(state)
    if arr.ndim == 2 and arr.shape[0] == arr.shape[1] and arr.shape[0] > 1 and arr.size == N:
        return arr.ravel(order='F')
    return arr.ravel()


class StateDependentConstraint(ABC):
    """A running cost g_b(phi(t), t).  ``forward_states[k][n]`` is phi_k(t_n) -- states of the caller's type, rows of a
    ``(K, nt, N)`` array, or the device trajectories of a GPU run."""

    def operators(self, objectives):
        """One ``(N, N)`` array (or ``None``: unconstrained) per objective when ``W_k(t_n) = factors[n] D_k phi_k(t_n)``,
        which the device then forms itself; ``None`` (default) when :meth:`source` is the only form."""
        return None

    def factors(self, tlist):
        """The real factor per time point that goes with :meth:`operators`."""
        return np.ones(len(tlist))

    @abstractmethod
    def source(self, forward_states, tlist):
        """``W_k(t_n) = -d g_b / d <phi_k|`` on the given trajectories, a ``(K, nt, N)`` complex array."""

    @abstractmethod
    def integral(self, forward_states, tlist):
        """The integral of g_b over ``tlist`` on the given trajectories, by the trapezoid rule."""


class QuadraticStateConstraint(StateDependentConstraint):
    """``g_b(t) = (lambda_b / T) s_b(t) sum_k <phi_k(t)|D_k|phi_k(t)>`` with ``T = tlist[-1] - tlist[0]``.

    Args:
        D: a Hermitian ``N x N`` operator in the objectives' state space (array or Qobj-like) for every objective, or a
            list with one per objective (``None``: that objective is unconstrained).
        lambda_b: the weight.
        shape: ``s_b``, a callable ``s(t)`` or an array on ``tlist``; default 1.

    A subclass that overrides :meth:`source` has its W formed on the host, from the fetched trajectory, and uploaded;
    the backward sweep stays on the device."""

    def __init__(self, D, lambda_b, shape=None):
        self._shared = not isinstance(D, (list, tuple))
        ops = [D] if self._shared else list(D)
        cache = {}

        def dense(op):
            if op is None:
                return None
            if id(op) not in cache:  # (objectives sharing an operator share its array -- and its device copy)
                arr = np.ascontiguousarray(to_dense(op), dtype=np.complex128)
                if arr.ndim != 2 or arr.shape[0] != arr.shape[1]:
                    raise ValueError("D must be a square operator, not of shape %s" % (arr.shape,))
                cache[id(op)] = (arr, op)
            return cache[id(op)][0]

        self._ops = [dense(op) for op in ops]
        if self._shared and self._ops[0] is None:
            raise ValueError("D is None: no objective is constrained")
        self.lambda_b = float(lambda_b)
        self.shape = shape

    def operators(self, objectives):
        K = len(objectives)
        if self._shared:
            return [self._ops[0]] * K
        if len(self._ops) != K:
            raise ValueError("D lists %d operators for %d objectives" % (len(self._ops), K))
        return list(self._ops)

    def _shape_values(self, tlist):
        tlist = np.asarray(tlist, dtype=np.float64)
        if self.shape is None:
            return np.ones(len(tlist))
        if callable(self.shape):
            return np.array([float(self.shape(t)) for t in tlist], dtype=np.float64)
        s = np.asarray(self.shape, dtype=np.float64)
        if s.shape != tlist.shape:
            raise ValueError("shape must be a callable or an array on tlist")
        return s

    def factors(self, tlist):
        """``-(lambda_b / T) s_b(t_n)``."""
        tlist = np.asarray(tlist, dtype=np.float64)
        return -(self.lambda_b / (tlist[-1] - tlist[0])) * self._shape_values(tlist)

    def source(self, forward_states, tlist):
        ops = self.operators(forward_states)
        c = self.factors(tlist)
        K, nt = len(ops), len(tlist)
        N = next(op.shape[0] for op in ops if op is not None)
        W = np.zeros((K, nt, N), dtype=np.complex128)
        for k, op in enumerate(ops):
            if op is None:
                continue
            traj = forward_states[k]
            for n in range(nt):
                W[k, n] = c[n] * (op @ _vector(traj[n], N))
        return W

    def expectations(self, forward_states, tlist):
        """``sum_k <phi_k(t_n)|D_k|phi_k(t_n)>`` for every n (real part); device trajectories of a Hilbert-space run go
        through ``HipKrotovEngine.expect``."""
        ops = self.operators(forward_states)
        nt = len(tlist)
        engine = getattr(forward_states, '_engine', None)
        if engine is not None and not engine.mixed and not engine.is_super and forward_states._t.shape[0] == len(ops):
            vals = engine.expect(forward_states._t, [[op] for op in ops])  # (1, K, nt); None: exact zeros
            return vals[0].real.sum(dim=0).cpu().numpy()
        N = next(op.shape[0] for op in ops if op is not None)
        total = np.zeros(nt)
        for k, op in enumerate(ops):
            if op is None:
                continue
            traj = forward_states[k]
            for n in range(nt):
                v = _vector(traj[n], N)
                total[n] += np.vdot(v, op @ v).real
        return total

    def integral(self, forward_states, tlist):
        g_b = -self.factors(tlist) * self.expectations(forward_states, tlist)
        return float(np.dot(trapezoid_weights(tlist), g_b))
