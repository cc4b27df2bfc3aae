"""Objectives of different dimension or kind on one engine: the per-objective layout (host only, no GPU needed).

The reference propagates every objective on its own (its own ``H``, its own propagator call, its own state:
reference src/krotov/optimize.py:254-261, 806-911), so an objective list may mix a 3-level ket with a 5-level ket and
a qutrit density matrix under a Liouvillian.  On the device such a list runs on ONE mixed engine
(``kh_engine_create_mixed``): objective k keeps its states in rows of the stride ``S = max N_k``, the first ``N_k``
entries hold the state and the engine writes exact zeros behind them.  :class:`Layout` decides ``N_k`` and the kind
(Hilbert or Liouville) of every objective, pads states into such rows and slices them back.
"""
import numpy as np

from ._ingest import obj_type, state_array, state_to_vector, to_dense, vector_to_state

__all__ = ['Layout', 'layout_of', 'objective_kind', 'LindbladLayout', 'lindblad_layout_of']


class Layout:
    """Dimension ``dims[k]`` and kind ``kinds[k]`` (True: Liouville space) of every objective; ``stride`` = max N_k.
    ``mixed``: the objectives differ in dimension or kind (a uniform list keeps the uniform engine)."""

    def __init__(self, dims, kinds):
        self.dims = [int(n) for n in dims]
        self.kinds = [bool(x) for x in kinds]
        if len(self.dims) != len(self.kinds) or not self.dims:
            raise ValueError("one dimension and one kind per objective")
        self.stride = max(self.dims)
        self.mixed = len(set(self.dims)) > 1 or len(set(self.kinds)) > 1

    def vector(self, state, k):
        """``state`` as objective k's row: the length-N_k vector (kets raveled, density matrices column-stacked) and
        zeros up to the stride; None if it is not a state of objective k (e.g. the target 'PE')."""
        vec = state_to_vector(state, self.dims[k], self.kinds[k])
        if vec is None or vec.size == self.stride:
            return vec
        row = np.zeros(self.stride, dtype=np.complex128)
        row[:vec.size] = vec
        return row

    def unpad(self, row, k):
        """The first N_k entries of objective k's row."""
        return np.asarray(row)[:self.dims[k]]

    def state(self, row, k, like):
        """Objective k's row as a state of the same kind and class as ``like`` (ket, density matrix, Qobj-like)."""
        return vector_to_state(self.unpad(row, k), like)


def _drift(obj, k):
    H = obj.H if isinstance(obj.H, list) else [obj.H]
    drift = [t for t in H if not isinstance(t, list)]
    if len(drift) == 0:
        raise ValueError("objective %d has no drift term in H" % k)
    return drift[0]


def _dim(op):
    shape = getattr(op, 'shape', None)
    if shape is None:
        shape = to_dense(op).shape
    return int(shape[0])


def objective_kind(obj, drift_op, dim, propagator=None):
    """Hilbert (False) or Liouville (True) space for one objective, in this order of precedence: the objective's own
    ``HipExpm(liouville=...)``; ``.type`` of its first drift operator; the shape of its initial state (a square
    matrix with N_k entries is a density matrix under a Liouvillian)."""
    liouville = getattr(propagator, 'liouville', None)
    if liouville is not None:
        return bool(liouville)
    if obj_type(drift_op) is not None:
        return obj_type(drift_op) == 'super'
    s0 = state_array(obj.initial_state)
    return bool(s0.ndim == 2 and s0.shape[0] == s0.shape[1] and s0.shape[0] > 1 and s0.size == dim)


def layout_of(objectives, propagator=None):
    """The :class:`Layout` of an objective list.  ``propagator``: one propagator for all objectives, or a list of one
    per objective (the reference's ``propagator=[...]``)."""
    K = len(objectives)
    props = propagator if isinstance(propagator, list) else [propagator]
    per_obj = len(props) == K
    common = None  # (a list of another length: its last explicit liouville= holds for every objective)
    for p in props:
        if getattr(p, 'liouville', None) is not None:
            common = p
    dims, kinds = [], []
    for k, obj in enumerate(objectives):
        op = _drift(obj, k)
        n = _dim(op)
        prop = props[k] if per_obj else common
        dims.append(n)
        kinds.append(objective_kind(obj, op, n, prop))
    return Layout(dims, kinds)


# the limits of the Lindblad-form kernels (krotov_amd/csrc/kh_lind.h: KH_LIND_DMAX, KH_LIND_MAX_NC, KH_LIND_MAX_L)
LIND_DMAX, LIND_MAX_NC, LIND_MAX_L = 32, 4, 4


class LindbladLayout:
    """How an objective list with ``c_ops`` runs on the device (:func:`lindblad_layout_of`).  ``decision``:
    ``'matrix'`` -- the Lindblad-form engine (``"lindblad/matrix"``): every objective a d x d density matrix under a
    d x d Hamiltonian, ``d`` common, ``n_c`` the largest number of Lindblad operators; or ``'liouvillian'`` -- the
    Liouvillian fallback: ``liouvillian(H, c_ops)`` is built on the host for every objective with ``c_ops`` and today's
    uniform / mixed engine runs, for the ``reason`` given."""

    def __init__(self, decision, reason=None, d=None, n_c=0):
        self.decision, self.reason, self.d, self.n_c = decision, reason, d, n_c

    @property
    def matrix(self):
        return self.decision == 'matrix'

    @staticmethod
    def liouvillian_objectives(objectives):
        """The same list with every Lindblad-form objective rewritten as ``H = liouvillian(H, c_ops)``, ``c_ops = []``
        (the nested-list positions of the controls do not change)."""
        from .objectives import Objective, liouvillian

        out = []
        for obj in objectives:
            if len(obj.c_ops) == 0:
                out.append(obj)
                continue
            new = Objective(initial_state=obj.initial_state, H=liouvillian(obj.H, obj.c_ops), target=obj.target, c_ops=[])
            if getattr(obj, 'weight', None) is not None:
                new.weight = obj.weight
            out.append(new)
        return out


def lindblad_layout_of(objectives, propagator=None, n_controls=None, second_order=False, parametrized=False,
                       nonlinear=False):
    """Decide, on the host, how a list in which some objective carries ``c_ops`` runs (see :class:`LindbladLayout`).
    A control inside ``c_ops`` raises ``NotImplementedError`` (as the reference's ``mu`` does, mu.py:135-139).  Objectives
    without ``c_ops`` are fine in a matrix-form list when they, too, are d x d density matrices under a d x d
    Hamiltonian."""
    for obj in objectives:
        if any(isinstance(c, list) for c in obj.c_ops):
            raise NotImplementedError("Time-dependent collapse operators not implemented")
    if second_order:
        return LindbladLayout('liouvillian', "second-order update (sigma=)")
    if parametrized:
        return LindbladLayout('liouvillian', "pulse parametrization ('parametrization' in pulse_options)")
    if nonlinear:
        return LindbladLayout('liouvillian', "non-linear controls (a ControlFunction in H)")
    ds, n_c = set(), 0
    for k, obj in enumerate(objectives):
        op = _drift(obj, k)
        d = _dim(op)
        s0 = state_array(obj.initial_state)
        if obj_type(op) == 'super' or not (s0.ndim == 2 and s0.shape == (d, d) and d > 1):
            return LindbladLayout('liouvillian', "objective %d is not a d x d density matrix under a d x d Hamiltonian "
                                  "(kets and Lindblad-form objectives mixed)" % k)
        if any(_dim(c) != d for c in obj.c_ops):
            raise ValueError("objective %d: c_ops must have the dimension of H" % k)
        ds.add(d)
        n_c = max(n_c, len(obj.c_ops))
    if len(ds) > 1:
        return LindbladLayout('liouvillian', "objectives of different dimension %s" % sorted(ds))
    d = ds.pop()
    if d > LIND_DMAX:
        return LindbladLayout('liouvillian', "d = %d > %d" % (d, LIND_DMAX), d=d, n_c=n_c)
    if n_c > LIND_MAX_NC:
        return LindbladLayout('liouvillian', "%d Lindblad operators > %d" % (n_c, LIND_MAX_NC), d=d, n_c=n_c)
    if n_controls is not None and n_controls > LIND_MAX_L:
        return LindbladLayout('liouvillian', "%d controls > %d" % (n_controls, LIND_MAX_L), d=d, n_c=n_c)
    return LindbladLayout('matrix', d=d, n_c=n_c)
