"""Non-linear controls: terms ``g(eps(t)) H`` in an objective's nested list.

A field strong enough to need amplitude bounds also drives the quadratic Stark shift and two-photon couplings:
``H(eps) = H0 + eps H1 + eps^2 H2`` with ONE physical control eps(t).  Written as ::

    H = [H0, [H1, eps], [H2, krotov_amd.Power(eps, 2)]]

the wrapped control is the same control as the bare one: one pulse, one entry of ``pulse_options`` (keyed by ``eps``),
one row in ``Result``.  Krotov's update keeps dH/d eps inside the sum, evaluated for the guess pulse (the reference's
derivation, docs/07_krotovs_method.rst:339-347, and the reason its ``mu`` takes ``pulses`` and ``time_index``):

    D_c = sum_j g_j'(eps_guess[n]) D_j,   eps[n] = eps_guess[n] + (S[n] / lambda) D_c,

and interval n is propagated with the coefficients ``g_j(eps[n])``.  Integer powers 1..4 run inside the device's update
sweep (``kh_set_nonlinear``: one operator slot per distinct (control, power)); any other :class:`ControlFunction` runs
the host loop, like a user-defined ``Parametrization``.
"""
import abc

import numpy as np

__all__ = ['ControlFunction', 'Power', 'unwrap', 'has_control_function', 'needs_host_loop', 'TermPlan', 'term_plan']

MAX_DEVICE_POWER = 4  # (include/krotov_hip.h: kh_set_nonlinear takes powers 1..4)


class ControlFunction(abc.ABC):
    """``g(eps)`` of a control, standing where the control stands in a nested list: ``[H, g]``.  ``control`` is the
    underlying control (a function of t or an array on the time grid); ``value`` and ``derivative`` take a pulse value
    or an array of them; ``power`` is the integer p when g(eps) = eps^p, else None (then the host loop runs)."""

    power = None

    def __init__(self, control):
        if isinstance(control, ControlFunction):
            raise ValueError("a ControlFunction wraps a control, not another ControlFunction")
        self.control = control

    @abc.abstractmethod
    def value(self, eps):
        """g(eps)"""

    @abc.abstractmethod
    def derivative(self, eps):
        """dg/d eps"""

    def with_control(self, control):
        """The same function of another control (``Result.optimized_objectives`` plugs the optimized control in)."""
        import copy

        new = copy.copy(self)
        new.control = control
        return new

    def __eq__(self, other):
        if type(other) is not type(self):
            return NotImplemented
        mine = {k: v for k, v in self.__dict__.items() if k != 'control'}
        theirs = {k: v for k, v in other.__dict__.items() if k != 'control'}
        a, b = self.control, other.control
        same = a is b or (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape
                          and bool(np.all(a == b)))
        return same and mine == theirs

    __hash__ = None

    def __repr__(self):
        return "%s(%r)" % (type(self).__name__, self.control)


class Power(ControlFunction):
    """``eps^p`` for an integer p in 1..4 -- written out as repeated products, as the device forms it."""

    def __init__(self, control, p):
        super().__init__(control)
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 1 <= int(p) <= MAX_DEVICE_POWER:
            raise ValueError("Power: p must be an integer in 1..%d, not %r" % (MAX_DEVICE_POWER, p))
        self.power = int(p)

    def value(self, eps):
        out = eps
        for _ in range(self.power - 1):
            out = out * eps
        return out

    def derivative(self, eps):
        out = self.power * (eps * 0 + 1)
        for _ in range(self.power - 1):
            out = out * eps
        return out

    def __repr__(self):
        return "Power(%r, %d)" % (self.control, self.power)


def unwrap(control):
    """The control itself: a :class:`ControlFunction`'s underlying control, anything else unchanged."""
    return control.control if isinstance(control, ControlFunction) else control


def has_control_function(objectives, c_ops_too=True):
    """Whether any nested list of ``objectives`` holds a :class:`ControlFunction`."""
    for obj in objectives:
        lists = [obj.H] + (list(obj.c_ops) if c_ops_too else [])
        for lst in lists:
            if isinstance(lst, list):
                for term in lst:
                    if isinstance(term, list) and len(term) == 2 and isinstance(term[1], ControlFunction):
                        return True
    return False


def needs_host_loop(objectives):
    """Whether some ``H`` holds a :class:`ControlFunction` that is no integer power (``power None``): the device's sweeps
    cannot evaluate it."""
    for obj in objectives:
        if isinstance(obj.H, list):
            for term in obj.H:
                if isinstance(term, list) and len(term) == 2 and isinstance(term[1], ControlFunction) and term[1].power is None:
                    return True
    return False


class TermPlan:
    """How the engine's operator slots map to the controls: slot 1 + j holds the sum of the operators that stand with
    ``controls[term_control[j]] ** term_power[j]``; ``mapping[k][0][j]`` are their positions in objective k's ``H``."""

    def __init__(self, term_control, term_power, mapping, n_controls):
        self.term_control = np.asarray(term_control, dtype=np.int32)
        self.term_power = np.asarray(term_power, dtype=np.int32)
        self.mapping = mapping
        self.C = n_controls
        self.J = len(term_control)


def term_plan(objectives, pulses_mapping, n_controls):
    """The :class:`TermPlan` of ``objectives`` -- one term per distinct (control, power), ordered by control, then
    power --, ``None`` when no ``H`` holds a :class:`ControlFunction`, ``False`` when one of them is no integer power
    (``power is None``: the host loop).  ``ControlFunction`` s inside ``c_ops`` are not looked at here (``mu`` raises
    for them)."""
    if not has_control_function(objectives, c_ops_too=False):
        return None
    pairs = set()
    for k, obj in enumerate(objectives):
        for c in range(n_controls):
            for i in pulses_mapping[k][0][c]:
                g = obj.H[i][1]
                p = g.power if isinstance(g, ControlFunction) else 1
                if p is None:
                    return False
                pairs.add((c, int(p)))
    for c in range(n_controls):
        if not any(pc == c for pc, _ in pairs):
            pairs.add((c, 1))  # (a control only inside c_ops: an empty slot, as without this module)
    terms = sorted(pairs)
    mapping = []
    for k, obj in enumerate(objectives):
        row = []
        for c, p in terms:
            row.append([i for i in pulses_mapping[k][0][c]
                        if (obj.H[i][1].power if isinstance(obj.H[i][1], ControlFunction) else 1) == p])
        mapping.append([row])
    return TermPlan([c for c, _ in terms], [p for _, p in terms], mapping, n_controls)
