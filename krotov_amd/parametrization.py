"""Pulse parametrizations: bounded controls.

A control that must stay inside a range is written as eps(t) = f(u(t)) with an unconstrained u(t); Krotov's method
then updates u.  With dH/du = f'(u) dH/d eps taken at the guess, the update of control l at interval n is

    c      = f'(u_old[n])
    D'     = c * D                                # D: the update sum of the unparametrized method
    u_new  = u_old[n] + (S[n] / lambda_a) * D'
    g_a   += (S[n] / lambda_a) * D'**2 * dt       # the running cost in u: the quantity that is monotone
    eps_new = f(u_new)                            # what the interval is propagated with

(the reference's how-to "How to limit the amplitude of the controls" writes the method down and lists it as planned;
clipping in ``modify_params_after_iter``, its stand-in, loses monotonic convergence).  Use::

    pulse_options[ctrl] = dict(lambda_a=..., update_shape=..., parametrization=TanhParametrization(-0.4, 0.45))

``Result``, hooks and dumps keep holding eps.  The built-in kinds run inside the device's update sweep
(``kh_set_parametrization``); a subclass of :class:`Parametrization` of your own runs through the host loop.
"""
from abc import ABC, abstractmethod

import numpy as np

__all__ = ['Parametrization', 'LinearParametrization', 'SquareParametrization', 'TanhSqParametrization',
           'TanhParametrization']

# enum kh_par_kind of include/krotov_hip.h
KH_PAR_NONE, KH_PAR_LINEAR, KH_PAR_SQUARE, KH_PAR_TANHSQ, KH_PAR_TANH = range(5)

# the interior point nearest to +-1, for the argument of atanh
_INSIDE = float(np.nextafter(1.0, 0.0))
# how far beyond a bound a value may lie and still count as "rounding put it there", in ulps of the larger bound:
# f(u) = a t + b rounds three times (a, b, the sum); ``pull`` may name a larger number (a pulse that went through the
# grid-point form and back, a recurrence over the intervals, collects an ulp per interval)
_ON_BOUND_ULPS = 4


def _ulps(pull):
    return _ON_BOUND_ULPS if pull is True else float(pull)


def _first_bad(bad):
    return int(np.flatnonzero(bad)[0])


class Parametrization(ABC):
    """eps = f(u).  Subclasses give ``eps(u)``, ``deps_du(u)`` and the inverse ``u(eps)``, all element-wise on arrays.

    ``kind`` / ``a`` / ``b`` name a form the device evaluates itself (``enum kh_par_kind``); ``kind = None`` -- every
    user-defined subclass -- runs through the host loop."""

    kind = None
    a = 0.0
    b = 0.0

    @abstractmethod
    def eps(self, u):
        """The control amplitude f(u)."""

    @abstractmethod
    def deps_du(self, u):
        """f'(u)."""

    @abstractmethod
    def u(self, eps, pull=False):
        """The parameter of the amplitude ``eps``.  A value outside the range of f raises ``ValueError``; with ``pull``
        (True, or a number of ulps of the larger bound) a value that rounding put on a bound -- an f(u) computed
        earlier -- is taken as the nearest point inside."""


class LinearParametrization(Parametrization):
    """eps = a u + b: the unparametrized update with lambda_a / a**2 (no bound; the form the oracle checks as it
    stands)."""

    kind = KH_PAR_LINEAR

    def __init__(self, a, b=0.0):
        if a == 0:
            raise ValueError("LinearParametrization: a must not be zero")
        self.a, self.b = float(a), float(b)

    def eps(self, u):
        return self.a * np.asarray(u, dtype=np.float64) + self.b

    def deps_du(self, u):
        return np.full(np.shape(u), self.a)

    def u(self, eps, pull=False):
        return (np.asarray(eps, dtype=np.float64) - self.b) / self.a


class SquareParametrization(Parametrization):
    """eps = u**2 >= 0."""

    kind = KH_PAR_SQUARE

    def eps(self, u):
        u = np.asarray(u, dtype=np.float64)
        return u * u

    def deps_du(self, u):
        return 2.0 * np.asarray(u, dtype=np.float64)

    def u(self, eps, pull=False):
        eps = np.asarray(eps, dtype=np.float64)
        bad = ~(eps >= 0.0)
        if np.any(bad):
            i = _first_bad(bad)
            raise ValueError("value %r at index %d is outside the range [0, inf) of SquareParametrization"
                             % (float(eps.flat[i]), i))
        return np.sqrt(eps)


class TanhSqParametrization(Parametrization):
    """eps = eps_max tanh(u)**2, in [0, eps_max)."""

    kind = KH_PAR_TANHSQ

    def __init__(self, eps_max):
        if not eps_max > 0:
            raise ValueError("TanhSqParametrization: eps_max must be positive")
        self.eps_max = self.a = float(eps_max)

    def eps(self, u):
        t = np.tanh(np.asarray(u, dtype=np.float64))
        return self.a * (t * t)

    def deps_du(self, u):
        t = np.tanh(np.asarray(u, dtype=np.float64))
        return 2.0 * self.a * t * (1.0 - t * t)

    def u(self, eps, pull=False):
        eps = np.asarray(eps, dtype=np.float64)
        x = eps / self.a
        if pull:
            x = np.where((x >= 1.0) & (eps <= self.a + _ulps(pull) * np.spacing(self.a)), _INSIDE, x)
        bad = ~((x >= 0.0) & (x < 1.0))
        if np.any(bad):
            i = _first_bad(bad)
            raise ValueError("value %r at index %d is outside the range [0, %r) of TanhSqParametrization"
                             % (float(eps.flat[i]), i, self.a))
        return np.arctanh(np.minimum(np.sqrt(x), _INSIDE))


class TanhParametrization(Parametrization):
    """eps = a tanh(u) + b with a = (eps_max - eps_min) / 2, b = (eps_max + eps_min) / 2: in (eps_min, eps_max)."""

    kind = KH_PAR_TANH

    def __init__(self, eps_min, eps_max):
        if not eps_max > eps_min:
            raise ValueError("TanhParametrization: eps_max must be larger than eps_min")
        self.eps_min, self.eps_max = float(eps_min), float(eps_max)
        self.a = 0.5 * (self.eps_max - self.eps_min)
        self.b = 0.5 * (self.eps_max + self.eps_min)

    def eps(self, u):
        return self.a * np.tanh(np.asarray(u, dtype=np.float64)) + self.b

    def deps_du(self, u):
        t = np.tanh(np.asarray(u, dtype=np.float64))
        return self.a * (1.0 - t * t)

    def u(self, eps, pull=False):
        eps = np.asarray(eps, dtype=np.float64)
        x = (eps - self.b) / self.a
        if pull:
            slack = _ulps(pull) * np.spacing(max(abs(self.eps_min), abs(self.eps_max)))
            near = (eps >= self.eps_min - slack) & (eps <= self.eps_max + slack)
            x = np.where(near, np.clip(x, -_INSIDE, _INSIDE), x)
        bad = ~((x > -1.0) & (x < 1.0))
        if np.any(bad):
            i = _first_bad(bad)
            raise ValueError("value %r at index %d is outside the range (%r, %r) of TanhParametrization"
                             % (float(eps.flat[i]), i, self.eps_min, self.eps_max))
        return np.arctanh(x)


class PulseParameters:
    """What ``optimize_pulses`` carries from sweep to sweep for a parametrized control list: u per control (never
    re-inverted while the pulses stay what the last sweep made them) and the pulses it belongs to."""

    def __init__(self, params, pulses, pull=False):
        self.params = list(params)
        self.L = len(self.params)
        self.u = [None] * self.L
        self.seen = [None] * self.L  # eps the u of a control stands for: a copy, to notice an edited pulse
        self.sync(pulses, pull=pull)

    @property
    def device_kinds(self):
        """``(kind, a, b)`` arrays for ``kh_set_parametrization``, or None when a user-defined subclass takes part."""
        if any(p is not None and p.kind is None for p in self.params):
            return None
        kind = np.array([KH_PAR_NONE if p is None else p.kind for p in self.params], dtype=np.int32)
        a = np.array([0.0 if p is None else p.a for p in self.params], dtype=np.float64)
        b = np.array([0.0 if p is None else p.b for p in self.params], dtype=np.float64)
        return kind, a, b

    def sync(self, pulses, pull=True):
        """Bring u in line with ``pulses``: a control whose pulse is not the one its u stands for (the first call; a
        pulse that ``modify_params_after_iter`` edited) gets u = f^-1(pulse).  Returns the controls re-derived."""
        redone = []
        for l, par in enumerate(self.params):
            eps = np.asarray(pulses[l], dtype=np.float64)
            if self.seen[l] is not None and np.array_equal(self.seen[l], eps):
                continue
            if par is None:
                self.u[l] = eps.copy()
            else:
                try:
                    with np.errstate(all='ignore'):
                        # (a stored pulse may have been through the grid-point form and back: an ulp per interval)
                        slack = max(_ON_BOUND_ULPS, 2 * eps.size) if pull else False
                        u = np.asarray(par.u(eps, pull=slack) if par.kind is not None else par.u(eps), dtype=np.float64)
                except ValueError as exc:
                    raise ValueError("control %d: %s (the index is the time interval)" % (l, exc))
                if u.shape != eps.shape or not np.all(np.isfinite(u)):
                    i = _first_bad(~np.isfinite(u)) if u.shape == eps.shape else 0
                    raise ValueError("control %d: value %r at time interval %d is outside the range of its "
                                     "parametrization" % (l, float(eps.flat[i]), i))
                self.u[l] = u
            self.seen[l] = eps.copy()
            redone.append(l)
        return redone

    def dfdu(self):
        """f'(u) per control, (L, nt-1); 1 for a control without a parametrization."""
        return np.array([np.ones_like(self.u[l]) if par is None else np.asarray(par.deps_du(self.u[l]), dtype=np.float64)
                         for l, par in enumerate(self.params)])

    def eps(self, l, u):
        par = self.params[l]
        return u if par is None else float(par.eps(u))

    def commit(self, u_new, pulses):
        """After a sweep: its u and the pulses f(u) it propagated with."""
        for l in range(self.L):
            self.u[l] = np.array(u_new[l], dtype=np.float64)
            self.seen[l] = np.array(pulses[l], dtype=np.float64)
