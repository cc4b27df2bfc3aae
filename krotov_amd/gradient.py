"""The exact gradient of the final-time functional for the pulse values, on the device.

Krotov's method converges monotonically but slowly near the optimum; the reference's own advice ("Krotov vs GRAPE") is
to hand its pulses to a quasi-Newton method on the gradient of the time-discretised functional,

    dJ_T/d eps_l[n] = -2 sum_k Re < chi_k(t_{n+1}) | d exp(f A_kn dt_n)/d eps_l[n] | phi_k(t_n) >,

with phi and chi propagated under the SAME pulses and chi_k(T) = -dJ_T/d<phi_k(T)| from the ``chi_constructor``.  The
update sum of Krotov's method is only the first order in dt of this; :class:`PulseGradient` evaluates it exactly (the
Frechet derivative of the matrix exponential, ``kh_pulse_gradient``: krotov_amd/csrc/kh_grad.h)::

    pg = krotov_amd.PulseGradient(objectives, pulse_options, tlist, propagator=expm, chi_constructor=chis_ss, J_T=J_T_ss)
    x0 = numpy.concatenate(result_pulses_on_the_intervals)
    res = scipy.optimize.minimize(pg.value_and_gradient, x0, jac=True, method='L-BFGS-B')

Running costs (g_a, g_b) are not part of the gradient, and there is no optimiser here: SciPy's is the user's.
"""
import logging

import numpy as np

from . import _run
from . import functionals as _functionals
from .mixed import layout_of
from .nonlinear import term_plan
from .optimize import _HipBackend, _device_costates, _initialize_krotov_controls, _parametrizations
from .propagators import HipExpm, expm

__all__ = ['PulseGradient', 'GradientResult']

# the limits of kh_pulse_gradient (krotov_amd/csrc/kh_grad.h: KH_GRAD_NMAX, KH_GRAD_MAX_L)
GRADIENT_NMAX, GRADIENT_LMAX = 96, 4


class GradientResult:
    """What one evaluation returns: ``gradient`` (a list of L arrays on the nt - 1 intervals, dJ_T/d eps_l[n]),
    ``fw_states_T`` (the states phi_k(T)), ``tau_vals`` and ``J_T`` (None without a ``J_T`` callable)."""

    def __init__(self, gradient, fw_states_T, tau_vals, J_T):
        self.gradient = gradient
        self.fw_states_T = fw_states_T
        self.tau_vals = tau_vals
        self.J_T = J_T


def _refusal(objectives, propagator, process_group):
    """Why the device cannot differentiate this problem (a black-box propagator has no derivative, so there is no host
    loop to fall back on), or None."""
    props = propagator if isinstance(propagator, list) else [propagator]
    if not props or any(not (p is expm or isinstance(p, HipExpm)) for p in props):
        return "the gradient needs propagator=krotov_amd.propagators.expm / HipExpm (a propagator of your own has no derivative)"
    if any(isinstance(p, HipExpm) and getattr(p, 'sparse', False) for p in props):
        return "the gradient serves dense operators, not HipExpm(sparse=True)"
    if process_group is not None:
        return "the gradient runs on one GPU: process_group= (sharding) is not supported"
    if any(len(obj.c_ops) > 0 for obj in objectives):
        return "the gradient is not implemented for objectives with c_ops (Lindblad form)"
    layout = layout_of(objectives, propagator)
    if layout.mixed:
        return "the gradient needs objectives of one dimension and kind (mixed lists are not supported)"
    if layout.stride > GRADIENT_NMAX:
        return "state dimension N = %d: the gradient serves N <= %d" % (layout.stride, GRADIENT_NMAX)
    return None


class PulseGradient:
    """``dJ_T/d eps_l[n]`` of the objectives' final-time functional for piecewise-constant pulses, evaluated on the GPU.

    ``objectives``, ``pulse_options``, ``tlist``, ``propagator`` and ``chi_constructor`` are those of
    :func:`krotov_amd.optimize_pulses`; the controls are discretised in the same way and ONE engine is built, which
    every call reuses.  ``J_T(fw_states_T, objectives, tau_vals=...)`` is optional (``.J_T`` of the result,
    :meth:`value_and_gradient`).

    Per call: forward sweep with storage, ``kh_tau``, the boundary co-states (on the device for the built-in ``chis_*``,
    else ``chi_constructor`` on the host), backward sweep under the same pulses, ``kh_pulse_gradient``.

    Non-linear controls (:class:`~krotov_amd.nonlinear.Power`) are differentiated by the chain rule over their terms.
    The gradient is for eps: a ``'parametrization'`` in ``pulse_options`` is ignored -- d/du = f'(u) d/d eps
    (:meth:`Parametrization.deps_du`) is the caller's.  ``NotImplementedError`` for what the device cannot
    differentiate: another propagator, ``c_ops``, mixed lists, ``process_group``, N > 96, more than 4 terms.
    """

    def __init__(self, objectives, pulse_options, tlist, *, propagator, chi_constructor, J_T=None, process_group=None):
        logger = logging.getLogger('krotov')
        reason = _refusal(objectives, propagator, process_group)
        if reason is not None:
            raise NotImplementedError(reason)
        self.objectives = objectives
        self.tlist = np.asarray(tlist, dtype=np.float64)
        self.chi_constructor = chi_constructor
        self.J_T_func = J_T
        _, self.guess_pulses, pulses_mapping, _, _ = _initialize_krotov_controls(objectives, pulse_options, tlist)
        self.n_controls = len(self.guess_pulses)
        plan = term_plan(objectives, pulses_mapping, self.n_controls)
        if plan is False:
            raise NotImplementedError("a ControlFunction that is no integer power (power None) has no derivative on the device")
        n_terms = self.n_controls if plan is None else plan.J
        if n_terms > GRADIENT_LMAX:
            raise NotImplementedError("%d control terms: the gradient serves at most %d" % (n_terms, GRADIENT_LMAX))
        if n_terms < 1:
            raise ValueError("the objectives contain no control")
        if _parametrizations(objectives, pulse_options) is not None:
            logger.info("PulseGradient: 'parametrization' in pulse_options is ignored -- the gradient is for eps; "
                        "d/du = f'(u) d/d eps (Parametrization.deps_du) is the caller's chain rule")
        self._backend = _HipBackend(objectives, pulses_mapping, tlist, self.n_controls, propagator)
        self._plan = plan
        self._chi_store = None
        self._grad = None

    # -- one evaluation ---------------------------------------------------------
    def __call__(self, pulses=None):
        """The gradient under ``pulses`` (a list of L arrays on the nt - 1 intervals; default: the guess)."""
        be = self._backend
        t, eng = be.torch, be.engine
        nI = len(self.tlist) - 1
        if pulses is None:
            pulses = self.guess_pulses
        pulses = [np.asarray(p, dtype=np.float64) for p in pulses]
        if len(pulses) != self.n_controls or any(p.shape != (nI,) for p in pulses):
            raise ValueError("pulses: %d arrays of %d interval values each" % (self.n_controls, nI))
        eps = be._pulses(pulses)
        terms = be._terms(eps)
        fw_states_T, _ = be.initial_forward(pulses, store=True)
        tau_vals = be.tau_vals(fw_states_T)
        chi_coef, chi_li = _device_costates(be, self.chi_constructor, tau_vals)
        chi_T = chi_norms = None
        if chi_coef is None and chi_li is None:
            _, chi_norms, chi_T = _run.host_costates(
                self.chi_constructor, _run.default_norm, be.state_vector, fw_states_T=fw_states_T,
                objectives=self.objectives, tau_vals=tau_vals)
        chi_loc, norms_loc, li_J = be._boundary_costates(chi_T, chi_norms, chi_coef, chi_li)
        self._chi_store = eng.backward(chi_loc, terms, out=self._chi_store)
        self._grad = eng.pulse_gradient(be.fw_prev, self._chi_store, norms_loc, terms, out=self._grad)
        grad = self._grad
        if self._plan is not None:
            # eps^p terms: d/d eps_c = sum_j p_j eps_c^(p_j - 1) g_j over the terms j of control c
            rows = eps.index_select(0, be._nl_rows)
            w = be._nl_pow.expand_as(rows)
            for q in range(1, 4):
                w = t.where(be._nl_pow - 1 >= q, w * rows, w)
            grad = t.zeros_like(eps).index_add_(0, be._nl_rows, w * grad)
        if chi_li is not None:
            chi_li.set_device_values(li_J.cpu().numpy())
        host = grad.cpu().numpy()
        J = None
        if self.J_T_func is not None:
            J = self.J_T_func(fw_states_T, self.objectives, tau_vals=tau_vals)
        return GradientResult([host[l].copy() for l in range(self.n_controls)], fw_states_T, tau_vals, J)

    def value_and_gradient(self, x):
        """``(J_T, gradient)`` for the flat float64 vector ``x`` of all pulse values, control after control -- the form
        ``scipy.optimize.minimize(..., jac=True)`` takes.  Needs ``J_T``."""
        if self.J_T_func is None:
            raise ValueError("value_and_gradient needs the J_T callable")
        nI = len(self.tlist) - 1
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (self.n_controls * nI,):
            raise ValueError("x: a flat vector of %d values" % (self.n_controls * nI))
        res = self([x[l * nI:(l + 1) * nI] for l in range(self.n_controls)])
        return float(res.J_T), np.concatenate(res.gradient).astype(np.float64)
