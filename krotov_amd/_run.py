"""The run record of one optimisation -- ``Result`` bookkeeping, hook calls and stop verdict (reference
optimize.py:331-389, 503-590) --, which ``optimize_pulses`` holds one of and every replica of ``optimize_pulses_batch``
is one of, and the host side of the boundary co-states, which both form the same way.  No device work here."""
import copy
import logging
import time

import numpy as np

from .conversions import pulse_onto_tlist
from .info_hooks import chain
from .result import Result


def default_norm(state):
    """The ``norm`` of ``optimize_pulses`` when the caller gives none."""
    return state.norm() if hasattr(state, 'norm') else float(np.linalg.norm(np.asarray(state)))


def chained_hook(modify_params_after_iter, info_hook):
    """The one hook a driver calls per iteration: ``modify_params_after_iter`` first, then ``info_hook``."""
    if modify_params_after_iter is None:
        return info_hook
    return modify_params_after_iter if info_hook is None else chain(modify_params_after_iter, info_hook)


def host_costates(chi_constructor, norm, to_vector, **kwargs):
    """``chi_constructor(**kwargs)`` on the host: ``(chi_states, chi_norms, vectors)`` -- the normalised co-states, their
    norms, and ``to_vector(chi, k)`` of each, the form the backend's sweeps take (None from it: wrong dimension)."""
    chi_states = chi_constructor(**kwargs)
    chi_norms = [norm(chi) for chi in chi_states]
    chi_states = [chi / nrm for chi, nrm in zip(chi_states, chi_norms)]
    vectors = [to_vector(chi, k) for k, chi in enumerate(chi_states)]
    if any(v is None for v in vectors):
        raise ValueError("chi_constructor returned states that do not match the state dimension")
    return chi_states, chi_norms, vectors


class RunRecord:
    """One optimisation's ``Result`` and what decides how it is filled and when it ends.  ``static_args``: the keyword
    arguments every hook call gets, ``iter_start`` and ``iter_stop`` among them -- a hook may change ``iter_stop``
    there; the loop's own bound (``range_stop``) is fixed here, at the start."""

    def __init__(self, static_args, continue_from=None, store_all_pulses=False, info_hook=None, check_convergence=None):
        self.static_args = static_args
        self.iter_start, self.range_stop = static_args['iter_start'], static_args['iter_stop']
        self.continue_from, self.store_all_pulses = continue_from, store_all_pulses
        self.info_hook, self.check_convergence = info_hook, check_convergence
        self.result = Result() if continue_from is None else copy.deepcopy(continue_from)
        if continue_from is None:
            self.result.start_local_time = time.localtime()

    def _append(self, iteration, seconds, info, tau_vals, pulses):
        result = self.result
        result.iters.append(iteration)
        result.iter_seconds.append(int(seconds))
        if info is not None:
            result.info_vals.append(info)
        if not np.all(tau_vals == None):  # noqa: E711
            result.tau_vals.append(tau_vals)
        if self.store_all_pulses:
            result.all_pulses.append(pulses)

    def record_initial(self, guess_controls, pulses_mapping, guess_pulses, optimized_pulses, g_a_integrals, fw_states_T,
                       tau_vals, forward_states, tic, toc):
        """Iteration 0: the hook sees the propagation under the guess (the states under "optimized" and guess pulses
        coincide); a run that continues another appends nothing and goes on from that run's last iteration."""
        info = None
        if self.info_hook is not None:
            info = self.info_hook(
                backward_states=None, forward_states=forward_states, forward_states0=forward_states,
                guess_pulses=guess_pulses, optimized_pulses=optimized_pulses, g_a_integrals=g_a_integrals,
                fw_states_T=fw_states_T, tau_vals=tau_vals, start_time=tic, stop_time=toc, iteration=0, info_vals=[],
                shared_data={}, **self.static_args,
            )
        result = self.result
        result.tlist, result.objectives = self.static_args['tlist'], self.static_args['objectives']
        result.guess_controls = guess_controls
        result.optimized_controls = optimized_pulses
        result.controls_mapping = pulses_mapping
        result.states = fw_states_T
        if self.continue_from is None:
            self._append(0, toc - tic, info, tau_vals, guess_pulses)
        else:
            self.iter_start = self.continue_from.iters[-1]
            logging.getLogger('krotov').info("Continuing from previous result, with iteration %d", self.iter_start + 1)

    def record_iteration(self, iteration, backward_states, forward_states, forward_states0, fw_states_T, guess_pulses,
                         optimized_pulses, g_a_integrals, tau_vals, tic, toc):
        """A finished iteration: the hook call, then the appends."""
        info = None
        if self.info_hook is not None:
            info = self.info_hook(
                backward_states=backward_states, forward_states=forward_states, forward_states0=forward_states0,
                fw_states_T=fw_states_T, guess_pulses=guess_pulses, optimized_pulses=optimized_pulses,
                g_a_integrals=g_a_integrals, tau_vals=tau_vals, start_time=tic, stop_time=toc,
                info_vals=self.result.info_vals, shared_data={}, iteration=iteration, **self.static_args,
            )
        self._append(iteration, toc - tic, info, tau_vals,
                     copy.deepcopy(optimized_pulses) if self.store_all_pulses else None)
        self.result.optimized_controls = optimized_pulses
        self.result.states = fw_states_T

    def convergence(self):
        """What ``check_convergence`` says to the Result as recorded so far (None without one)."""
        return None if self.check_convergence is None else self.check_convergence(self.result)

    def verdict(self, iteration, msg=None):
        """Whether the run goes on behind ``iteration``; if not, ``result.message`` says why.  Behind a recorded iteration
        (``msg``: what :meth:`convergence` said to it) ``static_args['iter_stop']``, which a hook may have changed, goes
        before convergence; then, and alone behind the iteration a run starts from, the loop's own end (the for-else)."""
        result = self.result
        if iteration > self.iter_start and iteration >= self.static_args['iter_stop']:
            result.message = "Reached %d iterations" % self.static_args['iter_stop']
        elif iteration > self.iter_start and bool(msg) is True:
            result.message = "Reached convergence" + (": " + msg if isinstance(msg, str) else "")
        elif iteration + 1 > self.range_stop:
            result.message = "Reached %d iterations" % max(self.iter_start, self.range_stop)
        else:
            return True
        return False

    def finish(self, optimized_pulses):
        """What follows the loop (reference optimize.py:583-590); the Result is not touched afterwards."""
        from .optimize import _LazyStates  # (imports this module)

        self.result.end_local_time = time.localtime()
        self.result.optimized_controls = [pulse_onto_tlist(np.asarray(p)) for p in optimized_pulses]
        if isinstance(self.result.states, _LazyStates):
            self.result.states = list(self.result.states)
