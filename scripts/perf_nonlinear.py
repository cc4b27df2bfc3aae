#!/usr/bin/env python3
"""What non-linear controls cost on the update sweep's serial chain (dev tool, GPU only; writes profiles/nonlinear.txt).

    python scripts/perf_nonlinear.py [output file]

Config 5's shape (K = 256, N = 64, nt = 4001), two operator slots, the update sweep by HIP events; ROUNDS rounds, in each
of them, alternating, REPEATS timed launches (after WARMUP untimed ones) of

  (nl)  one control with the terms {eps, eps^2}: kh_tile_forward_update_nl<1, 2, false>;
  (a)   the linear two-control sweep under KH_KERNEL=tile512: kh_tile_forward_update<1, 2, false, true>;
  (b)   the same two controls under TanhParametrization: kh_tile_forward_update_par<1, 2, false>;
  (b')  (b) once more: the difference between (b) and (b') is the spread of the measurement.

Reported per leg: the median over all rounds of the per-round median, in us per interval.  (a) and (b) are code this
feature does not change.  (nl) does strictly less scalar work per interval than (b) -- no tanh -- so it must not be
slower than (b) beyond |(b) - (b')|; its distance from (a) is what the weights and the powers cost.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from krotov_amd import _lib, configs
from krotov_amd.conversions import control_onto_interval, discretize
from krotov_amd.engine import HipKrotovEngine
from krotov_amd.parametrization import PulseParameters, TanhParametrization

WARMUP, REPEATS, ROUNDS = 2, 10, 3
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'nonlinear.txt')
lines = []


def say(text=''):
    print(text, flush=True)
    lines.append(text)


def events_ms(call):
    times = []
    for rep in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


class Leg:
    """One engine on config 5's operators with a second slot, set up for one of the forms; ``time()`` is one round."""

    def __init__(self, label, spec, form):
        self.label, self.form = label, form
        os.environ['KH_KERNEL'] = 'tile512'
        try:
            eng = HipKrotovEngine([[spec.H0[k], spec.Hc[k][0], spec.Hc[k][1]] for k in range(spec.K)], np.diff(spec.tlist),
                                  is_super=spec.is_super)
        finally:
            os.environ.pop('KH_KERNEL', None)
        self.eng, self.nt = eng, len(spec.tlist)
        nt = self.nt
        gp = [control_onto_interval(discretize(c, spec.tlist, args=({},), via_midpoints=True)) for c in spec.controls]
        S = control_onto_interval(discretize(spec.update_shape, spec.tlist, args=(), via_midpoints=True))
        rows = 1 if form == 'nl' else 2
        eps = np.array(gp[:rows])
        terms = np.array([eps[0], eps[0] * eps[0]]) if form == 'nl' else eps
        pulses, shapes = eng.dev(eps, torch.float64), eng.dev(np.array([S] * rows), torch.float64)
        lam = eng.dev(np.full(rows, spec.lambda_a), torch.float64)
        init = eng.dev(spec.init, torch.complex128)
        chi_T = eng.dev(spec.target / np.linalg.norm(spec.target, axis=1)[:, None], torch.complex128)
        norms = eng.dev(np.full(spec.K, 1.0 / spec.K), torch.float64)
        chi = eng.backward(chi_T, terms)
        if form == 'par':
            state = PulseParameters([TanhParametrization(-1.0, 1.0)] * 2, gp[:2])
            kind, a, b = state.device_kinds
            self.u_opt = torch.empty((2, nt - 1), dtype=torch.float64, device=eng.device)
            eng.set_parametrization(kind, a, b, np.array(state.u), state.dfdu(), self.u_opt)
        elif form == 'nl':
            eng.set_nonlinear([0, 0], [1, 2], np.array([np.ones_like(eps[0]), 2.0 * eps[0]]))
        self.args = (chi, norms, init, pulses, shapes, lam)
        self.bufs = eng.forward_update(*self.args)
        eng.check()
        self.us = []

    def time(self):
        _lib.forget_launched_kernels()
        ms = events_ms(lambda: self.eng.forward_update(*self.args, out=self.bufs))
        self.eng.check()
        self.ran = [n for n in _lib.kernel_instantiations(launched_only=True) if 'forward_update' in n]
        self.us.append(1e3 * ms / (self.nt - 1))

    def report(self):
        say('%-5s %-22s %7.3f us per interval  (rounds: %s)   %s' % (
            self.label, {'nl': '{eps, eps^2}', 'linear': 'linear, two controls', 'par': 'Tanh, two controls'}[self.form],
            float(np.median(self.us)), ' '.join('%.3f' % x for x in self.us), ', '.join(self.ran)))
        return float(np.median(self.us))


spec = configs.config_c5(L=2)
say('update sweep with non-linear controls on %s; K = %d, N = %d, nt = %d, two operator slots; events: %d rounds of %d '
    'warm-up + %d timed launches per leg, alternating' % (torch.cuda.get_device_name(0), spec.K, spec.N, len(spec.tlist),
                                                          ROUNDS, WARMUP, REPEATS))
say()
legs = [Leg('(nl)', spec, 'nl'), Leg('(a)', spec, 'linear'), Leg('(b)', spec, 'par'), Leg("(b')", spec, 'par')]
for _ in range(ROUNDS):
    for leg in legs:
        leg.time()
t_nl, t_a, t_b, t_b2 = (leg.report() for leg in legs)
for leg in legs:
    leg.eng.close()
spread = abs(t_b - t_b2)
say()
say("spread |(b) - (b')| = %.3f us per interval" % spread)
say('(nl) - (b) = %+.3f us per interval: %s' % (t_nl - min(t_b, t_b2), 'not slower than (b) beyond the spread'
                                                if t_nl <= max(t_b, t_b2) + spread else 'SLOWER than (b) beyond the spread'))
say('(nl) - (a) = %+.3f us per interval: the weights, the sum over the terms and the powers on the chain' % (t_nl - t_a))

os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
