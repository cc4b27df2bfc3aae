#!/usr/bin/env python3
"""What a pulse parametrization costs on the update sweep's serial chain (dev tool, GPU only; writes
profiles/parametrization.txt).

    python scripts/perf_parametrization.py [output file]

Config 5's shape (K = 256, N = 64, nt = 4001, one control), the update sweep by HIP events (WARMUP untimed and REPEATS
timed launches; reported: the median and min .. max, and the median per interval):

  (i)   unparametrized, the engine's own route (the two-terms-per-phase kernel, kh_q2_forward_update);
  (ii)  unparametrized under KH_KERNEL=tile512 (kh_tile_forward_update<1, 1, false, true>);
  (iii) TanhParametrization on the new route (kh_tile_forward_update_par<1, 1, false>).

(iii) - (ii) is the cost of f on the chain; (ii) - (i) is the cost of not having a two-terms-per-phase form of it.
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

WARMUP, REPEATS = 2, 10
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'parametrization.txt')
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
    return float(np.median(times)), min(times), max(times)


def update_sweep(label, spec, kernel=None, par=None):
    if kernel is not None:
        os.environ['KH_KERNEL'] = kernel
    try:
        eng = HipKrotovEngine([[spec.H0[k]] + list(spec.Hc[k]) for k in range(spec.K)], np.diff(spec.tlist),
                              is_super=spec.is_super)
    finally:
        os.environ.pop('KH_KERNEL', None)
    nt = len(spec.tlist)
    gp = [control_onto_interval(discretize(c, spec.tlist, args=({},), via_midpoints=True)) for c in spec.controls]
    S = [control_onto_interval(discretize(spec.update_shape, spec.tlist, args=(), via_midpoints=True))] * spec.L
    pulses, shapes = eng.dev(np.array(gp), torch.float64), eng.dev(np.array(S), torch.float64)
    lam = eng.dev(np.full(spec.L, spec.lambda_a), torch.float64)
    init = eng.dev(spec.init, torch.complex128)
    chi_T = eng.dev(spec.target / np.linalg.norm(spec.target, axis=1)[:, None], torch.complex128)
    norms = eng.dev(np.full(spec.K, 1.0 / spec.K), torch.float64)
    chi = eng.backward(chi_T, pulses)
    if par is not None:
        state = PulseParameters([par] * spec.L, gp)
        kind, a, b = state.device_kinds
        u_opt = torch.empty((spec.L, nt - 1), dtype=torch.float64, device=eng.device)
        eng.set_parametrization(kind, a, b, np.array(state.u), state.dfdu(), u_opt)
    bufs = eng.forward_update(chi, norms, init, pulses, shapes, lam)
    eng.check()
    _lib.forget_launched_kernels()
    ms = events_ms(lambda: eng.forward_update(chi, norms, init, pulses, shapes, lam, out=bufs))
    eng.check()
    ran = [n for n in _lib.kernel_instantiations(launched_only=True) if 'forward_update' in n]
    say('%-6s %-34s %9.3f ms  (min %.3f .. max %.3f)  %7.3f us per interval   engine "%s", %s' % (
        label, 'unparametrized' if par is None else type(par).__name__, ms[0], ms[1], ms[2], 1e3 * ms[0] / (nt - 1),
        eng.kernel, ', '.join(ran)))
    eng.close()
    return 1e3 * ms[0] / (nt - 1)


spec = configs.config_c5()
say('update sweep with and without a pulse parametrization on %s; K = %d, N = %d, nt = %d, L = %d; events: %d warm-up + %d '
    'timed launches' % (torch.cuda.get_device_name(0), spec.K, spec.N, len(spec.tlist), spec.L, WARMUP, REPEATS))
say()
t1 = update_sweep('(i)', spec)
t2 = update_sweep('(ii)', spec, kernel='tile512')
t3 = update_sweep('(iii)', spec, par=TanhParametrization(-1.0, 1.0))
say()
say('(iii) - (ii) = %+.3f us per interval: f on the serial chain' % (t3 - t2))
say('(ii)  - (i)  = %+.3f us per interval: no two-terms-per-phase form of the parametrized kernel' % (t2 - t1))

os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
