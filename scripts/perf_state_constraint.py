#!/usr/bin/env python3
"""What a state-dependent constraint costs per iteration (dev tool, GPU only; writes profiles/state_constraint.txt).

    python scripts/perf_state_constraint.py [output file]

Config 5's shape (K = 256, N = 64, nt = 4001, one control), by HIP events (WARMUP untimed and REPEATS timed launches;
reported: the median and min .. max, and the median per interval):

  backward sweep
  (i)   kh_backward_store, the engine's own route (the two-terms-per-phase kernel, kh_q2_sweep_store);
  (ii)  kh_backward_store under KH_KERNEL=tile512 (kh_tile_sweep_store<1, 1>);
  (iii) kh_backward_store_source with a non-zero W (kh_tile_sweep_store_src<1, 1>);
  the kh_apply_store launch that forms W (kh_gen_apply_store);
  update sweep: first order against the second-order kernels with sigma = 0 (the route that stores phi(t_n)).

(iii) is read against (ii) on the same build: if (iii) - (ii) exceeds one series phase of (ii) -- (ii) divided by its
phases per interval, from the engine's matvec count -- the prefetch of the W rows does not hide their latency.
(ii) - (i) is the cost of having no two-terms-per-phase form of the source kernel.
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

WARMUP, REPEATS = 2, 10
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'state_constraint.txt')
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


def engine_of(spec, kernel=None):
    if kernel is not None:
        os.environ['KH_KERNEL'] = kernel
    try:
        return HipKrotovEngine([[spec.H0[k]] + list(spec.Hc[k]) for k in range(spec.K)], np.diff(spec.tlist),
                               is_super=spec.is_super)
    finally:
        os.environ.pop('KH_KERNEL', None)


def report(label, what, eng, ms, nt, match):
    ran = [n for n in _lib.kernel_instantiations(launched_only=True) if match in n]
    say('%-6s %-42s %9.3f ms  (min %.3f .. max %.3f)  %7.3f us per interval   engine "%s", %s' % (
        label, what, ms[0], ms[1], ms[2], 1e3 * ms[0] / (nt - 1), eng.kernel, ', '.join(ran)))
    return 1e3 * ms[0] / (nt - 1)


spec = configs.config_c5()
nt, K, N = len(spec.tlist), spec.K, spec.N
say('state-dependent constraint on %s; K = %d, N = %d, nt = %d, L = %d; events: %d warm-up + %d timed launches' % (
    torch.cuda.get_device_name(0), K, N, nt, spec.L, WARMUP, REPEATS))
say()
gp = [control_onto_interval(discretize(c, spec.tlist, args=({},), via_midpoints=True)) for c in spec.controls]
S = [control_onto_interval(discretize(spec.update_shape, spec.tlist, args=(), via_midpoints=True))] * spec.L
rng = np.random.default_rng(0)
G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
D = (G + G.conj().T) / np.linalg.norm(G + G.conj().T, 2)
factors = np.full(nt, 1.0 / (spec.tlist[-1] - spec.tlist[0]))  # -(lambda_b / T) s_b with lambda_b = -1, s_b = 1

results = {}
for label, kernel in (('(i)', None), ('(ii)', 'tile512')):
    eng = engine_of(spec, kernel)
    pulses = eng.dev(np.array(gp), torch.float64)
    chi_T = eng.dev(spec.target / np.linalg.norm(spec.target, axis=1)[:, None], torch.complex128)
    chi = eng.backward(chi_T, pulses)
    eng.check()
    _lib.forget_launched_kernels()
    ms = events_ms(lambda: eng.backward(chi_T, pulses, out=chi))
    results[label] = report(label, 'kh_backward_store', eng, ms, nt, 'sweep_store')
    phases = eng.stats()['matvecs'] / (K * (nt - 1.0))
    if kernel is not None:
        results['phases'] = phases
        say('       (%.2f series terms per interval and objective)' % phases)
        # (iii) on the same engine: W from its own forward states
        init = eng.dev(spec.init, torch.complex128)
        norms = eng.dev(np.full(K, 1.0 / K), torch.float64)
        _, states = eng.forward(pulses, init, store=True)
        W = torch.empty_like(states)
        eng.apply_store([D] * K, factors, states, out=W)
        eng.check()
        _lib.forget_launched_kernels()
        ms = events_ms(lambda: eng.apply_store([D] * K, factors, states, out=W))
        results['apply'] = report('', 'kh_apply_store (forms W)', eng, ms, nt, 'apply_store')
        eng.backward_source(chi_T, pulses, W, norms, out=chi)
        eng.check()
        _lib.forget_launched_kernels()
        ms = events_ms(lambda: eng.backward_source(chi_T, pulses, W, norms, out=chi))
        results['(iii)'] = report('(iii)', 'kh_backward_store_source, W != 0', eng, ms, nt, 'sweep_store')
        del W, states
    else:
        # the update sweep on the engine's own route: first order against sigma = 0
        init = eng.dev(spec.init, torch.complex128)
        norms = eng.dev(np.full(K, 1.0 / K), torch.float64)
        shapes, lam = eng.dev(np.array(S), torch.float64), eng.dev(np.full(spec.L, spec.lambda_a), torch.float64)
        bufs = eng.forward_update(chi, norms, init, pulses, shapes, lam)
        eng.check()
        _lib.forget_launched_kernels()
        ms = events_ms(lambda: eng.forward_update(chi, norms, init, pulses, shapes, lam, out=bufs))
        eng.check()
        results['fo'] = report('', 'update sweep, first order', eng, ms, nt, 'forward_update')
        _, prev = eng.forward(pulses, init, store=True)
        store = torch.empty_like(prev)
        eng.set_second_order(prev, store, np.zeros(nt - 1))
        eng.forward_update(chi, norms, init, pulses, shapes, lam, out=bufs)
        eng.check()
        _lib.forget_launched_kernels()
        ms = events_ms(lambda: eng.forward_update(chi, norms, init, pulses, shapes, lam, out=bufs))
        eng.check()
        results['so'] = report('', 'update sweep, sigma = 0 (stores phi)', eng, ms, nt, 'forward_update')
        eng.set_second_order()
        del prev, store
    eng.close()
    del chi
    torch.cuda.empty_cache()

say()
phase = results['(ii)'] / results['phases']
say('(iii) - (ii) = %+.3f us per interval; one series phase of (ii) = %.3f us: the prefetch of the W rows %s their latency' % (
    results['(iii)'] - results['(ii)'], phase, 'hides' if results['(iii)'] - results['(ii)'] <= phase else 'does NOT hide'))
say('(ii)  - (i)  = %+.3f us per interval: no two-terms-per-phase form of the source kernel' % (results['(ii)'] - results['(i)']))
say('update sweep, sigma = 0 - first order = %+.3f us per interval: storing phi(t_n) through the second-order kernels' % (
    results['so'] - results['fo']))
say('kh_apply_store = %.3f us per interval (one launch per iteration, off the chain)' % results['apply'])

os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
