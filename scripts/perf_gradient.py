#!/usr/bin/env python3
"""The exact pulse gradient (kh_pulse_gradient, kh_grad.h) next to the two plain sweeps of the same engine (dev tool, GPU
only; writes profiles/gradient.txt).

    python scripts/perf_gradient.py [output file]

Config 5's shape (K = 256, N = 64, nt = 4001) with L = 1 and L = 2.  Per shape, in one run:

  * kh_pulse_gradient by HIP events (WARMUP untimed and REPEATS timed launches; the median and min .. max);
  * kh_forward_store and kh_backward_store of the same engine in the same way, their sum and the ratio to it -- nothing
    comparable exists to compare with, so the two sweeps that feed the gradient are the yardstick;
  * the flops the kernel executes -- 8 Np^2 (1 + L)^2 per term and column, Np = N rounded up to 16, with the terms
    s (m + 1) of every group of sixteen intervals as the kernel chooses them (the largest theta of the group) -- and the
    fraction of FP64_TFLOPS (the MI355X's public fp64 vector = matrix peak) the median reaches.
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from krotov_amd import _lib, configs
from krotov_amd.engine import HipKrotovEngine

WARMUP, REPEATS = 2, 10
FP64_TFLOPS = 78.6
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'gradient.txt')
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


def pulses_of(spec):
    from krotov_amd.conversions import control_onto_interval, discretize

    return np.array([control_onto_interval(discretize(c, spec.tlist, args=({},))) for c in spec.controls])


def executed_terms(eng, pulses, dt):
    """sum over the objectives and groups of sixteen intervals of 16 s (m + 1): the kernel's own choice, restated."""
    th, ra = (ctypes.c_double * 65)(), (ctypes.c_double * (65 * 65))()
    assert _lib.load().kh_series_tables(0, 0.0, th, ra) == 0
    tab = np.array(th)
    theta = dt[None, :] * (eng.op_norms[:, :1] + eng.op_norms[:, 1:] @ np.abs(pulses))  # (K, nt-1)
    pad = (-theta.shape[1]) % 16
    top = np.pad(theta, ((0, 0), (0, pad))).reshape(theta.shape[0], -1, 16).max(axis=2)
    s = np.where(top > 1.0, np.ceil(top), 1.0)
    m = np.searchsorted(tab[1:], top / s, side='left') + 1
    return float((16.0 * s * (np.minimum(m, 64) + 1)).sum())


def shape(L):
    spec = configs.config_c5(L=L)
    K, N, nt = spec.K, spec.init.shape[1], len(spec.tlist)
    eng = HipKrotovEngine([[spec.H0[k]] + list(spec.Hc[k]) for k in range(K)], np.diff(spec.tlist), is_super=spec.is_super)
    host_pulses = pulses_of(spec)
    pulses, init = eng.dev(host_pulses, torch.float64), eng.dev(spec.init, torch.complex128)
    psi_T, fw = eng.forward(pulses, init, store=True)
    chi_T, norms = eng.chi_boundary(eng.dev(spec.target, torch.complex128), psi_T,
                                    eng.dev(np.full(K, 0.5 / K), torch.complex128), eng.dev(np.zeros(K), torch.complex128))
    chi = eng.backward(chi_T, pulses)
    grad = eng.pulse_gradient(fw, chi, norms, pulses)
    t_fw = events_ms(lambda: eng.forward(pulses, init, store=True, out=(psi_T, fw)))
    t_bw = events_ms(lambda: eng.backward(chi_T, pulses, out=chi))
    t_g = events_ms(lambda: eng.pulse_gradient(fw, chi, norms, pulses, out=grad))
    Np = 16 * ((N + 15) // 16)
    terms = executed_terms(eng, host_pulses, np.diff(spec.tlist))
    flops = 8.0 * Np * Np * (1 + L) ** 2 * terms
    say('config 5, L = %d: K = %d, N = %d, nt = %d, engine "%s"' % (L, K, N, nt, eng.kernel))
    say('  kh_forward_store   %9.3f ms  (min %.3f .. max %.3f)' % t_fw)
    say('  kh_backward_store  %9.3f ms  (min %.3f .. max %.3f)' % t_bw)
    say('  kh_pulse_gradient  %9.3f ms  (min %.3f .. max %.3f)' % t_g)
    say('  gradient / (forward + backward) = %.2f' % (t_g[0] / (t_fw[0] + t_bw[0])))
    say('  %.3e terms x columns, %.2f TFLOP executed -> %.1f TFLOP/s = %.1f %% of the fp64 peak (%.1f TFLOP/s)' % (
        terms, flops / 1e12, flops / 1e12 / (t_g[0] * 1e-3), 100.0 * flops / 1e12 / (t_g[0] * 1e-3) / FP64_TFLOPS, FP64_TFLOPS))
    say('  largest |gradient| %.3e' % float(grad.abs().max()))
    say()
    eng.close()


say('kh_pulse_gradient on %s; events: %d warm-up + %d timed launches' % (torch.cuda.get_device_name(0), WARMUP, REPEATS))
say()
for L in (1, 2):
    shape(L)
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
