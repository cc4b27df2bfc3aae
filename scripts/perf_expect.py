#!/usr/bin/env python3
"""Device-side expectation values (kh_expect, kh_expect.h) and the batched propagation built on them (dev tool, GPU only;
writes profiles/expect.txt).

    python scripts/perf_expect.py [output file]

Two shapes: config 5's (Hilbert space, K = 256, N = 64, nt = 4001) and config 4's (Liouville space, K = 16, N = 400,
nt = 1001), n_e = 2 operators each.  Per shape:

  * the kh_expect time by HIP events, next to the kh_forward_store time of the same engine (WARMUP untimed and REPEATS
    timed launches each; reported: the median and min .. max);
  * the bytes and flops of kh_expect.h's header comment and the fraction of each bound the median reaches, against
    HBM_TBS and FP64_MATRIX_TFLOPS below (the MI355X's public peak figures);
  * the wall time of ``propagate_objectives`` (one untimed call, then WALL_REPEATS timed ones, the median) against the
    per-objective way of getting the same numbers -- the loop of ``Objective.propagate(..., e_ops=...)``, timed on
    LOOP_OBJECTIVES objectives (after one untimed call) and scaled to K.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import krotov_amd
from krotov_amd import configs
from krotov_amd.engine import HipKrotovEngine

WARMUP, REPEATS, WALL_REPEATS, LOOP_OBJECTIVES = 2, 10, 3, 8
HBM_TBS, FP64_MATRIX_TFLOPS = 8.0, 78.6
N_E = 2
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'expect.txt')
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


def kernels(name, spec, side):
    K, N, nt = spec.K, spec.init.shape[1], len(spec.tlist)
    rng = np.random.default_rng(1)
    eng = HipKrotovEngine([[spec.H0[k]] + list(spec.Hc[k]) for k in range(K)], np.diff(spec.tlist), is_super=spec.is_super)
    pulses, init = eng.dev(pulses_of(spec), torch.float64), eng.dev(spec.init, torch.complex128)
    _, states = eng.forward(pulses, init, store=True)
    G = rng.standard_normal((side, side)) + 1j * rng.standard_normal((side, side))
    ops = [G + G.conj().T, G]
    outbuf = eng.expect(states, ops)
    fw = events_ms(lambda: eng.forward(pulses, init, store=True))
    ex = events_ms(lambda: eng.expect(states, ops, out=outbuf))
    nbytes = 16.0 * K * nt * N
    flops = 0.0 if spec.is_super else 8.0 * N * N * N_E * K * nt
    say('%s: K = %d, N = %d, nt = %d, n_e = %d, engine "%s"' % (name, K, N, nt, N_E, eng.kernel))
    say('  kh_forward_store  %9.3f ms  (min %.3f .. max %.3f)' % fw)
    say('  kh_expect         %9.3f ms  (min %.3f .. max %.3f)' % ex)
    t_mem, t_mma = nbytes / (HBM_TBS * 1e12) * 1e3, flops / (FP64_MATRIX_TFLOPS * 1e12) * 1e3
    say('  store read once: %.1f MB = %.3f ms at %.1f TB/s -> %.1f %% of the memory bound' % (
        nbytes / 1e6, t_mem, HBM_TBS, 100.0 * t_mem / ex[0]))
    if flops:
        say('  8 N^2 n_e K nt = %.2f GFLOP = %.3f ms at %.1f TFLOP/s -> %.1f %% of the fp64 MFMA bound' % (
            flops / 1e9, t_mma, FP64_MATRIX_TFLOPS, 100.0 * t_mma / ex[0]))
    say('  fraction of max(bounds): %.1f %%' % (100.0 * max(t_mem, t_mma) / ex[0]))
    eng.close()
    return ops


def wall(name, objectives, tlist, propagator, ops):
    K = len(objectives)
    call = lambda: krotov_amd.propagate_objectives(objectives, tlist, propagator=propagator, e_ops=ops)  # noqa: E731
    call()
    times = []
    for _ in range(WALL_REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    batched = float(np.median(times))
    few = objectives[:LOOP_OBJECTIVES]
    few[0].propagate(tlist, propagator=propagator, e_ops=ops)
    t0 = time.perf_counter()
    ref = [obj.propagate(tlist, propagator=propagator, e_ops=ops) for obj in few]
    loop = (time.perf_counter() - t0) / len(few)
    err = max(float(np.abs(res[k].expect[i] - ref[k].expect[i]).max()) for k in range(len(few)) for i in range(N_E))
    say('  propagate_objectives, %d objectives:            %9.3f s  (median of %d)' % (K, batched, WALL_REPEATS))
    say('  loop of Objective.propagate: %.4f s per objective (timed on %d) x %d = %9.3f s  -> %.1fx' % (
        loop, len(few), K, loop * K, loop * K / batched))
    say('  largest difference of the two on those %d objectives: %.2e' % (len(few), err))
    say()


say('kh_expect and propagate_objectives on %s; events: %d warm-up + %d timed launches' % (
    torch.cuda.get_device_name(0), WARMUP, REPEATS))
say()
spec = configs.config_c5()
ops = kernels('Hilbert space (config 5)', spec, spec.init.shape[1])
objectives, _ = configs.spec_to_objectives(spec, krotov_amd)
wall('Hilbert space', objectives, spec.tlist, krotov_amd.propagators.expm, ops)

spec = configs.config_c4()
d = int(round(np.sqrt(spec.init.shape[1])))
ops = kernels('Liouville space (config 4)', spec, d)
objectives = [krotov_amd.Objective(initial_state=spec.init[k].reshape(d, d, order='F'),
                                   target=spec.target[k].reshape(d, d, order='F'),
                                   H=[spec.H0[k], [spec.Hc[k][0], spec.controls[0]]]) for k in range(spec.K)]
wall('Liouville space', objectives, spec.tlist, krotov_amd.propagators.HipExpm(liouville=True), ops)

os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
