#!/usr/bin/env python3
"""Measure ``optimize_pulses_batch`` (kernel family "replica16/wave") against the loop of ``optimize_pulses`` it replaces.

    python scripts/perf_replicas.py                # the batch: B = 1, 64, 256, 1024, 4096 -> profiles/replicas.txt
    python scripts/perf_replicas.py --loop 8       # the yardstick: 8 of the same problems one after another (this mode
                                                   # uses nothing but optimize_pulses: it runs on the parent commit too)

Two shapes: config 3's (``configs.config_c3()``: K_r = 4, N = 4, nt = 2001, one control) and a two-control problem with
N = 16, K_r = 4, nt = 501.  The replicas differ in their guess amplitude and in lambda_a (a scan).  Per shape and B:
ms per Krotov iteration of the whole batch from HIP events around the two sweeps (KH_PROFILE) and from the wall clock
between two iterations inside the call (after a warm-up call), the update kernel's resident workgroups per CU
(hipOccupancyMaxActiveBlocksPerMultiprocessor) and the batch's whole wall time including its set-up.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('KH_PROFILE', '1')

import numpy as np  # noqa: E402


def problems_of(shape, B):
    """B problems of one shape: arrays as guess controls (amplitude scanned), lambda_a scanned, update_shape 1."""
    import krotov_amd
    from krotov_amd import configs

    spec = configs.config_c3() if shape == 'c3' else configs.config_c5(K=4, N=16, nt=501, L=2, distinct=True, seed=5)
    tl = spec.tlist
    base = [np.array([c(t, None) for t in tl]) for c in spec.controls]
    out = []
    for b in range(B):
        amp = 0.5 + (b % 97) / 97.0
        controls = [amp * g for g in base]
        objectives = [krotov_amd.Objective(initial_state=spec.init[k].reshape(-1, 1), target=spec.target[k].reshape(-1, 1),
                                           H=[spec.H0[k]] + [[spec.Hc[k][l], controls[l]] for l in range(spec.L)])
                      for k in range(spec.K)]
        lam = spec.lambda_a * (1.0 + 0.01 * (b % 89))
        out.append(dict(objectives=objectives, tlist=tl,
                        pulse_options={id(c): dict(lambda_a=lam, update_shape=1) for c in controls}))
    return out, spec


class Clock:
    """info_hook: wall-clock stamps of the first problem's iterations."""

    def __init__(self, first_objectives):
        self.first, self.stamps = first_objectives, []

    def __call__(self, **kw):
        if kw['objectives'] is self.first:
            self.stamps.append(time.perf_counter())


def shared():
    import krotov_amd

    return dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_re)


def measure_batch(shape, B, iters):
    import torch

    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    problems, spec = problems_of(shape, B)
    krotov_amd.optimize_pulses_batch(problems[:min(B, 2)], iter_stop=1, **shared())  # warm-up (library, allocator)
    torch.cuda.synchronize()
    clock = Clock(problems[0]['objectives'])
    t0 = time.perf_counter()
    krotov_amd.optimize_pulses_batch(problems, iter_stop=iters, info_hook=clock, **shared())
    torch.cuda.synchronize()
    wall_all = time.perf_counter() - t0
    eng = LAST_ENGINE()
    assert eng.kernel == 'replica16/wave', eng.kernel
    ev = eng.kernel_times_ms()
    sweeps = (np.median(ev['backward']) + np.median(ev['update'])) if ev['update'] else float('nan')
    per_iter = np.diff(clock.stamps)  # (between the hook calls of consecutive iterations; the first follows the set-up)
    return dict(shape=shape, B=B, K_r=spec.K, N=spec.N, L=spec.L, nt=len(spec.tlist), sweeps_ms=float(sweeps),
                backward_ms=float(np.median(ev['backward'])), update_ms=float(np.median(ev['update'])),
                wall_iter_ms=1e3 * float(np.median(per_iter[1:])) if len(per_iter) > 1 else float('nan'),
                wall_all_s=wall_all, occupancy=occupancy_of(spec))


def occupancy_of(spec):
    """Resident workgroups per CU of the update kernel for this shape (a one-replica engine is asked)."""
    from krotov_amd.engine import HipKrotovEngine

    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), is_super=spec.is_super, replicas=1)
    try:
        return eng.replica_occupancy()
    finally:
        eng.close()


def measure_loop(shape, n, iters):
    import torch

    import krotov_amd

    problems, spec = problems_of(shape, n)
    krotov_amd.optimize_pulses(problems[0]['objectives'], problems[0]['pulse_options'], spec.tlist, iter_stop=1, **shared())
    torch.cuda.synchronize()
    per_iter, t0 = [], time.perf_counter()
    for p in problems:
        clock = Clock(p['objectives'])
        krotov_amd.optimize_pulses(p['objectives'], p['pulse_options'], p['tlist'], iter_stop=iters, info_hook=clock, **shared())
        per_iter += list(np.diff(clock.stamps)[1:])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return dict(shape=shape, n=n, iter_ms=1e3 * float(np.median(per_iter)), problem_s=wall / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,64,256,1024,4096')
    ap.add_argument('--shapes', default='c3,n16l2')
    ap.add_argument('--iters', type=int, default=4)
    ap.add_argument('--loop', type=int, default=0, help="time this many problems as a loop of optimize_pulses instead")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'replicas.txt'))
    args = ap.parse_args()
    import torch

    lines = ["# scripts/perf_replicas.py on %s, %d CUs" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count)]
    for shape in args.shapes.split(','):
        if args.loop:
            r = measure_loop(shape, args.loop, args.iters)
            lines.append("loop   %-6s n %4d: %8.3f ms per iteration and problem, %8.4f s per problem with its set-up "
                         "(scaled: B problems take B times that)" % (r['shape'], r['n'], r['iter_ms'], r['problem_s']))
            print(lines[-1], flush=True)
            continue
        for B in [int(x) for x in args.batches.split(',')]:
            r = measure_batch(shape, B, args.iters)
            lines.append("batch  %-6s K_r %d N %2d L %d nt %4d  B %5d: sweeps %9.3f ms per iteration (backward %8.3f + update %8.3f, "
                         "HIP events), wall %9.3f ms per iteration, %7.2f s for the whole call; update kernel: %s workgroups per CU"
                         % (r['shape'], r['K_r'], r['N'], r['L'], r['nt'], r['B'], r['sweeps_ms'], r['backward_ms'],
                            r['update_ms'], r['wall_iter_ms'], r['wall_all_s'], r['occupancy']))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a' if args.loop else 'w') as f:
        f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
