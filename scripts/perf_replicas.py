#!/usr/bin/env python3
"""Measure ``optimize_pulses_batch`` (kernel family "replica16/wave") against the loop of ``optimize_pulses`` it replaces.

    python scripts/perf_replicas.py                # the batch: B = 1, 64, 256, 1024, 4096 -> profiles/replicas.txt
    python scripts/perf_replicas.py --loop 8       # the yardstick: 8 of the same problems one after another (this mode
                                                   # uses nothing but optimize_pulses: it runs on the parent commit too)
    python scripts/perf_replicas.py --second-order             # the second-order leg: B = 1, 64, 256, 1024 (appended)
    python scripts/perf_replicas.py --second-order --loop 8    # its yardstick: the loop of optimize_pulses(sigma=)

Two shapes: config 3's (``configs.config_c3()``: K_r = 4, N = 4, nt = 2001, one control) and a two-control problem with
N = 16, K_r = 4, nt = 501.  The replicas differ in their guess amplitude and in lambda_a (a scan).  Per shape and B:
ms per Krotov iteration of the whole batch from HIP events around the two sweeps (KH_PROFILE) and from the wall clock
between two iterations inside the call (after a warm-up call), the update kernel's resident workgroups per CU
(hipOccupancyMaxActiveBlocksPerMultiprocessor) and the batch's whole wall time including its set-up.

The second-order leg (``--second-order``) takes the reference's notebook 07 shape -- config 3's system on 250 grid
points (K_r = 4, N = 4, one control), functional J_T_sm, sigma(t) = -max(eps_A, 2 A + eps_A) with A re-estimated every
iteration -- and reports the batch with ``sigma=`` next to the first-order batch of the same problems (the expected
extra cost per objective and interval: one 16 N byte load and one store) and, with ``--loop``, the loop of
``optimize_pulses(sigma=)`` over the same problems.
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

    if shape == 'nb07':
        spec = configs.config_c3(nt=250)
    else:
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


def shared(shape='c3'):
    import krotov_amd

    chis = krotov_amd.functionals.chis_sm if shape == 'nb07' else krotov_amd.functionals.chis_re
    return dict(propagator=krotov_amd.propagators.expm, chi_constructor=chis)


def new_sigma():
    """Notebook 07's sigma(t) (cell 30): -max(eps_A, 2 A + eps_A), A from ``numerical_estimate_A`` after every iteration."""
    import krotov_amd
    from krotov_amd.second_order import Sigma, numerical_estimate_A

    class _Sigma(Sigma):
        def __init__(self, A=0.0, epsA=2.0):
            self.A, self.epsA = A, epsA

        def __call__(self, t):
            return -max(self.epsA, 2 * self.A + self.epsA)

        def refresh(self, forward_states, forward_states0, chi_states, chi_norms, optimized_pulses, guess_pulses,
                    objectives, result):
            J = krotov_amd.functionals.J_T_sm
            dJ = J(None, objectives, tau_vals=result.tau_vals[-1]) - J(None, objectives, tau_vals=result.tau_vals[-2])
            self.A = numerical_estimate_A(forward_states, forward_states0, chi_states, chi_norms, dJ)

    return _Sigma()


def measure_batch(shape, B, iters, second_order=False):
    import torch

    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    problems, spec = problems_of(shape, B)

    def so(n):
        return dict(sigma=[new_sigma() for _ in range(n)]) if second_order else {}

    krotov_amd.optimize_pulses_batch(problems[:min(B, 2)], iter_stop=1, **so(min(B, 2)), **shared(shape))  # warm-up (library, allocator)
    torch.cuda.synchronize()
    clock = Clock(problems[0]['objectives'])
    t0 = time.perf_counter()
    krotov_amd.optimize_pulses_batch(problems, iter_stop=iters, info_hook=clock, **so(B), **shared(shape))
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
                wall_all_s=wall_all, occupancy=occupancy_of(spec, second_order))


def occupancy_of(spec, second_order=False):
    """Resident workgroups per CU of the update kernel for this shape (a one-replica engine is asked)."""
    import torch

    from krotov_amd.engine import HipKrotovEngine

    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), is_super=spec.is_super, replicas=1)
    try:
        if second_order:  # (the instantiation the next update sweep launches)
            store = torch.zeros((spec.K, len(spec.tlist), spec.N), dtype=torch.complex128, device=eng.device)
            eng.set_second_order_replicas(store, store.clone(), np.zeros((1, len(spec.tlist) - 1)))
        return eng.replica_occupancy()
    finally:
        eng.close()


def measure_loop(shape, n, iters, second_order=False):
    import torch

    import krotov_amd

    def so():
        return dict(sigma=new_sigma()) if second_order else {}

    problems, spec = problems_of(shape, n)
    krotov_amd.optimize_pulses(problems[0]['objectives'], problems[0]['pulse_options'], spec.tlist, iter_stop=1, **so(),
                               **shared(shape))
    torch.cuda.synchronize()
    per_iter, t0 = [], time.perf_counter()
    for p in problems:
        clock = Clock(p['objectives'])
        krotov_amd.optimize_pulses(p['objectives'], p['pulse_options'], p['tlist'], iter_stop=iters, info_hook=clock, **so(),
                                   **shared(shape))
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
    ap.add_argument('--second-order', action='store_true',
                    help="the second-order leg: notebook 07's shape, sigma= next to the first-order batch (appended to --out)")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'replicas.txt'))
    args = ap.parse_args()
    if args.second_order:
        if args.shapes == ap.get_default('shapes'):
            args.shapes = 'nb07'
        if args.batches == ap.get_default('batches'):
            args.batches = '1,64,256,1024'
    import torch

    lines = ["# scripts/perf_replicas.py on %s, %d CUs" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).multi_processor_count)]
    for shape in args.shapes.split(','):
        orders = (True, False) if args.second_order else (False,)
        if args.loop:
            for so in orders:
                r = measure_loop(shape, args.loop, args.iters, second_order=so)
                lines.append("loop%s %-6s n %4d: %8.3f ms per iteration and problem, %8.4f s per problem with its set-up "
                             "(scaled: B problems take B times that)" % (
                                 '/so' if so else '   ', r['shape'], r['n'], r['iter_ms'], r['problem_s']))
                print(lines[-1], flush=True)
            continue
        for B in [int(x) for x in args.batches.split(',')]:
            for so in orders:
                r = measure_batch(shape, B, args.iters, second_order=so)
                lines.append("batch%s %-6s K_r %d N %2d L %d nt %4d  B %5d: sweeps %9.3f ms per iteration (backward %8.3f + update %8.3f, "
                             "HIP events), wall %9.3f ms per iteration, %7.2f s for the whole call; update kernel: %s workgroups per CU"
                             % ('/so' if so else '  ', r['shape'], r['K_r'], r['N'], r['L'], r['nt'], r['B'], r['sweeps_ms'],
                                r['backward_ms'], r['update_ms'], r['wall_iter_ms'], r['wall_all_s'], r['occupancy']))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a' if (args.loop or args.second_order) else 'w') as f:
        f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
