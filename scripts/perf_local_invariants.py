#!/usr/bin/env python3
"""Measure the device route of the perfect-entangler functional (``kh_chi_local_invariants``) against the host route.

    python scripts/perf_local_invariants.py            # B = 256, 1024 -> profiles/local_invariants.txt (appended)

Workload: the reference's notebook 07 (config 3's system on 250 grid points, K_r = 4 Bell-state objectives, N = 4, one
control, second order with sigma(t) = -max(0, 2 A), A re-estimated every iteration), B copies that differ in their guess
amplitude, as one ``optimize_pulses_batch``.  Per B, alternating and in one process:

* device: ``PerfectEntanglerChi`` passed as ``chi_constructor`` (co-states by ``kh_chi_local_invariants``);
* host:   the same object behind a lambda -- the route of any user constructor: psi(T) fetched, B calls of the
          constructor in Python, chi uploaded.

ms per Krotov iteration of the whole batch: the wall clock between the hook calls of consecutive iterations of the first
problem (every iteration ends in device-to-host copies: synchronised), median over the iterations after the first.  The
launch RATE of ``kh_chi_local_invariants``: HIP events around 200 back-to-back launches from Python on the batch's shape,
after a warm-up -- what the driver pays to issue it.  The kernel's execution time is a profiler's number, from a run of
its own: ``rocprofv3 --kernel-trace --stats -- python scripts/perf_local_invariants.py --kernel-only 1024``.  The
largest deviation between the two routes' pulses is printed with the times.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def problems_of(B, nt=250):
    import krotov_amd
    from krotov_amd import configs

    spec = configs.config_c3(nt=nt)
    tl = spec.tlist
    base = np.array([spec.controls[0](t, None) for t in tl])
    basis = [np.eye(4, dtype=np.complex128)[j].reshape(-1, 1) for j in range(4)]
    out = []
    for b in range(B):
        control = (0.7 + 0.6 * (b % 97) / 97.0) * base
        objectives = krotov_amd.gate_objectives(basis, 'PE', [spec.H0[0], [spec.Hc[0][0], control]])
        out.append(dict(objectives=objectives, tlist=tl,
                        pulse_options={id(control): dict(lambda_a=spec.lambda_a, update_shape=spec.update_shape)}))
    return out, krotov_amd.functionals.PerfectEntanglerChi(basis)


def new_sigma():
    from krotov_amd.second_order import Sigma, numerical_estimate_A

    class _Sigma(Sigma):
        def __init__(self):
            self.A = 0.0

        def __call__(self, t):
            return -max(0.0, 2 * self.A)

        def refresh(self, forward_states, forward_states0, chi_states, chi_norms, optimized_pulses, guess_pulses,
                    objectives, result):
            dJ = result.info_vals[-1] - result.info_vals[-2]
            self.A = numerical_estimate_A(forward_states, forward_states0, chi_states, chi_norms, dJ)

    return _Sigma()


def run(problems, con, chi_constructor, iters):
    """(ms per iteration of the whole batch, all pulses of problem 0 and of the last problem)."""
    import torch

    import krotov_amd

    first, stamps = problems[0]['objectives'], []

    def hook(**kw):
        if kw['objectives'] is first:
            stamps.append(time.perf_counter())
        return con.J_T(kw['fw_states_T'], kw['objectives'])

    res = krotov_amd.optimize_pulses_batch(problems, propagator=krotov_amd.propagators.expm, chi_constructor=chi_constructor,
                                           sigma=[new_sigma() for _ in problems], iter_stop=iters, store_all_pulses=True,
                                           info_hook=hook)
    torch.cuda.synchronize()
    per_iter = np.diff(stamps)
    ms = 1e3 * float(np.median(per_iter[1:])) if len(per_iter) > 1 else float('nan')  # (a warm-up run has one iteration)
    return ms, np.array([np.array(res[0].all_pulses), np.array(res[-1].all_pulses)])


def kernel_alone(B, launches=200):
    """us per LAUNCH of kh_chi_local_invariants on K = 4 B objectives, N = 4: HIP events around `launches` back-to-back
    calls from Python -- the rate at which the driver can issue it, not the kernel's execution time (that: ``--kernel-only``
    under ``rocprofv3 --kernel-trace --stats``, a run of its own)."""
    import torch

    from krotov_amd import configs
    from krotov_amd.engine import HipKrotovEngine

    rng = np.random.default_rng(0)
    H0, H1 = configs.herm(rng, 4, 1.0), configs.herm(rng, 4, 0.5)
    eng = HipKrotovEngine([[H0, H1]] * (4 * B), np.full((B, 4), 0.1), replicas=B)
    bell = np.array([[1, 0, 0, 1], [0, 1j, 1j, 0], [0, 1, -1, 0], [1j, 0, 0, -1j]]) / np.sqrt(2)
    q = np.linalg.qr(rng.standard_normal((B, 4, 4)) + 1j * rng.standard_normal((B, 4, 4)))[0]
    psi = eng.dev((np.transpose(q, (0, 2, 1)) @ bell).reshape(4 * B, 4), torch.complex128)
    bell_dev = eng.dev(bell, torch.complex128)
    out = eng.chi_local_invariants(psi, bell_dev, 'PE')
    for _ in range(10):
        eng.chi_local_invariants(psi, bell_dev, 'PE', out=out)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        eng.chi_local_invariants(psi, bell_dev, 'PE', out=out)
    stop.record()
    torch.cuda.synchronize()
    us = 1e3 * start.elapsed_time(stop) / launches
    eng.close()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='256,1024')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3, help="device / host pairs per B (alternating)")
    ap.add_argument('--kernel-only', type=int, default=0, metavar='B',
                    help="only launch kh_chi_local_invariants 200 times on B gates: the program to put behind "
                         "`rocprofv3 --kernel-trace --stats --` for the kernel's execution time")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'local_invariants.txt'))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("perf_local_invariants: no GPU (there is no fallback: nothing is measured)")
    if args.kernel_only:
        print("kh_chi_local_invariants, B = %d: %.1f us per launch (HIP events, launch rate)" % (
            args.kernel_only, kernel_alone(args.kernel_only)))
        return
    lines = ["# notebook 07's shape (K_r = 4, N = 4, nt = 250, L = 1), second order, optimize_pulses_batch; %s"
             % torch.cuda.get_device_name(0),
             "# B  route   ms per Krotov iteration of the whole batch (rounds)   kh_chi_local_invariants launch rate [us / launch from Python]"]
    for B in [int(x) for x in args.batches.split(',')]:
        problems, con = problems_of(B)
        run(problems[:2], con, con, 1)  # warm-up: library, allocator, both routes
        run(problems[:2], con, lambda **kw: con(**kw), 1)
        times = {'device': [], 'host': []}
        pulses = {}
        for _ in range(args.rounds):
            for route, chi in (('device', con), ('host', lambda **kw: con(**kw))):
                ms, pulses[route] = run(problems, con, chi, args.iters)
                times[route].append(ms)
        us = kernel_alone(B)
        dev = float(np.abs(pulses['device'] - pulses['host']).max())
        for route in ('device', 'host'):
            lines.append("%5d  %-6s  %s%s" % (B, route, "  ".join("%8.2f" % x for x in times[route]),
                                             "   %8.1f" % us if route == 'device' else ""))
        lines.append("%5d  host / device (medians) %.2fx; largest |pulse(device) - pulse(host)| after %d iterations %.2e"
                     % (B, np.median(times['host']) / np.median(times['device']), args.iters, dev))
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
