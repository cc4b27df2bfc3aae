#!/usr/bin/env python3
"""One sparse objective on S workgroups ("ellsplit/csr", kh_ellg.h's split form) against one workgroup per objective
("ellglobal/csr", its plain form: S = 1, the baseline) on spin chains beyond N = 4096 (dev tool, GPU only; writes
profiles/ellsplit.txt).

    python scripts/perf_ellsplit.py [nt] [output file]

Problems: chains of n = 13, 15, 17 qubits (N = 8192, 32 768, 131 072), K = 1 and 3 objectives.  Per problem and S in
{1, 2, 4, 8, 16, 32, 64}: us per propagation (one objective over one interval) and per term of the series, for the
backward sweep and for the update sweep; device events around each launch, one warm-up and REPEATS timed launches per
point, the S values alternating inside every repeat; reported: the median and the spread (max - min) over the repeats.
Per problem the file then names the best S, the smallest S within the best one's spread of it, and whether that beats
S = 1 by more than the spread -- what ``row_split='auto'`` is to be set from."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from krotov_amd import _lib, configs
from krotov_amd.engine import HipKrotovEngine

REPEATS = 5
SPLITS = (1, 2, 4, 8, 16, 32, 64)
nt = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'ellsplit.txt')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def measure(n, K):
    os.environ.pop('KH_KERNEL', None)
    spec = configs.config_spin_chain(n, nt=nt, K=K)
    ops = configs.sparse_ops(spec)
    bounds = [float(abs(m).sum(axis=1).max()) for m in ops[0]]
    tl = spec.tlist
    steps = len(tl) - 1
    mid = 0.5 * (tl[1:] + tl[:-1]) / tl[-1]
    pulses = np.array([0.3 * np.sin((l + 1) * np.pi * mid) ** 2 + 0.1 * (l + 1) for l in range(spec.L)])
    shapes, lam = np.ones((spec.L, steps)), np.full(spec.L, 2.0)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(K, 1.0 / (2 * K))
    eng = HipKrotovEngine(ops, np.diff(tl), op_norms=np.tile(bounds, K))
    assert eng.kernel == 'ellglobal/csr', eng.kernel
    eng.profile = True
    usable = []
    for S in SPLITS:
        try:
            eng.set_row_split(S)
            usable.append(S)
        except _lib.KrotovHipError as exc:
            say('  n=%d K=%d S=%d: refused (%s)' % (n, K, S, exc))
    times = {S: {'backward': [], 'update': []} for S in usable}
    terms = {}
    for rep in range(REPEATS + 1):  # (rep 0: warm-up of every shape)
        for S in usable:
            eng.set_row_split(S)
            chi = eng.backward(chi_T, pulses)
            eng.check()
            terms[S] = eng.stats()['matvecs'] / (K * steps)
            eng.forward_update(chi, norms, spec.init, pulses, shapes, lam)
            eng.check()
            t = eng.kernel_times_ms()
            if rep > 0:
                times[S]['backward'].append(1e3 * t['backward'][-1] / (K * steps))
                times[S]['update'].append(1e3 * t['update'][-1] / (K * steps))
    union = (abs(ops[0][0]) + sum(abs(o) for o in ops[0][1:])).nnz
    say('spin chain n=%d  N=%d  K=%d  %d intervals  entries/row %.1f  %.1f terms/step  %.2f MB of pool and gathers per term' % (
        n, spec.N, K, steps, union / spec.N, terms[1], union * 36.0 / 1e6))
    say('    S  kernel          backward us/propagation (median, spread)  us/term   update us/propagation (median, spread)  us/term')
    med = {}
    for S in usable:
        bw, up = np.array(times[S]['backward']), np.array(times[S]['update'])
        med[S] = (np.median(bw), bw.max() - bw.min(), np.median(up), up.max() - up.min())
        say('  %3d  %-14s  %12.1f  %10.1f  %18.2f  %14.1f  %10.1f  %16.2f' % (
            S, 'ellglobal/csr' if S == 1 else 'ellsplit/csr', med[S][0], med[S][1], med[S][0] / terms[S], med[S][2], med[S][3],
            med[S][2] / terms[S]))
    for name, i in (('backward', 0), ('update', 2)):
        best = min(usable, key=lambda S: med[S][i])
        spread = max(med[best][i + 1], med[1][i + 1])
        smallest = min(S for S in usable if med[S][i] <= med[best][i] + spread)
        gain = med[1][i] / med[best][i]
        say('  %-8s best S = %d (%.2fx of S = 1); smallest S within the spread of it: %d; beats S = 1 by more than the spread: %s' % (
            name, best, gain, smallest, 'yes' if med[1][i] - med[best][i] > spread else 'no'))
    eng.close()


say('# scripts/perf_ellsplit.py, %d intervals, %d repeats per point (median, spread = max - min)' % (nt - 1, REPEATS))
for n in (13, 15, 17):
    for K in (1, 3):
        measure(n, K)
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print('written:', out)
