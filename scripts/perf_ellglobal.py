#!/usr/bin/env python3
"""The padded-row family's form with global vectors ("ellglobal/csr", kh_ellg.h) next to the streamed form where both
run, and alone beyond N = 4096 (dev tool, GPU only; writes profiles/ellglobal.txt).

    python scripts/perf_ellglobal.py [nt]

Per case: us per propagation (one objective over one interval; backward sweep and update sweep, K = 3 objectives on 3
CUs), terms of the series per step, and the bytes a term must move -- nnz x 20 B of pool (offset + value) plus nnz x 16 B
of gathers -- against the L2 rate of one CU (MI355X_MICROARCH.md: 34.5 TB/s over 256 CUs = 135 GB/s)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from krotov_amd import configs
from krotov_amd.engine import HipKrotovEngine

L2_PER_CU = 34.5e12 / 256  # bytes per second
nt = int(sys.argv[1]) if len(sys.argv) > 1 else 41
K = 3
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def run(label, spec, force):
    if force:
        os.environ['KH_KERNEL'] = force
    else:
        os.environ.pop('KH_KERNEL', None)
    ops = configs.sparse_ops(spec)
    tl = spec.tlist
    mid = 0.5 * (tl[1:] + tl[:-1])
    pulses = np.array([[c(t, None) for t in mid] for c in spec.controls])
    S, lam = np.ones((spec.L, len(tl) - 1)), np.full(spec.L, 2.0)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 1.0 / (2 * spec.K))
    eng = HipKrotovEngine(ops, np.diff(tl), is_super=spec.is_super)
    eng.profile = True
    for _ in range(2):
        chi = eng.backward(chi_T, pulses)
        eng.forward_update(chi, norms, spec.init, pulses, S, lam)
    eng.check()
    t = eng.kernel_times_ms()
    steps = len(tl) - 1
    terms = eng.stats()['matvecs'] / (spec.K * steps) - spec.L  # (the update sweep's control products are not terms)
    union = (abs(ops[0][0]) + sum(abs(o) for o in ops[0][1:])).nnz
    us_bw, us_up = 1e3 * min(t['backward']) / steps, 1e3 * min(t['update']) / steps
    per_term = us_bw / terms
    need = union * 36.0
    say('%-22s %-14s N=%-6d entries/row %5.1f  backward %8.1f us  update %8.1f us per propagation  %5.1f terms/step  '
        '%6.2f us/term  %6.2f MB/term = %5.1f GB/s = %4.0f %% of one CU\'s L2 rate' % (
            label, eng.kernel, spec.N, union / spec.N, us_bw, us_up, terms, per_term, need / 1e6, need / per_term / 1e3,
            100.0 * need / (per_term * 1e-6) / L2_PER_CU))
    eng.close()
    return us_bw


say('# scripts/perf_ellglobal.py, K = %d, %d intervals' % (K, nt - 1))
ladder = configs.config_sparse_lindblad(d=64, nt=nt, K=K)
a = run('ladder d=64, streamed', ladder, 'ellstream')
b = run('ladder d=64, global', ladder, 'ellglobal')
say('global / streamed at N = 4096: %.2f' % (b / a))
for n in (13, 16):
    run('spin chain n=%d' % n, configs.config_spin_chain(n, nt=nt, K=K), None)
out = os.path.join(ROOT, 'profiles', 'ellglobal.txt')
with open(out, 'w') as f:
    f.write('\n'.join(lines) + '\n')
print('written:', out)
