#!/usr/bin/env python3
"""Time the sweeps of Lindblad-form problems on the matrix-form engine ("lindblad/matrix", krotov_amd/csrc/kh_lind.h) at
engine level, with HIP events on the launch stream (dev tool, GPU only):

  c4        BASELINE config 4 in Lindblad form (configs.config_c4_lindblad: K = 16, d = 20, 1000 intervals)
  k256 D    K = 256 objectives with their own operators at d = D (one Lindblad operator, one control, 200 intervals)

usage: python scripts/perf_lindblad.py c4 | k256 16 | k256 32   [--liouvillian]
--liouvillian: the same problem as Liouvillians on the uniform engine (what a caller had to do before), for comparison."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from krotov_amd import configs
from krotov_amd.engine import HipKrotovEngine

args = [a for a in sys.argv[1:] if not a.startswith('--')]
liouvillian = '--liouvillian' in sys.argv
what = args[0] if args else 'c4'
if what == 'c4':
    ls = configs.config_c4_lindblad()
    K, d, tlist = ls.K, ls.d, ls.tlist
    H = [[ls.H0, ls.H1]] * K
    C = [list(ls.c_ops)] * K
    init, target = ls.init, ls.target
    tl = tlist
    pulses = np.array([[ls.controls[0](t + 0.5 * (tl[1] - tl[0]), None) for t in tl[:-1]]])
else:
    K, d, nt = 256, int(args[1]), 201
    rng = np.random.default_rng(0)
    tlist = np.linspace(0, 0.05 * (nt - 1), nt)
    H = [[configs.herm(rng, d, 6.0), configs.herm(rng, d, 2.0)] for _ in range(K)]
    C = [[0.4 * (rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))) / np.sqrt(d)] for _ in range(K)]

    def rho():
        G = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        r = G @ G.conj().T
        return r / np.trace(r).real

    init, target = np.array([rho() for _ in range(K)]), np.array([rho() for _ in range(K)])
    pulses = 0.5 * np.sin(np.pi * tlist[:-1] / tlist[-1])[None, :]
nt = len(tlist)
vec = lambda a: np.array([r.ravel(order='F') for r in a])  # noqa: E731
if liouvillian:
    made = {}

    def sup(op, cs=()):
        key = (id(op),) + tuple(id(c) for c in cs)
        if key not in made:
            made[key] = configs.liouvillian_dense(op, cs)
        return made[key]

    eng = HipKrotovEngine([[sup(H[k][0], C[k]), sup(H[k][1])] for k in range(K)], np.diff(tlist), is_super=True)
else:
    eng = HipKrotovEngine(H, np.diff(tlist), c_ops=C)
eng.profile = True
init, target = vec(init), vec(target)
S, lam = np.ones((1, nt - 1)), np.ones(1)
chi_T = target / np.linalg.norm(target, axis=1)[:, None]
norms = np.full(K, 1.0 / (2 * K))
chi = None
for _ in range(3):
    chi = eng.backward(chi_T, pulses, out=chi)
    out = eng.forward_update(chi, norms, init, pulses, S, lam)
eng.check()
t = eng.kernel_times_ms()
bw, up = min(t['backward']), min(t['update'])
terms = eng.stats()['matvecs'] / (K * (nt - 1))
print('%s %s K=%d d=%d N=%d intervals=%d: backward %.2f ms (%.2f us per interval)  update %.2f ms (%.2f us per interval)  '
      'iteration (backward + update) %.2f ms  series terms per interval and objective %.1f' % (
          what, eng.kernel, K, d, d * d, nt - 1, bw, 1e3 * bw / (nt - 1), up, 1e3 * up / (nt - 1), bw + up, terms))
