#!/usr/bin/env python3
"""Generate tests/golden/ref_mixed.npz: the reference's own ``optimize_pulses`` loop on objective lists that mix
dimensions and kinds (``krotov_amd.configs.config_mixed``).

Runs ONLY where the reference's sources are available (see make_reference_goldens.py, whose
``import_reference_krotov`` and numpy-mode plugin style this file reuses); the GPU box and the test-suite read the
committed ``.npz`` data.  The reference treats every objective on its own (its own ``H``, its own propagator call, its
own state: optimize.py:254-261, 806-911), so ``propagator=[...]`` holds one numpy-mode ``expm`` per objective, each
with its objective's equation-of-motion factor (-i for kets, 1 for Liouvillians), and ``mu`` dispatches on ``i_obj``
(mu.py:130-134).  Density matrices are handed over column-stacked, as the numpy mode needs.

Cases (keys ``<case>_<run>_<array>``): case ``dims`` (N = 3, 5, 9 with a Liouvillian) and ``same_n`` (a 4-level ket
next to a damped qubit density matrix, both N = 4); runs ``re`` / ``sm`` (chis_re / chis_sm, 3 iterations) and ``so``
(second order, chis_re, constant sigma = SO_SIGMA, 3 iterations).

Usage:  python tests/golden/make_mixed_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_reference_goldens import import_reference_krotov  # noqa: E402

CASES = ('dims', 'same_n')
RUNS = {'re': ('re', False), 'sm': ('sm', False), 'so': ('re', True)}
ITERS = 3
NT = 201
SO_SIGMA = -2.0  # constant sigma(t) of the second-order run (a Sigma whose refresh changes nothing)


def numpy_plugins(kinds):
    """(propagator list, mu) of the reference's numpy mode for objectives of their own kind."""
    import scipy.linalg as la

    def make_expm(is_super):
        f0 = (1.0 + 0j) if is_super else -1j  # propagators.py:94-99

        def expm(H, state, dt, c_ops=None, backwards=False, initialize=False):
            f = f0.conjugate() if backwards else f0
            A = f * H[0]
            for part in H[1:]:
                A = A + (f * part[1]) * part[0]
            return la.expm(A * dt) @ state

        return expm

    def mu(objs, i_obj, pulses, mapping, i_pulse, n):
        op = objs[i_obj].H[1 + i_pulse][0]
        return (lambda s: 1j * (op @ s)) if kinds[i_obj] else (lambda s: op @ s)

    return [make_expm(x) for x in kinds], mu


def run(krotov, case, chi, second_order):
    from krotov_amd import configs

    spec = configs.config_mixed(case, nt=NT, chi=chi)
    objectives, pulse_options = configs.mixed_to_objectives(spec, krotov, vectorized=True)
    props, mu = numpy_plugins(spec.kinds)
    sigma = None
    if second_order:
        class Sigma(krotov.second_order.Sigma):
            def __call__(self, t):
                return SO_SIGMA

            def refresh(self, **kwargs):
                pass

        sigma = Sigma()
    res = krotov.optimize_pulses(
        objectives, pulse_options, spec.tlist, propagator=props,
        chi_constructor=getattr(krotov.functionals, 'chis_' + chi), mu=mu,
        overlap=lambda a, b: complex(np.vdot(a, b)), norm=np.linalg.norm, iter_stop=ITERS,
        store_all_pulses=True, sigma=sigma)
    S = spec.N
    fw_T = np.zeros((spec.K, S), dtype=np.complex128)
    for k, st in enumerate(res.states):
        v = np.asarray(st).ravel()
        fw_T[k, :v.size] = v
    return dict(all_pulses=np.array([np.array(p) for p in res.all_pulses]), tau_vals=np.array(res.tau_vals),
                fw_T=fw_T)


def main():
    from krotov_amd import configs

    krotov = import_reference_krotov()
    out = dict(iter_stop=ITERS, nt=NT, so_sigma=SO_SIGMA)
    for case in CASES:
        spec = configs.config_mixed(case, nt=NT)
        out['%s_dims' % case] = np.array(spec.dims)
        out['%s_kinds' % case] = np.array(spec.kinds)
        for name, (chi, so) in RUNS.items():
            res = run(krotov, case, chi, so)
            for key, val in res.items():
                out['%s_%s_%s' % (case, name, key)] = val
            print('%-7s %-3s tau[-1] = %s' % (case, name, np.round(res['tau_vals'][-1], 6)))
    path = os.path.join(HERE, 'ref_mixed.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
