#!/usr/bin/env python3
"""Randomised parity sweep: the three device sweeps (forward with storage, backward, forward with sequential update) of
randomly drawn small problems against the oracle -- shapes picked around the dispatch boundaries of the kernel families
(N = 16 / 17, 64 / 65, 96 / 97, 128 / 129; 4 / 5 and 8 / 9 controls; one objective, more objectives than CUs; shared,
scaled and per-objective operators; objectives without one of their controls; Hilbert and Liouville space; dense and CSR).

Test infrastructure (it imports ``oracle/``): run on a GPU box,

    python tests/fuzz_parity.py [--seconds 300] [--seed 1] [--cases 0] [--level sweeps|optimize] [--regimes] [--drop-any] [--nonselfadjoint] [--short-grids]
                                 [--bounded-constrained] [--nonlinear]

prints one line per case (kernel, shape, largest deviation) and a summary; exit code 1 if any case is off by more than
the tolerance of tests/test_hip_parity.py (1e-12, 1e-11 in Liouville space).  ``tests/test_hip_parity.py::
test_fuzz_parity_fixed_seed`` runs a fixed-seed slice of it in the suite.  ``--regimes`` (sweeps level) puts every drawn
problem into a randomly chosen regime of the per-interval series (``ramp``, ``pulse_ramp``, ``tiny``: tests/helpers.py) and adds
Lindblad-form and mixed-dimension problems; it draws from a generator of its own, so the default stream stays what it is.
``--drop-any`` (sweeps level) takes a control from an objective of the drawn ``config_c5`` problems more often and where the
default stream never does -- with one control, with one objective, from objective 0, a middle objective or the last one
(tests/test_absent_controls.py) -- again decided by a generator of its own.  ``--nonselfadjoint`` (sweeps level) replaces a
random subset of the controls of the drawn ``config_c5`` problems by operators that are not Hermitian (``lower``, ``ladder``,
``anti``: tests/test_nonselfadjoint_controls.py), by a third generator of its own.  ``--short-grids`` (sweeps level) cuts
every drawn problem's grid to nt = 2 or 3 with update shapes, guess pulses and step widths of ``helpers.grid_ends`` (the
drawn ones vanish at both ends of the grid: tests/test_grid_ends.py), decided by a fourth generator of its own.
``--bounded-constrained`` (sweeps level) gives every drawn problem random pulse parametrizations with bounds from its guess
and a random Hermitian D with a linear shape, and runs one parametrized update sweep and one backward sweep with the
source against the two restatements (tests/parametrization_cases.py, tests/constraint_cases.py), by a fifth generator of
its own (tests/test_bounded_constrained_axes.py).  ``--nonlinear`` (sweeps level) runs, per case, a problem with a random term
table (terms eps_c^p H_j) on a random engine base in a random regime against tests/nonlinear_cases.py, drawn by a sixth
generator of its own (tests/test_nonlinear_axes.py).
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from krotov_amd import configs  # noqa: E402
from oracle import krotov_oracle as ko  # noqa: E402

import helpers as hp  # noqa: E402
from helpers import oracle_controls, spec_to_oracle  # noqa: E402

N_CHOICES = [2, 3, 4, 5, 7, 8, 15, 16, 17, 24, 31, 32, 33, 48, 63, 64, 65, 72, 80, 81, 95, 96, 97, 112, 127, 128, 129, 144]
L_CHOICES = [1, 1, 1, 2, 2, 3, 4, 4, 5, 5, 6, 7, 8, 8, 9, 12]
K_CHOICES = [1, 2, 3, 4, 5, 6, 8, 9]


def drop_any_control(rng_drop, spec, tag):
    """``--drop-any``: with probability 0.6 one control leaves objective 0, a middle objective or the last one (one control
    and one objective included); ``rng_drop`` is NOT the generator of :func:`draw`."""
    if rng_drop.random() < 0.6:
        k, l = int(rng_drop.choice([0, spec.K // 2, spec.K - 1])), int(rng_drop.integers(0, spec.L))
        if spec.Hc[k][l] is not None:
            spec.Hc[k] = list(spec.Hc[k])
            spec.Hc[k][l] = None
            tag += ' -Hc[%d][%d]' % (k, l)
    return tag


NSA_KINDS = ('lower', 'ladder', 'anti')


def nonselfadjoint_controls(rng_nsa, spec, tag):
    """``--nonselfadjoint``: one or two controls (of all objectives, of the last one, or of a random subset) become
    ``lower`` / ``ladder`` / ``anti`` variants of themselves, the ensemble's scales kept (``spec.mu``); ``spec.changed``:
    {(k, l): kind}.  The part that makes the generator non-normal is scaled so that, times the guess's 0.5 and the total
    time, it stays at 0.5 per changed control: the states stay O(1).  ``rng_nsa`` is NOT the generator of :func:`draw`."""
    spec.changed = {}
    if rng_nsa.random() < 0.15:  # (some problems stay as they are)
        return tag
    nt = len(spec.tlist)
    weight = min(1.0, 10.0 / (nt - 1))
    for l in sorted({int(l) for l in rng_nsa.integers(0, spec.L, size=int(rng_nsa.integers(1, 3)))}):
        kind = str(rng_nsa.choice(NSA_KINDS))
        where = str(rng_nsa.choice(['all', 'last', 'some']))
        ks = {'all': list(range(spec.K)), 'last': [spec.K - 1]}.get(where) or [k for k in range(spec.K) if rng_nsa.random() < 0.5]
        base = next((spec.Hc[k][l] / spec.mu[k] for k in range(spec.K) if spec.Hc[k][l] is not None), None)
        if base is None:
            continue
        new = hp.nonselfadjoint_variant(kind, base, rng_nsa)
        new = weight * new if kind != 'lower' else base + weight * (new - base)
        spec.Hc = [list(row) for row in spec.Hc]
        for k in ks:
            if spec.Hc[k][l] is not None:
                spec.Hc[k][l] = spec.mu[k] * new
                spec.changed[k, l] = kind
        tag += ' %s[%s][%d]' % (kind, where, l)
    return tag


def has_absent_control(spec):
    return any(op is None for row in getattr(spec, 'Hc', ()) for op in row)


def draw(rng, drop_controls=True, rng_drop=None, rng_nsa=None):
    """A random ProblemSpec (and a tag that says how it was made).  ``rng_drop``: the generator of ``--drop-any``;
    ``rng_nsa``: that of ``--nonselfadjoint``."""
    kind = rng.choice(['c5', 'c5', 'c5', 'c5', 'c5', 'c4', 'sparse', 'manyK'])
    if kind == 'c4':  # Liouville space, shared operator list, one control (cooperative / generic kernels)
        d = int(rng.choice([3, 4, 5, 6, 8, 9]))
        nt = int(rng.integers(4, 16))
        spec = configs.config_c4(d=d, nt=nt, n_logical=int(rng.integers(2, min(d, 4) + 1)))
        return spec, 'c4(d=%d, nt=%d)' % (d, nt), None
    if kind == 'sparse':  # CSR Lindbladians, two controls
        d = int(rng.choice([3, 4, 5, 6, 8]))
        nt = int(rng.integers(4, 14))
        K = int(rng.integers(1, min(d, 4) + 1))
        spec = configs.config_sparse_lindblad(d=d, nt=nt, K=K)
        return spec, 'sparse(d=%d, nt=%d, K=%d)' % (d, nt, K), 'csr'
    if kind == 'manyK':  # more objectives than CUs (tiny states: the oracle has to finish)
        K = int(rng.choice([257, 300, 513, 520]))
        N = int(rng.choice([2, 3, 4, 6]))
        L = int(rng.choice([1, 1, 2, 4, 5]))
        nt = int(rng.integers(3, 7))
        distinct = bool(rng.integers(0, 2))
        spec = configs.config_c5(K=K, N=N, nt=nt, L=L, distinct=distinct, seed=int(rng.integers(0, 1000)))
        tag = 'c5(K=%d, N=%d, nt=%d, L=%d%s)' % (K, N, nt, L, ', distinct' if distinct else '')
        if rng_drop is not None:
            tag = drop_any_control(rng_drop, spec, tag)
        if rng_nsa is not None:
            tag = nonselfadjoint_controls(rng_nsa, spec, tag)
        return spec, tag, None
    N = int(rng.choice(N_CHOICES))
    L = int(rng.choice(L_CHOICES))
    K = int(rng.choice(K_CHOICES))
    # the oracle's cost: K nt (L + 14) N^2 -- keep a case under a second or two
    nt = int(max(3, min(24, 4e6 // (K * (L + 14) * N * N))))
    nt = int(rng.integers(3, nt + 1))
    distinct = bool(rng.integers(0, 2))
    spec = configs.config_c5(K=K, N=N, nt=nt, L=L, distinct=distinct, seed=int(rng.integers(0, 1000)))
    tag = 'c5(K=%d, N=%d, nt=%d, L=%d%s)' % (K, N, nt, L, ', distinct' if distinct else '')
    if drop_controls and L > 1 and K > 1 and rng.random() < 0.3:  # an objective without one of its controls
        k, l = int(rng.integers(0, K)), int(rng.integers(0, L))
        spec.Hc[k][l] = None
        tag += ' -Hc[%d][%d]' % (k, l)
    if rng_drop is not None:
        tag = drop_any_control(rng_drop, spec, tag)
    if rng_nsa is not None:
        tag = nonselfadjoint_controls(rng_nsa, spec, tag)
    if rng.random() < 0.15:  # all objectives share ONE operator list (what gate_objectives builds)
        for k in range(1, K):
            spec.H0[k] = spec.H0[0]
            spec.Hc[k] = spec.Hc[0]
        if rng_nsa is not None:  # (objective 0's controls are everybody's now)
            spec.changed = {(k, l): kind for (k0, l), kind in spec.changed.items() if k0 == 0 for k in range(K)}
        tag += ' shared'
    return spec, tag, None


def draw_regime(rng, spec, tag, fmt):
    """``--regimes``: sometimes another kind of problem (Lindblad form, mixed dimensions), then a random regime; ``rng`` is
    NOT the generator of :func:`draw`.  Returns the regime problem, its tag and the theta_max it was built for."""
    kind = rng.choice(['drawn', 'drawn', 'drawn', 'drawn', 'lindblad', 'mixed'])
    if kind == 'lindblad':
        import test_lindblad_form as tlf

        d, n_c, L = int(rng.choice([3, 5, 8, 12, 17, 23])), int(rng.integers(0, 3)), int(rng.integers(1, 3))
        spec = tlf._random(d, int(rng.integers(1, 4)), L, n_c, int(rng.integers(12, 16)), int(rng.integers(0, 1000)),
                           per_objective=bool(rng.integers(0, 2)))
        spec.pulses = tlf._pulses(spec)
        spec.shapes = [np.linspace(0.2, 1.0, len(spec.dt)) for _ in range(L)]
        spec.lambdas = [0.7 + 0.3 * l for l in range(L)]
        tag, fmt = 'lindblad(d=%d, K=%d, L=%d, n_c=%d)' % (d, spec.K, L, n_c), 'lindblad'
    elif kind == 'mixed':
        case = str(rng.choice(['dims', 'same_n', 'wide']))
        spec = configs.config_mixed(case, nt=int(rng.integers(12, 24)))
        tag, fmt = 'mixed(%s)' % case, 'mixed'
    regime = str(rng.choice(['tiny', 'ramp', 'ramp', 'long'] + (['pulse_ramp'] if fmt in (None, 'csr') else [])))
    if regime == 'long' and not (fmt in (None, 'csr') and spec.K * spec.N ** 2 <= 2e4):
        regime = 'ramp'  # (140 intervals: where the oracle finishes in seconds)
    # theta_max is given to the engine explicitly: the value of most families or that of the cooperative / padded-row kernels
    theta_max = float(rng.choice([1.0, 1.0, 4.0]))
    wanted = {'long': 140, 'tiny': 0}.get(regime, int(rng.integers(hp.RAMP_MIN_INTERVALS, 17)))
    if fmt != 'lindblad' and len(spec.tlist) - 1 < wanted:
        # (the drawn grids have 2 ... 23 intervals and a ramp needs 11: the same time span on a finer grid; the regime sets
        # the step lengths anyway)
        spec.tlist = np.linspace(spec.tlist[0], spec.tlist[-1], wanted + 1)
    obj = hp.explicit(spec, 'dense' if fmt is None else fmt)
    try:
        out = hp.REGIMES[regime](obj, theta_max)
    except ValueError:  # (a pulse ramp needs the drift alone below theta_max: the stiff Liouvillians are beyond it)
        regime = 'ramp'
        out = hp.REGIMES[regime](obj, theta_max)
    return out, '%s %s theta_max=%g' % (tag, regime, theta_max), theta_max


def draw_short_grid(rng, spec, tag, fmt):
    """``--short-grids``: the drawn problem on one or two intervals (nt = 2, 3) as ``helpers.grid_ends`` builds it; ``rng`` is
    NOT the generator of :func:`draw`.  Returns the regime problem, its tag and the theta_max it was built for."""
    nt = int(rng.choice([2, 3]))
    theta_max = float(rng.choice([1.0, 1.0, 4.0]))
    spec.tlist = np.linspace(spec.tlist[0], spec.tlist[-1], nt)
    obj = hp.grid_ends(hp.explicit(spec, 'dense' if fmt is None else fmt), theta_max)
    hp.grid_ends_witness(obj, theta_max)
    return obj, '%s short nt=%d theta_max=%g' % (tag, nt, theta_max), theta_max


def run_regime_case(obj, theta_max):
    """:func:`run_case` for a regime problem (explicit interval values, any operator form)."""
    prob = hp.regime_oracle(obj)
    pulses, Sa, lama = np.array(obj.pulses), np.array(obj.shapes), np.array(obj.lambdas)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    norms = np.full(obj.K, 0.3 * min(1.0, 8.0 / obj.K) * min(1.0, 4.0 / obj.L))
    if obj.fmt == 'dense' and obj.is_super:
        norms *= 0.02
    with hp.MemoExpm():
        ref_T, ref_states = ko.forward_propagation(prob, obj.pulses, store=True)
        ref_chi = ko.backward_sweep(prob, chi_T, obj.pulses)
        ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, obj.pulses, obj.shapes, obj.lambdas)
    eng = hp.regime_engine(obj, theta_max)
    try:
        fw_T, states = eng.forward(pulses, prob.init, store=True)
        chi = eng.backward(chi_T, pulses)
        opt, psi_T, g_a = eng.forward_update(chi, norms, prob.init, pulses, Sa, lama)
        eng.check()
        scale = max(1.0, np.abs(np.array(ref_opt)).max())
        dev = {
            'states': np.abs(states.cpu().numpy() - ref_states).max(),
            'chi': np.abs(chi.cpu().numpy() - ref_chi).max(),
            'opt': np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() / scale,
            'psi_T': np.abs(psi_T.cpu().numpy() - ref_psi).max(),
            'g_a': np.abs(g_a.cpu().numpy() - ref_ga).max() / max(1.0, np.abs(ref_ga).max()),
        }
        return eng.kernel, dev
    finally:
        eng.close()


def run_case(spec, fmt):
    """Largest deviations (states, co-states, pulses, final states, g_a) of the device sweeps from the oracle's."""
    import scipy.sparse as sp

    from krotov_amd.engine import HipKrotovEngine

    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    pulses, Sa, lama = np.array(gp), np.array(S), np.array(lam)
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    # (the sequential update is a feedback loop: with many controls on a tiny state space -- L = 8 ... 12 at N = 2, 3 -- and
    # ||chi|| = 0.3 it amplifies the last-digit differences of ANY two implementations to 1e-11 within 20 intervals, while
    # states and co-states agree to 1e-15: seeds 11, 13 of the first run, generic and tile64x kernels alike)
    norms = np.full(spec.K, 0.3 * min(1.0, 8.0 / spec.K) * min(1.0, 4.0 / spec.L))
    if spec.is_super:  # (||H_1|| ~ 1e2..1e3 there: keep the updated pulses O(1), as tests/test_hip_parity.py does)
        norms *= 0.02
    ref_T, ref_states = ko.forward_propagation(prob, gp, store=True)
    ref_chi = ko.backward_sweep(prob, chi_T, gp)
    ref_opt, ref_psi, ref_ga = ko.forward_update_sweep(prob, ref_chi, norms, gp, S, lam)
    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    if fmt == 'csr':
        ops = [[None if o is None else sp.csr_matrix(o) for o in row] for row in ops]
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), is_super=spec.is_super)
    try:
        fw_T, states = eng.forward(pulses, spec.init, store=True)
        chi = eng.backward(chi_T, pulses)
        opt, psi_T, g_a = eng.forward_update(chi, norms, spec.init, pulses, Sa, lama)
        eng.check()
        scale = max(1.0, np.abs(np.array(ref_opt)).max())
        dev = {
            'states': np.abs(states.cpu().numpy() - ref_states).max(),
            'chi': np.abs(chi.cpu().numpy() - ref_chi).max(),
            'opt': np.abs(opt.cpu().numpy() - np.array(ref_opt)).max() / scale,
            'psi_T': np.abs(psi_T.cpu().numpy() - ref_psi).max(),
            'g_a': np.abs(g_a.cpu().numpy() - ref_ga).max() / max(1.0, np.abs(ref_ga).max()),
        }
        return eng.kernel, dev
    finally:
        eng.close()


def draw_kinds(rng_bc, pulses):
    """``--bounded-constrained``: a random kind (tests/parametrization_cases.py) per control with bounds from its guess --
    ``tanh`` bounds that hold the guess with a margin of 10 ... 100 % of max|guess|, not symmetric; ``tanhsq`` where the
    guess is >= 0, ``square`` where it is > 0."""
    out = []
    for p in pulses:
        p = np.asarray(p, dtype=np.float64)
        m = float(np.abs(p).max()) or 1.0
        kind = str(rng_bc.choice(['none', 'linear', 'tanh', 'tanh'] + (['tanhsq'] if p.min() >= 0.0 else []) +
                                 (['square'] if p.min() > 0.0 else [])))
        margin, where = 1.1 + 0.9 * rng_bc.random(), 2.0 * rng_bc.random() - 1.0
        if kind == 'tanh':
            shift = 0.9 * (margin - 1.0) * where
            out.append(('tanh', (shift - margin) * m, (shift + margin) * m))
        elif kind == 'tanhsq':
            out.append(('tanhsq', margin * m))
        elif kind == 'linear':
            out.append(('linear', (1.0 if where >= 0.0 else -1.0) * (0.5 + margin), 0.3 * m * where))
        else:
            out.append(None if kind == 'none' else ('square',))
    return out


def bounded_constrained_inputs(rng_bc, spec):
    """``--bounded-constrained``, host side: the drawn kinds, u and f' under the guess, lambda_a in u, the source of a random
    Hermitian D with the shape s_b(t) = c_0 + c_1 t / T on the states of a "previous iteration", norms != 1, and the two
    restated sweeps.  ``rng_bc`` is NOT the generator of :func:`draw`."""
    import constraint_cases as cc
    import parametrization_cases as pc

    prob = spec_to_oracle(spec)
    gp, S, lam = oracle_controls(spec)
    kinds = draw_kinds(rng_bc, gp)
    u_guess = [pc.inverse(k, p) for k, p in zip(kinds, gp)]
    dfdu = [pc.dfdu(k, u) for k, u in zip(kinds, u_guess)]
    # (the update moves the pulse by about f'^2 S / lambda Im D: lambda_a in u keeps it what the drawn problem was made for)
    lam_u = [x * max(1.0, float(np.abs(c).max()) ** 2) for x, c in zip(lam, dfdu)]
    chi_T = spec.target / np.linalg.norm(spec.target, axis=1)[:, None]
    norms = np.full(spec.K, 0.3 * min(1.0, 8.0 / spec.K) * min(1.0, 4.0 / spec.L))  # (run_case)
    if spec.is_super:
        norms *= 0.02
    D = configs.herm(rng_bc, prob.N, 1.0)
    lambda_b, c0, c1 = -(0.5 + 2.0 * rng_bc.random()), 0.3 + rng_bc.random(), 2.0 * rng_bc.random() - 1.0
    t0, t1 = spec.tlist[0], spec.tlist[-1]
    older = [p * (1.0 + 0.1 * rng_bc.standard_normal(np.shape(p))) for p in gp]
    src_norms = 0.2 + 0.7 * rng_bc.random(spec.K)
    with hp.MemoExpm():
        states = ko.forward_propagation(prob, older, store=True)[1]
        W = cc.source(D, cc.factors(lambda_b, spec.tlist, lambda t: c0 + c1 * (t - t0) / (t1 - t0)), states)
        ref_chi = ko.backward_sweep(prob, chi_T, gp)
        opt, u, psi_T, g_a = pc.update_sweep(prob, ref_chi, norms, u_guess, kinds, S, lam_u)
        src_chi = cc.backward_sweep(prob, chi_T, gp, W, src_norms)
    return dict(prob=prob, gp=gp, S=S, lam=lam_u, kinds=kinds, u_guess=np.array(u_guess), dfdu=np.array(dfdu), chi_T=chi_T,
                norms=norms, W=W, src_norms=src_norms, chi=ref_chi, opt=np.array(opt), u=np.array(u), psi_T=psi_T,
                g_a=np.array(g_a), src_chi=src_chi)


def run_bounded_constrained_case(rng_bc, spec, fmt):
    """``--bounded-constrained``: largest deviations of one parametrized update sweep (pulses, u, final states, g_a) and of
    one backward sweep with a source from the restatements; an engine that takes no parametrization says so in the kernel
    tag and runs nothing."""
    import scipy.sparse as sp
    import torch

    import parametrization_cases as pc
    from krotov_amd import _lib
    from krotov_amd.engine import HipKrotovEngine
    from krotov_amd.parametrization import PulseParameters

    r = bounded_constrained_inputs(rng_bc, spec)
    ops = [[spec.H0[k]] + [spec.Hc[k][l] for l in range(spec.L)] for k in range(spec.K)]
    if fmt == 'csr':
        ops = [[None if o is None else sp.csr_matrix(o) for o in row] for row in ops]
    eng = HipKrotovEngine(ops, np.diff(spec.tlist), is_super=spec.is_super)
    try:
        pulses = np.array(r['gp'])
        kind, a, b = PulseParameters([pc.to_product(k) for k in r['kinds']], r['gp']).device_kinds
        u_opt = torch.full(pulses.shape, float('nan'), dtype=torch.float64, device=eng.device)
        try:
            eng.set_parametrization(kind, a, b, r['u_guess'], r['dfdu'], u_opt)
        except _lib.KrotovHipError as exc:
            if exc.code != _lib.KH_ERR_UNSUPPORTED:
                raise
            return eng.kernel + ' (no parametrization)', {'skipped': 0.0}
        chi = eng.backward(r['chi_T'], pulses)
        opt, psi_T, g_a = eng.forward_update(chi, r['norms'], spec.init, pulses, np.array(r['S']), np.array(r['lam']))
        eng.check()
        src = eng.backward_source(r['chi_T'], pulses, r['W'], r['src_norms'])
        eng.check()
        kinds = ','.join('none' if k is None else k[0] for k in r['kinds'])
        return '%s [%s]' % (eng.kernel, kinds), {
            'chi': np.abs(chi.cpu().numpy() - r['chi']).max(),
            'opt': np.abs(opt.cpu().numpy() - r['opt']).max() / max(1.0, np.abs(r['opt']).max()),
            'u': np.abs(u_opt.cpu().numpy() - r['u']).max() / max(1.0, np.abs(r['u']).max()),
            'psi_T': np.abs(psi_T.cpu().numpy() - r['psi_T']).max(),
            'g_a': np.abs(g_a.cpu().numpy() - r['g_a']).max() / max(1.0, np.abs(r['g_a']).max()),
            'src': np.abs(src.cpu().numpy() - r['src_chi']).max() / max(1.0, np.abs(r['src_chi']).max()),
        }
    finally:
        eng.close()


NONLINEAR_BASES = {
    # name: (builder(J, nt), operator form, theta_max): a base of every engine family that takes a term table at small sizes
    'mini4': (lambda J, nt: configs.config_c5(K=2, N=4, nt=nt, L=J, distinct=True), 'dense', 1.0),
    'mini16': (lambda J, nt: configs.config_c5(K=6, N=16, nt=nt, L=J, distinct=True), 'dense', 1.0),
    'tile33': (lambda J, nt: configs.config_c5(K=5, N=33, nt=nt, L=J, distinct=True), 'dense', 1.0),
    'tile64': (lambda J, nt: configs.config_c5(K=4, N=64, nt=nt, L=J, distinct=True), 'dense', 1.0),
    'tile128': (lambda J, nt: configs.config_c5(K=3, N=80, nt=nt, L=J), 'dense', 1.0),
    'coop': (lambda J, nt: configs.config_shared(K=8, N=96, nt=nt, L=J), 'dense', 4.0),
    'csr33': (lambda J, nt: configs.config_c5(K=5, N=33, nt=nt, L=J, distinct=True), 'csr', 1.0),
    'csr12': (lambda J, nt: configs.config_c5(K=5, N=12, nt=nt, L=J, distinct=True), 'csr', 1.0),
}
NONLINEAR_REGIMES = ('ramp', 'pulse_ramp', 'tiny', 'amplitude', 'ends')


def draw_nonlinear(rng_nl):
    """``--nonlinear``: a problem with a term table (tests/nonlinear_cases.py, ``helpers`` with ``obj.terms``) -- J in 1..6
    slots, a table that meets ``kh_set_nonlinear``'s rules (1 <= C <= min(J, 3) controls, every control with a term, powers
    1..4, at least one power above 1, in random order), an engine base, a regime of the series entered under the
    coefficient pulses (or ``helpers.grid_ends`` on 1..6 intervals) and a sign per control.  ``rng_nl`` is NOT the
    generator of :func:`draw`.  Returns (problem, tag, theta_max)."""
    import nonlinear_cases as nc

    J = int(rng_nl.integers(1, 7))
    C = int(rng_nl.integers(1, min(J, 3) + 1))
    ctrl = list(range(C)) + [int(c) for c in rng_nl.integers(0, C, J - C)]
    rng_nl.shuffle(ctrl)
    power = [int(p) for p in rng_nl.integers(1, 5, J)]
    if max(power) == 1:
        power[int(rng_nl.integers(0, J))] = int(rng_nl.integers(2, 5))
    terms = list(zip(ctrl, power))
    base = str(rng_nl.choice(sorted(NONLINEAR_BASES)))
    regime = str(rng_nl.choice(NONLINEAR_REGIMES))
    signs = rng_nl.choice([-1.0, 1.0], C)
    build, fmt, theta_max = NONLINEAR_BASES[base]
    intervals = int(rng_nl.integers(1, 7)) if regime == 'ends' else 33
    obj = nc.with_terms(hp.explicit(build(J, intervals + 1), fmt), terms)
    obj = hp.grid_ends(obj, theta_max) if regime == 'ends' else hp.REGIMES[regime](obj, theta_max)
    obj.pulses = [s * np.asarray(p) for s, p in zip(signs, obj.pulses)]  # (theta sees |eps| only: the regime stays)
    obj.lambdas = nc.lambdas_in_eps(obj)
    tag = '%s %s I=%d terms=%s signs=%s' % (base, regime, intervals, ''.join('%d^%d ' % t for t in terms).strip().replace(' ', ','),
                                          ''.join('+' if s > 0 else '-' for s in signs))
    return obj, tag, theta_max


def nonlinear_inputs(obj):
    """``--nonlinear``, host side: co-states on the coefficient pulses and the restated non-linear update sweep."""
    import nonlinear_cases as nc

    view = nc.coefficient_view(obj)
    prob = hp.regime_oracle(view)
    chi_T = prob.target / np.linalg.norm(prob.target, axis=1)[:, None]
    norms = np.full(obj.K, 0.3 * min(1.0, 8.0 / obj.K) * min(1.0, 4.0 / obj.L))  # (run_regime_case)
    if getattr(obj, 'name', '').startswith('shared'):
        norms *= 0.02
    with hp.MemoExpm():
        chi = ko.backward_sweep(prob, chi_T, view.pulses)
        opt, psi_T, g_a = nc.update_sweep(prob, chi, norms, obj.pulses, obj.terms, obj.shapes, obj.lambdas)
    return dict(prob=prob, chi_T=chi_T, norms=norms, coef=np.array(view.pulses), dcde=nc.weights(obj.terms, obj.pulses),
                chi=chi, opt=np.array(opt), psi_T=psi_T, g_a=np.array(g_a))


def run_nonlinear_case(obj, theta_max):
    """``--nonlinear``: largest deviations of the co-states and of one non-linear update sweep from the restatement."""
    from krotov_amd import _lib

    r = nonlinear_inputs(obj)
    eng = hp.regime_engine(obj, theta_max)
    try:
        chi = eng.backward(r['chi_T'], r['coef'])
        eng.set_nonlinear([c for c, _ in obj.terms], [p for _, p in obj.terms], r['dcde'])
        _lib.forget_launched_kernels()
        opt, psi_T, g_a = eng.forward_update(chi, r['norms'], r['prob'].init, np.array(obj.pulses), np.array(obj.shapes),
                                             np.array(obj.lambdas))
        eng.check()
        form = [n for n in _lib.kernel_instantiations(launched_only=True) if '_nl<' in n]
        assert len(form) == 1, form
        return '%s %s' % (eng.kernel, form[0]), {
            'chi': np.abs(chi.cpu().numpy() - r['chi']).max(),
            'opt': np.abs(opt.cpu().numpy() - r['opt']).max() / max(1.0, np.abs(r['opt']).max()),
            'psi_T': np.abs(psi_T.cpu().numpy() - r['psi_T']).max(),
            'g_a': np.abs(g_a.cpu().numpy() - r['g_a']).max() / max(1.0, np.abs(r['g_a']).max()),
        }
    finally:
        eng.close()


def run_optimize_case(spec, fmt, rng):
    """Two iterations of ``krotov_amd.optimize_pulses`` on the GPU against ``oracle.optimize``: a random chi constructor
    (``chis_re / ss / sm``; ``chis_hs`` for density matrices), first or second order (the reference's notebook-07 sigma with
    A re-estimated every iteration); pulses after every iteration, tau, final states."""
    import krotov_amd
    import krotov_amd.engine as engine_mod

    from helpers import SigmaA, oracle_optimize, product_sigma

    chis = ['re', 'ss', 'sm'] + (['hs'] if spec.is_super else [])
    spec.chi = str(rng.choice(chis))
    # second order only where the update's feedback is well conditioned: with hundreds of objectives (||chi_k|| ~ 1 / K in
    # the bra's 0.5 sigma / ||chi|| (phi - phi_prev)) or many controls on a tiny state space, ANY two implementations differ
    # by 1e-11 ... 1e-8 after two iterations (first run of this mode: 13 such cases, all second order, four kernel families)
    second = bool(rng.random() < 0.35) and spec.K <= 16 and spec.L <= 4 and spec.N >= 2 * spec.L
    eps_a = 2e-3 if spec.is_super else 0.5
    objectives, pulse_options = configs.spec_to_objectives(spec, krotov_amd)
    # (the CSR cases run as dense Liouvillians here: the sparse propagator's state containers are covered by the suite)
    prop = krotov_amd.propagators.HipExpm(liouville=True) if spec.is_super else krotov_amd.propagators.expm
    kw = dict(sigma=product_sigma(0.0, eps_a)) if second else {}
    res = krotov_amd.optimize_pulses(objectives, pulse_options, spec.tlist, propagator=prop,
                                     chi_constructor=getattr(krotov_amd.functionals, 'chis_' + spec.chi), iter_stop=2,
                                     store_all_pulses=True, **kw)
    ref = oracle_optimize(spec, 2, **(dict(sigma=SigmaA(0.0, eps_a)) if second else {}))
    got = np.array([np.array(p) for p in res.all_pulses])
    scale = max(1.0, np.abs(ref['all_pulses']).max())
    fw_T = np.array([np.asarray(st).ravel(order='F') for st in res.states])
    dev = {
        'pulses': np.abs(got - ref['all_pulses']).max() / scale,
        'tau': np.abs(np.array(res.tau_vals) - ref['tau_vals']).max(),
        'states': np.abs(fw_T - ref['fw_T']).max(),
    }
    return '%s chis_%s%s' % (engine_mod.LAST_ENGINE().kernel, spec.chi, ' 2nd' if second else ''), dev


def fuzz(seed, seconds=None, cases=None, verbose=True, level='sweeps', regimes=False, drop_any=False, stats=None,
         nonselfadjoint=False, short_grids=False, bounded_constrained=False, nonlinear=False):
    """Run random cases until `seconds` have passed or `cases` are done; returns (number run, list of failures).
    ``stats``: a dict that receives how many cases had an absent control (``'absent'``) and how many of those had one
    control (``'absent_L1'``), and how many a control that is not self-adjoint (``'nonselfadjoint'``)."""
    rng = np.random.default_rng(seed)
    rng_regimes = np.random.default_rng([int(seed), 0x7e91]) if regimes else None  # (the default stream stays untouched)
    rng_drop = np.random.default_rng([int(seed), 0xd709]) if drop_any and level == 'sweeps' else None  # (likewise)
    rng_nsa = np.random.default_rng([int(seed), 0x5ad1]) if nonselfadjoint and level == 'sweeps' else None  # (likewise)
    rng_short = np.random.default_rng([int(seed), 0x2e9d]) if short_grids and level == 'sweeps' else None  # (likewise)
    rng_bc = np.random.default_rng([int(seed), 0xbc0d]) if bounded_constrained and level == 'sweeps' else None  # (likewise)
    rng_nl = np.random.default_rng([int(seed), 0x4e11]) if nonlinear and level == 'sweeps' else None  # (likewise)
    counts = {'absent': 0, 'absent_L1': 0}
    if rng_nsa is not None:  # (the key only where it was asked for: the older tests compare the whole dict)
        counts['nonselfadjoint'] = 0
    if rng_bc is not None:  # (likewise: the engines that took no parametrization, whose case ran nothing)
        counts['no_parametrization'] = 0
    t0 = time.time()
    done, failures, by_kernel = 0, [], {}
    while True:
        if cases is not None and done >= cases:
            break
        if seconds is not None and time.time() - t0 > seconds:
            break
        # (optimize level: every Objective lists every control -- configs.spec_to_objectives has no form for a missing one)
        spec, tag, fmt = draw(rng, drop_controls=level != 'optimize', rng_drop=rng_drop, rng_nsa=rng_nsa)
        if rng_nsa is not None:
            counts['nonselfadjoint'] += 1 if getattr(spec, 'changed', None) else 0
        if has_absent_control(spec):  # (counted on the problem itself: a shared operator list may have taken the entry back)
            counts['absent'] += 1
            counts['absent_L1'] += 1 if spec.L == 1 else 0
        if level == 'optimize' and spec.L > spec.N:
            # more controls than state dimensions: after two iterations with the host's own ||chi|| any two implementations
            # are 1e-10 apart (seed 24: generic kernels, K = 1, N = 2, L = 12, first order) -- conditioning, not a kernel
            continue
        tol = (1e-10 if spec.is_super else 1e-11) if level == 'optimize' else (1e-11 if spec.is_super else 1e-12)
        tol2 = 1e-9  # second order (the kernel tag ends in '2nd'): sigma's A is a ratio of small differences (1e-9)
        try:
            if rng_short is not None:
                obj, tag, theta_max = draw_short_grid(rng_short, spec, tag, fmt)
                tol = 1e-11 if bool(np.any(obj.is_super)) else 1e-12
                kernel, dev = run_regime_case(obj, theta_max)
            elif rng_regimes is not None and level == 'sweeps':
                obj, tag, theta_max = draw_regime(rng_regimes, spec, tag, fmt)
                liouville = obj.fmt == 'lindblad' or bool(np.any(obj.is_super))
                tol = 1e-11 if liouville or ' ramp ' in tag else 1e-12  # (as tests/test_series_regimes.py)
                kernel, dev = run_regime_case(obj, theta_max)
            elif rng_nl is not None:  # (a problem of its own; the default stream drew its own above, as always)
                obj, tag, theta_max = draw_nonlinear(rng_nl)
                tol = 1e-11 if ' ramp ' in tag or ' amplitude ' in tag else 1e-12  # (as tests/test_nonlinear_axes.py)
                kernel, dev = run_nonlinear_case(obj, theta_max)
            elif rng_bc is not None:
                kernel, dev = run_bounded_constrained_case(rng_bc, spec, fmt)
                counts['no_parametrization'] += 1 if kernel.endswith('(no parametrization)') else 0
            elif level == 'optimize':
                kernel, dev = run_optimize_case(spec, fmt, rng)
            else:
                kernel, dev = run_case(spec, fmt)
            worst = max(dev.values())
            ok = bool(np.isfinite(worst) and worst < (tol2 if kernel.endswith('2nd') else tol))
            line = '%-16s %-58s %s' % (kernel, tag, ' '.join('%s %.1e' % kv for kv in dev.items()))
        except Exception as exc:  # (an engine that refuses a shape it should take is a finding too)
            kernel, ok = '?', False
            line = '%-16s %-58s %r' % ('ERROR', tag, exc)
        by_kernel[kernel] = by_kernel.get(kernel, 0) + 1
        if not ok:
            failures.append(line)
        if verbose:
            print(('ok   ' if ok else 'FAIL ') + line, flush=True)
        done += 1
    if stats is not None:
        stats.update(counts)
    if verbose:
        print('%d cases in %.0f s, %d failed; kernels: %s' % (done, time.time() - t0, len(failures),
                                                             ', '.join('%s x %d' % kv for kv in sorted(by_kernel.items()))))
    return done, failures


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--seconds', type=float, default=300.0)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--cases', type=int, default=0)
    ap.add_argument('--level', choices=['sweeps', 'optimize'], default='sweeps',
                    help="'optimize': two iterations of optimize_pulses (random chi constructor, first / second order) against oracle.optimize")
    ap.add_argument('--regimes', action='store_true',
                    help="put every drawn problem into a random regime of the series (ramp, pulse_ramp, tiny) and add Lindblad-form "
                         "and mixed-dimension problems; drawn from a separate generator")
    ap.add_argument('--drop-any', action='store_true',
                    help="drawn config_c5 problems lose a control more often, also with one control or one objective and from "
                         "objective 0, a middle or the last objective; decided by a separate generator (sweeps level)")
    ap.add_argument('--nonselfadjoint', action='store_true',
                    help="a random subset of the controls of the drawn config_c5 problems becomes lower / ladder / anti variants "
                         "(not Hermitian); decided by a separate generator (sweeps level)")
    ap.add_argument('--short-grids', action='store_true',
                    help="every drawn problem on nt = 2 or 3 grid points with shapes, pulses and step widths that do not vanish "
                         "at the ends (helpers.grid_ends); decided by a separate generator (sweeps level)")
    ap.add_argument('--bounded-constrained', action='store_true',
                    help="every drawn problem gets random pulse parametrizations (bounds from its guess) and a random Hermitian D "
                         "with a linear shape: one parametrized update sweep and one backward sweep with the source against the "
                         "restatements; decided by a separate generator (sweeps level)")
    ap.add_argument('--nonlinear', action='store_true',
                    help="every case is a problem with a random term table (J in 1..6 slots, powers 1..4) on a random engine base "
                         "in a random regime with a random sign pattern: one non-linear update sweep against the restatement; "
                         "drawn from a separate generator (sweeps level)")
    a = ap.parse_args()
    n, bad = fuzz(a.seed, seconds=None if a.cases else a.seconds, cases=a.cases or None, level=a.level, regimes=a.regimes,
                  drop_any=a.drop_any, nonselfadjoint=a.nonselfadjoint, short_grids=a.short_grids,
                  bounded_constrained=a.bounded_constrained, nonlinear=a.nonlinear)
    sys.exit(1 if bad else 0)
