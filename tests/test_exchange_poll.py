"""The update sums' exchange of the q2 update kernels (kh_common.h: kh_publish / kh_gather_range, WIDE), against the oracle.

``kh_q2_forward_update`` polls the slot array with one 16-byte load per slot, through a buffer descriptor over one
parity's slots; lanes without a workgroup read slot 0 and drop it.  What can go wrong is an address, a bound of the
descriptor, a tag, or a slot that is dropped, swapped or counted twice -- none of which needs a large problem.

Cases (the smallest shapes at which this shows): N = 17 (beyond the one-wave-per-objective kernels of kh_mini.h, which
take N <= 16 at K <= 8; padded rows), six intervals, one control, which runs ``tile64q2/512``, at
K = 1 (no exchange), 2, 7, 8, 9 (a partial, a full and a started 128-byte line of eight slots), 63, 64, 65 and 255, 256
(the boundaries of the gather's 64-lane chunks, the last slot of the descriptor, the full grid).  Every objective has
operators, states and a co-state of its own, so the partial sums are pairwise different and none is small: a wrong
sum moves the pulses by >= 0.02 / K >= 7e-5, far beyond the tolerance (initial states are drawn until it does; asserted
on the oracle's side before the engine runs).  The three forms of the kernel (sums on the adjoint side, on the forward side under KH_NO_ADJ=1, second order)
run at K = 9 and K = 65; 70 intervals at K = 9 cross a KH_Q2_REFRESH boundary and reuse both parities of the slot
array 35 times, and a second sweep on the same engine must repeat the first bit for bit (the slots are cleared per
launch).

Tolerance: the project's 1e-12.
"""
import numpy as np
import pytest

from oracle import krotov_oracle as ko

N, TOL = 17, 1e-12
KS = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256)


def _hermitian(rng, n, norm):
    G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    H = (G + G.conj().T) / 2
    return H * (norm / np.linalg.norm(H, 2))


_refs = {}


def _reference(K, M):
    """Problem and oracle sweeps of (K objectives, M intervals), made once."""
    if (K, M) in _refs:
        return _refs[K, M]
    rng = np.random.default_rng(1000 * M + K)
    # ||H1_k|| = 0.5 ... 1: incommensurate from objective to objective
    ops = [[_hermitian(rng, N, 1.0), _hermitian(rng, N, 0.5 + 0.5 * ((k + 1) * np.sqrt(2.0) % 1.0))] for k in range(K)]
    unit = lambda a: a / np.linalg.norm(a, axis=1)[:, None]  # noqa: E731
    init = unit(rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
    target = unit(rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
    chi_T = unit(rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N)))
    tlist = np.concatenate([[0.0], np.cumsum(np.full(M, 0.4))])
    r = {'ops': ops, 'dt': np.diff(tlist), 'chi_T': chi_T, 'K': K, 'M': M,
         'pulses': [0.3 * np.cos(np.arange(M) * 0.7)], 'shapes': [np.linspace(0.5, 1.0, M)], 'lambdas': [0.05],
         'norms': np.full(K, 1.0 / K)}
    r['chi'] = ko.backward_sweep(ko.OracleProblem(ops, init, target, tlist), chi_T, r['pulses'])  # (does not read init)

    # the witness: what objective k adds to the first interval's pulse (optimize.py:470-477); an initial state that
    # happens to make it small is drawn again
    def move(k):
        return r['shapes'][0][0] / r['lambdas'][0] * r['norms'][k] * np.imag(np.vdot(r['chi'][k][0], ops[k][1] @ init[k]))

    for k in range(K):
        while abs(move(k)) < 0.02 / K:
            init[k] = unit(rng.standard_normal((1, N)) + 1j * rng.standard_normal((1, N)))[0]
    r['init'], r['moves'] = init, np.array([move(k) for k in range(K)])
    prob = ko.OracleProblem(ops, init, target, tlist)
    out = ko.forward_update_sweep(prob, r['chi'], r['norms'], r['pulses'], r['shapes'], r['lambdas'])
    r['opt'], r['upd_T'], r['g_a'] = np.array(out[0]), out[1], np.array(out[2])
    rng = np.random.default_rng(7)
    # (the earlier iteration's pulses lie close by: 0.5 sigma / ||chi|| is of the order of K here, and the second-order
    # term it multiplies feeds the state back into the pulse -- with states 20 % apart that loop amplifies rounding by 1e4)
    older = [q * (1.0 + 2e-3 * rng.standard_normal(q.shape)) for q in r['pulses']]
    r['prev'] = ko.forward_propagation(prob, older, store=True)[1]
    r['sigma'] = -(1.0 + rng.random(M))
    out = ko.forward_update_sweep(prob, r['chi'], r['norms'], r['pulses'], r['shapes'], r['lambdas'], sigma_vals=r['sigma'],
                                  fw_prev=r['prev'], store=True)
    r['so_opt'], r['so_T'], r['so_g_a'] = np.array(out[0]), out[1], np.array(out[2])
    _refs[K, M] = r
    return r


def _engine(r):
    from krotov_amd.engine import HipKrotovEngine

    eng = HipKrotovEngine(r['ops'], r['dt'])
    assert eng.kernel == 'tile64q2/512'
    return eng


def _update(eng, r):
    got = eng.forward_update(r['chi'], r['norms'], r['init'], np.array(r['pulses']), np.array(r['shapes']), np.array(r['lambdas']))
    eng.check()
    return got


def _devs(got, opt, upd_T, g_a):
    return {'opt': np.abs(got[0].cpu().numpy() - opt).max() / max(1.0, np.abs(opt).max()),
            'upd_T': np.abs(got[1].cpu().numpy() - upd_T).max(),
            'g_a': np.abs(got[2].cpu().numpy() - g_a).max() / max(1.0, np.abs(g_a).max())}


def _witness(r):
    moves = np.abs(r['moves'])
    assert moves.min() >= 0.02 / r['K'] > 1e7 * TOL, "an objective's sum is too small to be missed: %.1e" % moves.min()
    gaps = np.diff(np.sort(r['moves']))
    assert r['K'] == 1 or gaps.min() > 10 * TOL, "two objectives' sums coincide: %.1e" % gaps.min()
    assert np.abs(r['opt'] - np.array(r['pulses'])).max() > 1e-3


def test_reference_sums_are_all_visible():
    """No GPU: the oracle side of the smallest and of a 64-lane-boundary case -- every objective's sum would be missed."""
    for K in (2, 65):
        _witness(_reference(K, 6))


@pytest.mark.gpu
@pytest.mark.parametrize('K', KS)
def test_q2_update_sums_against_the_oracle(K):
    import torch

    if K > torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count:
        pytest.skip("one workgroup per objective: this device has fewer than %d CUs" % K)
    r = _reference(K, 6)
    _witness(r)
    eng = _engine(r)
    dev = _devs(_update(eng, r), r['opt'], r['upd_T'], r['g_a'])
    eng.close()
    print('exchange_poll K = %d: smallest move %.1e; %s' % (K, np.abs(r['moves']).min(), ' '.join('%s %.1e' % kv for kv in dev.items())))
    assert max(dev.values()) < TOL, dev


@pytest.mark.gpu
@pytest.mark.parametrize('K', (9, 65))
def test_every_form_of_the_q2_update_kernel(K, monkeypatch):
    """Second order (<true, false, *>) and the sums on the forward side (<false, false, *>) gather through the same code."""
    import torch

    from krotov_amd import _lib

    r = _reference(K, 6)
    _lib.forget_launched_kernels()
    eng = _engine(r)
    store = torch.full((K, r['M'] + 1, N), float('nan'), dtype=torch.complex128, device=eng.device)
    eng.set_second_order(r['prev'], store, r['sigma'])
    dev = {'so/' + k: v for k, v in _devs(_update(eng, r), r['so_opt'], r['so_T'], r['so_g_a']).items()}
    eng.close()
    monkeypatch.setenv('KH_NO_ADJ', '1')
    eng = _engine(r)
    dev.update({'fwd/' + k: v for k, v in _devs(_update(eng, r), r['opt'], r['upd_T'], r['g_a']).items()})
    eng.close()
    launched = _lib.kernel_instantiations(launched_only=True)
    for name in ('kh_q2_forward_update<true, false, true>', 'kh_q2_forward_update<false, false, true>'):
        assert name in launched, launched
    print('exchange_poll forms K = %d: %s' % (K, ' '.join('%s %.1e' % kv for kv in dev.items())))
    assert max(dev.values()) < TOL, dev


@pytest.mark.gpu
def test_slots_are_reused_and_cleared():
    """70 intervals: both parities 35 times, one restart of the resident tiles; two sweeps on one engine."""
    import torch

    r = _reference(9, 70)
    _witness(r)
    eng = _engine(r)
    first = _update(eng, r)
    again = _update(eng, r)
    dev = _devs(first, r['opt'], r['upd_T'], r['g_a'])
    eng.close()
    print('exchange_poll 70 intervals: %s' % ' '.join('%s %.1e' % kv for kv in dev.items()))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert max(dev.values()) < TOL, dev
