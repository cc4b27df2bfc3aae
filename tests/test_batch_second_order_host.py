"""``optimize_pulses_batch(..., sigma=[...])`` without a GPU: the driver on an oracle-backed replica engine double with the
second-order update (tests/replica_double_so.py), against separate ``optimize_pulses(sigma=)`` runs on the same double
-- bit for bit, since every sweep of the double runs replica by replica through the oracle -- and the C ABI's argument
checks of ``kh_set_second_order_replicas``.  Reference: optimize.py:429-442, 451-452, 468-469, 492-500, 566-577."""
import logging

import numpy as np
import pytest

from helpers import product_sigma
from krotov_amd import configs
from test_replicas import _loop, _opt_specs, _problems, _same_result, _shared_kw


@pytest.fixture
def replica_double_so(monkeypatch):
    import krotov_amd.engine as engine_mod
    from replica_double import ReplicaEngineDouble
    from replica_double_so import ReplicaEngineDoubleSO

    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', ReplicaEngineDoubleSO)
    ReplicaEngineDouble.created = []
    return ReplicaEngineDoubleSO


def _specs(kind):
    """Three problems of one shape that differ in lambda_a (and, in Liouville space, in the control's strength)."""
    if kind == 'hilbert':  # config 3 (notebook 07's Hamiltonian) on a short grid
        specs = [configs.config_c3(nt=13) for _ in range(3)]
        for spec, lam in zip(specs, (10.0, 20.0, 40.0)):
            spec.lambda_a = lam
        return specs
    specs = []
    for s, lam in ((1.0, 5.0), (0.7, 2.0), (1.3, 11.0)):
        spec = configs.config_c2_liouville(nt=9)
        spec.Hc = [[s * spec.Hc[0][0]]] * 3
        spec.lambda_a = lam
        specs.append(spec)
    return specs


def _kw(kind):
    import krotov_amd

    if kind == 'hilbert':
        return dict(propagator=krotov_amd.propagators.expm, chi_constructor=krotov_amd.functionals.chis_sm)
    return dict(propagator=krotov_amd.propagators.HipExpm(liouville=True), chi_constructor=krotov_amd.functionals.chis_re)


def _loop_so(problems, sigmas, **kw):
    import krotov_amd

    return [krotov_amd.optimize_pulses(p['objectives'], p['pulse_options'], p['tlist'], sigma=s, **kw)
            for p, s in zip(problems, sigmas)]


def _info(**kw):
    """An info_hook whose value depends on the trajectories it is handed."""
    fw, fw0 = kw['forward_states'], kw['forward_states0']
    mid = len(fw[0]) // 2
    return [complex(np.asarray(fw[k][mid]).ravel()[0]) - complex(np.asarray(fw0[k][mid]).ravel()[0]) for k in range(len(fw))]


@pytest.mark.parametrize('kind', ['hilbert', 'liouville'])
def test_second_order_batch_on_the_double_equals_separate_runs(kind, replica_double_so):
    import krotov_amd

    problems = _problems(_specs(kind))
    sig_b, sig_s = [product_sigma(0.0, 2.0) for _ in range(3)], [product_sigma(0.0, 2.0) for _ in range(3)]
    seen = []

    def hook(**kw):
        seen.append((kw['iteration'], kw['sigma']))
        return _info(**kw)

    results = krotov_amd.optimize_pulses_batch(problems, sigma=sig_b, iter_stop=3, store_all_pulses=True, info_hook=hook,
                                               **_kw(kind))
    engines = list(replica_double_so.created)
    assert [e.replicas for e in engines] == [3] and engines[0].so_calls == 3
    assert [s[0] for s in engines[0].sweeps] == ['forward'] + ['backward', 'update'] * 3
    # every replica's hook got its own Sigma object
    assert [s for _, s in seen[:3]] == sig_b and all(any(s is x for x in sig_b) for _, s in seen)
    loop = _loop_so(problems, sig_s, iter_stop=3, store_all_pulses=True, info_hook=_info, **_kw(kind))
    for res, seq, sb, ss in zip(results, loop, sig_b, sig_s):
        _same_result(res, seq)
        assert len(sb.history) == 2 and sb.history == ss.history  # (the A history, bit for bit)
        assert sb.calls == ss.calls and sb.calls[0][2] is True
    # ... and the sigma term was on: the first-order batch gives other pulses
    first = krotov_amd.optimize_pulses_batch(problems, iter_stop=1, store_all_pulses=True, **_kw(kind))
    for res, one in zip(results, first):
        assert np.abs(np.array(res.all_pulses[1]) - np.array(one.all_pulses[1])).max() > 1e-6


def _recording_sigma(events, b, T):
    from krotov_amd.second_order import Sigma, numerical_estimate_A

    class _Sigma(Sigma):
        """Time dependent, so that a replica's own mid-points matter; A from the trajectories' final states."""

        def __init__(self):
            self.A = 0.0

        def __call__(self, t):
            return -(2.0 + max(0.0, 2 * self.A)) * (1.0 + 0.5 * t / T)

        def refresh(self, forward_states, forward_states0, chi_states, chi_norms, optimized_pulses, guess_pulses,
                    objectives, result):
            events.append(('refresh', b, result.iters[-1], objectives, result, len(forward_states), len(forward_states[0]),
                           guess_pulses is optimized_pulses))
            self.A = numerical_estimate_A(forward_states, forward_states0, chi_states, chi_norms, -1e-3 * (1 + b))

    return _Sigma()


def test_refresh_runs_only_for_replicas_that_go_on(replica_double_so):
    import krotov_amd

    specs = [configs.config_c5(K=3, N=5, nt=9, distinct=True, seed=3, lambda_a=lam, T=(1.0 + 0.25 * b) * 8 / 4000.0)
             for b, lam in enumerate((15.0, 50.0, 400.0))]
    problems = _problems(specs)
    own = {id(p['objectives']): b for b, p in enumerate(problems)}

    def run(fn):
        events = []

        def check(result):  # replica 1 stops after its first iteration
            b = own[id(result.objectives)]
            events.append(('check', b, result.iters[-1]))
            return 'enough' if (b == 1 and result.iters[-1] >= 1) else None

        sigmas = [_recording_sigma(events, b, spec.tlist[-1]) for b, spec in enumerate(specs)]
        return fn(problems, sigmas, iter_stop=3, store_all_pulses=True, check_convergence=check, **_shared_kw()), events

    results, ev_b = run(lambda problems, sigmas, **kw: krotov_amd.optimize_pulses_batch(problems, sigma=sigmas, **kw))
    eng = replica_double_so.created[0]
    loop, ev_s = run(_loop_so)
    for res, seq in zip(results, loop):
        _same_result(res, seq)
    assert [r.iters[-1] for r in results] == [3, 1, 3]
    refreshes = [e for e in ev_b if e[0] == 'refresh']
    assert sorted((e[1], e[2]) for e in refreshes) == [(0, 1), (0, 2), (2, 1), (2, 2)]  # never replica 1, never the last
    assert sorted((e[1], e[2]) for e in ev_s if e[0] == 'refresh') == sorted((e[1], e[2]) for e in refreshes)
    for e in refreshes:
        _, b, it, objectives, result, n_obj, n_t, same = e
        assert ev_b.index(('check', b, it)) < ev_b.index(e)  # after the stopping decision
        assert objectives is problems[b]['objectives'] and result is results[b]
        assert (n_obj, n_t, same) == (3, 9, True)
    # the stopped replica is frozen through the mask while the others go on
    masks = [m for name, m in eng.sweeps if name == 'update']
    assert masks == [[1, 1, 1], [1, 0, 1], [1, 0, 1]]


def test_sigma_of_the_wrong_length_and_the_sequential_fallback(replica_double_so, caplog):
    import krotov_amd

    problems = _problems(_opt_specs('L1_small', B=3))
    with pytest.raises(ValueError):
        krotov_amd.optimize_pulses_batch(problems, sigma=[product_sigma() for _ in range(2)], iter_stop=1, **_shared_kw())
    # N = 17 does not fit a replica engine: problem by problem, each with its own sigma
    specs = [configs.config_c5(K=2, N=17, nt=7, distinct=True, seed=b, lambda_a=20.0 * (1 + b)) for b in range(2)]
    problems = _problems(specs)
    sig_b, sig_s = [product_sigma() for _ in range(2)], [product_sigma() for _ in range(2)]
    with caplog.at_level(logging.INFO, logger='krotov'):
        results = krotov_amd.optimize_pulses_batch(problems, sigma=sig_b, iter_stop=3, store_all_pulses=True, **_shared_kw())
    assert sum('optimize_pulses_batch: sequential' in rec.getMessage() for rec in caplog.records) == 1
    assert all(not e.replicas for e in replica_double_so.created)
    loop = _loop_so(problems, sig_s, iter_stop=3, store_all_pulses=True, **_shared_kw())
    for res, seq, sb, ss in zip(results, loop, sig_b, sig_s):
        _same_result(res, seq)
        assert len(sb.calls) == 2 and sb.history == ss.history
    assert sig_b[0].history != sig_b[1].history


def test_second_order_batch_counts_three_stores_per_replica(replica_double_so, monkeypatch, caplog):
    import krotov_amd
    import krotov_amd.batch as batch_mod
    from replica_double import ReplicaEngineDouble

    problems = _problems(_opt_specs('L1_small', B=4))
    store = 3 * 9 * 5 * 16  # K_r nt N 16 bytes
    monkeypatch.setattr(batch_mod, '_free_device_bytes', lambda: 4 * (2 * 3 * store + 1))  # a quarter: three stores of two
    sigmas = [product_sigma() for _ in range(4)]
    with caplog.at_level(logging.INFO, logger='krotov'):
        results = krotov_amd.optimize_pulses_batch(problems, sigma=sigmas, iter_stop=2, store_all_pulses=True, **_shared_kw())
    assert [e.replicas for e in replica_double_so.created] == [2, 2]
    assert any('sub-batches' in rec.getMessage() for rec in caplog.records)
    loop = _loop_so(problems, [product_sigma() for _ in range(4)], iter_stop=2, store_all_pulses=True, **_shared_kw())
    for res, seq in zip(results, loop):
        _same_result(res, seq)
    # first order under the same memory: one store per replica, all four fit
    ReplicaEngineDouble.created = []
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='krotov'):
        krotov_amd.optimize_pulses_batch(problems, iter_stop=1, **_shared_kw())
    assert [e.replicas for e in ReplicaEngineDouble.created] == [4]
    assert not any('sub-batches' in rec.getMessage() for rec in caplog.records)
    # ... down to the point where one store per replica still just fits
    ReplicaEngineDouble.created = []
    monkeypatch.setattr(batch_mod, '_free_device_bytes', lambda: 4 * (4 * store))
    krotov_amd.optimize_pulses_batch(problems, iter_stop=1, **_shared_kw())
    assert [e.replicas for e in ReplicaEngineDouble.created] == [4]


def test_set_second_order_replicas_is_exported_and_checks_its_engine():
    from krotov_amd import _lib

    lib = _lib.load()
    assert 'kh_set_second_order_replicas' in _lib.SYMBOLS and hasattr(lib, 'kh_set_second_order_replicas')
    assert lib.kh_set_second_order_replicas(None, None, None, None) == -1 == _lib.KH_ERR_INVALID
    assert b'null' in lib.kh_last_error()
    names = _lib.kernel_instantiations()
    for L in (1, 2, 3, 4):  # the first-order kernels keep their names next to the new ones
        assert 'kh_rep_forward_update<%d>' % L in names and 'kh_rep_forward_update_so<%d>' % L in names
