"""The perfect-entangler and local-invariants functionals (krotov_amd/functionals.py: ``PerfectEntanglerChi``,
``LocalInvariantsChi``, ``local_invariants``, ``F_PE``) and their co-states on the device (``kh_chi_local_invariants``,
krotov_amd/csrc/kh_chi_li.h) -- what the reference's notebook 07 takes from the ``weylchamber`` package.

Host: the invariants of known gates, the co-states against the central-difference Wirtinger gradient of a NumPy
restatement of J written here, notebook 07's problem and a local-invariants run towards CNOT through the oracle
(tests/golden/nb07_pe_table.json: the notebook's own table), the error paths.  GPU: the kernel against the host
constructor on every engine kind it serves (1e-12, the project's tolerance against its NumPy oracle; bitwise repeatable
and independent of a gate's place in the batch), the active mask, guarded buffers, the error codes, and ``optimize_pulses``
/ ``optimize_pulses_batch`` end to end against the oracle run of the host tests on a 41-point grid."""
import functools
import json
import os

import numpy as np
import pytest

import helpers
from krotov_amd import configs
from oracle import krotov_oracle as ko

TOL = 1e-12  # the project's tolerance against its NumPy oracle (Hilbert space)
TOL_REFERENCE = 1e-9  # ... against reference results (several iterations)

S2 = 1.0 / np.sqrt(2.0)
IDENTITY = np.eye(4, dtype=np.complex128)
CNOT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.complex128)
CZ = np.diag([1, 1, 1, -1]).astype(np.complex128)
SQRT_ISWAP = np.array([[1, 0, 0, 0], [0, S2, 1j * S2, 0], [0, 1j * S2, S2, 0], [0, 0, 0, 1]], dtype=np.complex128)
# the Bell states of gate_objectives(gate='PE') in the canonical basis, row i = B_i (restated here)
BELL = np.array([[1, 0, 0, 1], [0, 1j, 1j, 0], [0, 1, -1, 0], [1j, 0, 0, -1j]], dtype=np.complex128) * S2
MODES = ('PE', 'LI')
WEIGHTS = (0.0, 0.3)


# ---------------------------------------------------------------------------
# the test's own restatement of J (nothing of it imported from the package)
# ---------------------------------------------------------------------------
def restated_invariants(U_B):
    m = U_B.T @ U_B
    t, d = np.trace(m), np.linalg.det(U_B)
    return t * t / (16 * d), (t * t - np.trace(m @ m)) / (4 * d)


def restated_J(U_B, mode, target, w):
    G, H = restated_invariants(U_B)
    if mode == 'PE':
        F = H.real * abs(G) - G.real
    else:
        F = abs(G - target[0]) ** 2 + (H.real - target[1]) ** 2
    return (1 - w) * F + w * (1 - np.trace(U_B.conj().T @ U_B).real / 4)


def restated_target(gate):
    G, H = restated_invariants(BELL.conj() @ gate @ BELL.T)
    return G, H.real


def bell_of(basis):
    """B_i = sum_j BELL[i, j] basis[j] for a canonical basis given as rows."""
    return BELL @ np.asarray(basis)


def constructor(mode, basis, w=0.0, gate=CNOT):
    from krotov_amd import functionals

    if mode == 'PE':
        return functionals.PerfectEntanglerChi(list(basis), unitarity_weight=w)
    return functionals.LocalInvariantsChi(gate, list(basis), unitarity_weight=w)


def noisy_gate(rng, noise=0.05):
    """A seeded non-unitary U_B: unitary + noise."""
    q, _ = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))
    return q + noise * (rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))


def frame(rng, N):
    """A canonical basis: four orthonormal rows in C^N (N = 4: the unit vectors; N = 9: the logical subspace
    |00>, |01>, |10>, |11> of two qutrits; else seeded)."""
    if N == 4:
        return np.eye(4, dtype=np.complex128)
    if N == 9:
        return np.eye(9, dtype=np.complex128)[[0, 1, 3, 4]]
    q, _ = np.linalg.qr(rng.standard_normal((N, 4)) + 1j * rng.standard_normal((N, 4)))
    return np.ascontiguousarray(q.T)


def states_of(rng, basis, U_B, leak=0.1):
    """phi_k = sum_i U_B[i, k] B_i (+ seeded population outside the subspace where there is room)."""
    bell = bell_of(basis)
    psi = U_B.T @ bell
    N = bell.shape[1]
    if N > 4:
        out = rng.standard_normal((4, N)) + 1j * rng.standard_normal((4, N))
        out -= (out @ bell.conj().T) @ bell  # orthogonal to the subspace: U_B stays what it is
        psi = psi + leak * out
    return psi


# ---------------------------------------------------------------------------
# host: invariants, gradient, error paths
# ---------------------------------------------------------------------------
def test_invariants_of_known_gates():
    from krotov_amd import functionals

    for gate, want, fpe in ((IDENTITY, (1, 0, 3), 2), (CNOT, (0, 0, 1), 0), (CZ, (0, 0, 1), 0), (SQRT_ISWAP, (0.25, 0, 1), 0)):
        g = functionals.local_invariants(gate)
        assert np.abs(np.array(g) - np.array(want)).max() < 1e-14, (g, want)
        assert abs(functionals.F_PE(*g) - fpe) < 1e-14
    # invariance under k1 U k2 with local k1, k2
    rng = np.random.default_rng(7)

    def local(rng):
        qs = [np.linalg.qr(rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2)))[0] for _ in range(2)]
        return np.kron(qs[0], qs[1])

    for gate in (CNOT, SQRT_ISWAP, np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0]):
        g = np.array(functionals.local_invariants(gate))
        for _ in range(3):
            g2 = np.array(functionals.local_invariants(local(rng) @ gate @ local(rng)))
            assert np.abs(g2 - g).max() < 1e-12
    # the Bell basis is the one gate_objectives uses, and the weylchamber names give the same objects
    import krotov_amd

    basis = [np.eye(4, dtype=np.complex128)[j].reshape(-1, 1) for j in range(4)]
    objs = krotov_amd.gate_objectives(basis, 'PE', [IDENTITY])
    for obj, b, mine in zip(objs, functionals.bell_basis(basis), BELL):
        assert np.array_equal(np.asarray(obj.initial_state), np.asarray(b))
        assert np.abs(np.asarray(b).ravel() - mine).max() < 1e-16
    assert isinstance(functionals.make_PE_krotov_chi_constructor(basis), functionals.PerfectEntanglerChi)
    li = functionals.make_LI_krotov_chi_constructor(CNOT, basis, unitarity_weight=0.25)
    assert isinstance(li, functionals.LocalInvariantsChi) and li.unitarity_weight == 0.25
    assert abs(li.target_invariants[0]) < 1e-15 and abs(li.target_invariants[1] - 1) < 1e-15


@pytest.mark.parametrize('N', [4, 9])
@pytest.mark.parametrize('w', WEIGHTS)
@pytest.mark.parametrize('mode', MODES)
def test_costates_are_the_wirtinger_gradient(mode, w, N):
    """chi_k = -dJ / d<phi_k| by central differences (step 1e-6: accurate to ~1e-10 here, asserted at 1e-7) of the
    restatement above, for two gates at once (an ensemble: J is their mean)."""
    rng = np.random.default_rng(100 * N + 10 * MODES.index(mode) + int(10 * w))
    basis = frame(rng, N)
    bell = bell_of(basis)
    con = constructor(mode, basis, w)
    psi = np.concatenate([states_of(rng, basis, noisy_gate(rng)) for _ in range(2)])
    target = restated_target(CNOT)

    def J_of(states):
        vals = [restated_J(bell.conj() @ states[4 * g:4 * g + 4].T, mode, target, w) for g in range(2)]
        return vals, float(np.mean(vals))

    chis = con(list(psi), None, None)
    assert np.abs(con.values - J_of(psi)[0]).max() < 1e-13
    con.values = None
    assert abs(con.J_T(list(psi)) - J_of(psi)[1]) < 1e-13 and con.values is None  # (.values: the co-states' calls)
    h, worst = 1e-6, 0.0
    for k in range(8):
        for n in range(N):
            def shifted(z):
                moved = psi.copy()
                moved[k, n] += z
                return J_of(moved)[1]

            grad = 0.5 * ((shifted(h) - shifted(-h)) / (2 * h) + 1j * (shifted(1j * h) - shifted(-1j * h)) / (2 * h))
            worst = max(worst, abs(-grad - chis[k][n]))
    print("%s w=%.1f N=%d: |chi + dJ/d<phi|| <= %.2e" % (mode, w, N, worst))
    assert worst < 1e-7


@pytest.mark.parametrize('mode', MODES)
def test_costates_are_finite_exactly_at_cnot(mode):
    basis = frame(None, 4)
    con = constructor(mode, basis)
    psi = (BELL.conj() @ CNOT @ BELL.T).T @ bell_of(basis)  # U_B of CNOT, |G| = 0
    chis = np.array(con(list(psi), None, None))
    assert np.isfinite(chis).all() and abs(con.values[0]) < 1e-15
    # states of the caller's type: column vectors in, column vectors out
    cols = constructor(mode, [b.reshape(-1, 1) for b in basis])([p.reshape(-1, 1) for p in psi], None, None)
    assert all(c.shape == (4, 1) for c in cols) and np.array_equal(np.array(cols).reshape(4, 4), chis)


def test_error_paths():
    import krotov_amd

    rng = np.random.default_rng(3)
    basis = frame(rng, 4)
    psi = states_of(rng, basis, noisy_gate(rng))
    for mode in MODES:
        con = constructor(mode, basis)
        with pytest.raises(ValueError, match='4 objectives per gate'):
            con(list(psi) + [psi[0]], None, None)
        with pytest.raises(ValueError, match='4 objectives per gate'):
            con.J_T(list(psi) + [psi[0]])
        objs = [krotov_amd.Objective(initial_state=b, target='PE', H=[IDENTITY]) for b in bell_of(basis)]
        assert len(con(list(psi), objs, None)) == 4
        objs[2].weight = 0.5
        with pytest.raises(ValueError, match='weight'):
            con(list(psi), objs, None)
        same = psi.copy()
        same[3] = same[1]
        with pytest.raises(ValueError, match='linearly dependent'):
            con(list(same), None, None)
        with pytest.raises(ValueError, match='linearly dependent'):
            con.J_T(list(same))
    with pytest.raises(ValueError):
        constructor('PE', basis, w=1.5)


# ---------------------------------------------------------------------------
# notebook 07's problem (and the local-invariants run towards CNOT) through the oracle
# ---------------------------------------------------------------------------
def nb07_spec(nt, amplitude=0.3):
    """Notebook 07's system (krotov_amd.configs.config_c3: its Hamiltonian, guess, shape and lambda_a = 100) with the
    Bell states as initial states; ``amplitude`` scales the guess (the notebook's is 0.3)."""
    spec = configs.config_c3(nt=nt)
    spec.init = BELL.copy()
    guess = spec.controls[0]
    spec.controls = [lambda t, args, g=guess, s=amplitude / 0.3: s * g(t, args)]
    return spec


class OracleSigma:
    """The notebook's sigma class (cell 30, epsA = 0) in the oracle's array form: A from ``numerical_estimate_A``, Delta
    J_T from the constructor's ``J_T``."""

    def __init__(self, con):
        self.A, self.con, self.J, self.history = 0.0, con, [], []

    def __call__(self, t):
        return -max(0.0, 2 * self.A)

    def refresh(self, fw_T, fw_T0, chi_T, chi_norms, taus):
        if not self.J:
            self.J.append(self.con.J_T(list(fw_T0)))
        self.J.append(self.con.J_T(list(fw_T)))
        self.A = ko.numerical_estimate_A(fw_T, fw_T0, chi_T, chi_norms, self.J[-1] - self.J[-2])
        self.history.append(self.A)


@functools.lru_cache(maxsize=None)
def oracle_run(mode, nt, iters, amplitude=0.3):
    """``oracle.krotov_oracle.optimize`` as it is, second order, with the new constructor as its chi_constructor.
    dict(all_pulses, J: the functional after every iteration, chi: the un-normalised co-states of every iteration,
    g_a, A)."""
    spec = nb07_spec(nt, amplitude)
    con = constructor(mode, frame(None, 4))
    sig = OracleSigma(con)
    chis = []

    def chi_constructor(problem, fw_T, tau):
        chis.append(np.array(con(list(fw_T), None, tau)))
        return chis[-1]

    gp, S, lam = helpers.oracle_controls(spec)
    with helpers.MemoExpm():
        out = ko.optimize(helpers.spec_to_oracle(spec), gp, S, lam, chi_constructor, iters, sigma=sig)
    return dict(all_pulses=out['all_pulses'], J=list(sig.J), chi=chis, g_a=out['g_a'], A=list(sig.history))


def test_notebook_07_through_the_oracle():
    """F_PE at iteration 0 is the notebook's; it falls monotonically and reaches a perfect entangler (F_PE <= 0) at
    iteration 8 and not before, like the notebook.  Rows 1-8 of the notebook's table are not asserted: weylchamber's
    own gradient is not available here and its step differs (0.998102 after one iteration, 1.076839 here)."""
    with open(os.path.join(helpers.GOLDEN, 'nb07_pe_table.json')) as f:
        table = json.load(f)
    J = oracle_run('PE', 250, 8)['J']
    print("F_PE per iteration: %s (notebook: %s)" % (", ".join("%.6f" % x for x in J), table['F_PE']))
    assert len(J) == 9 == len(table['F_PE'])
    assert abs(J[0] - table['F_PE'][0]) < 1e-6 and table['F_PE'][0] == 1.447335
    assert all(b < a for a, b in zip(J, J[1:]))
    assert J[8] <= 0 and all(x > 0 for x in J[:8])
    assert table['F_PE'][8] <= 0 and all(x > 0 for x in table['F_PE'][:8])
    trial = (1.447335, 1.076839, 0.650446, 0.318097, 0.146600, 0.065953, 0.025773, 0.004146, -0.008310)
    assert np.abs(np.array(J) - trial).max() < 1e-6


def test_local_invariants_towards_cnot_through_the_oracle():
    J = oracle_run('LI', 250, 5)['J']
    print("J_LI per iteration: %s" % ", ".join("%.6f" % x for x in J))
    assert all(b < a for a, b in zip(J, J[1:]))
    assert J[3] < 0.1
    assert np.abs(np.array(J[:4]) - (3.598763, 1.189085, 0.092147, 0.083244)).max() < 1e-6


# ---------------------------------------------------------------------------
# host: the routing of the two drivers on oracle-backed engine doubles
# ---------------------------------------------------------------------------
@pytest.fixture
def li_double(monkeypatch):
    """``ReplicaEngineDoubleSO`` with ``chi_local_invariants`` (the host algebra, gate by gate, honouring the mask and
    reporting a singular gate the kernel's way)."""
    import torch

    import krotov_amd.engine as engine_mod
    from krotov_amd import functionals
    from replica_double import ReplicaEngineDouble
    from replica_double_so import ReplicaEngineDoubleSO

    class Double(ReplicaEngineDoubleSO):
        li_calls = 0

        def chi_local_invariants(self, psi_T, bell, mode, invariants=None, unitarity_weight=0.0, scale=1.0, out=None):
            psi, bell = self.dev(psi_T, torch.complex128).numpy(), self.dev(bell, torch.complex128).numpy()
            M = self.K // 4
            out = (None, None, None) if out is None else out
            chi = self._buffer(out[0], (self.K, self.N), torch.complex128)
            norms = self._buffer(out[1], (self.K,), torch.float64)
            J = self._buffer(out[2], (M,), torch.float64)
            target = None if invariants is None else (complex(invariants[0], invariants[1]), float(invariants[2]))
            mask = self.mask if self.replicas else [1] * M
            for g in range(M):
                if not mask[g * 4 // (self.Kr if self.replicas else 4)]:
                    continue
                try:
                    value, D = functionals._li_gate_terms(bell.conj() @ psi[4 * g:4 * g + 4].T, MODES.index(mode), target,
                                                          unitarity_weight)
                except ValueError:  # a singular U_B, as the kernel reports it: zero rows, norms 0, J NaN
                    chi[4 * g:4 * g + 4], norms[4 * g:4 * g + 4], J[g] = 0.0, 0.0, float('nan')
                    continue
                rows = -scale * (D.T @ bell)
                nrm = np.linalg.norm(rows, axis=1)
                chi[4 * g:4 * g + 4] = torch.from_numpy(rows / nrm[:, None])
                norms[4 * g:4 * g + 4] = torch.from_numpy(nrm)
                J[g] = value
            Double.li_calls += 1
            return chi, norms, J

    monkeypatch.setattr(engine_mod, 'HipKrotovEngine', Double)
    ReplicaEngineDouble.created = []
    return Double


def test_drivers_route_the_object_to_the_engine_and_a_batch_is_the_loop(li_double, caplog):
    """On the doubles: the object itself goes through ``chi_local_invariants`` (one call per iteration, of the batch or
    of the single problem), a lambda around it does not; ``optimize_pulses`` runs a one-gate problem as a batch of one on
    a replica engine, and ``results[b]`` of the batch is that run bit for bit -- sigma's A history and the co-states
    handed to ``refresh`` included."""
    import logging

    import krotov_amd
    from replica_double import ReplicaEngineDouble
    from test_replicas import _same_result

    built = [product_problem(13, a) for a in AMPLITUDES]
    problems, con = [p for p, _ in built], built[0][1]
    hook = lambda **kw: con.J_T(kw['fw_states_T'], kw['objectives'])  # noqa: E731
    sigmas = [product_sigma() for _ in problems]
    results = krotov_amd.optimize_pulses_batch(problems, propagator=krotov_amd.propagators.expm, chi_constructor=con,
                                               sigma=sigmas, iter_stop=3, store_all_pulses=True, info_hook=hook)
    assert [e.replicas for e in ReplicaEngineDouble.created] == [3] and li_double.li_calls == 3
    assert con.values.shape == (3,) and np.abs(con.values - [r.info_vals[-2] for r in results]).max() < 1e-13
    for b, (res, sig) in enumerate(zip(results, sigmas)):
        ref = oracle_run('PE', 13, 3, AMPLITUDES[b])
        assert deviations(res, sig, ref)[1] < 1e-12
        ReplicaEngineDouble.created, li_double.li_calls = [], 0
        solo_sigma = product_sigma()
        solo = run_product(problems[b], con, solo_sigma)
        assert [e.replicas for e in ReplicaEngineDouble.created] == [1] and li_double.li_calls == 3
        _same_result(res, solo)
        assert sig.history == solo_sigma.history and all(np.array_equal(x, y) for x, y in zip(sig.chi, solo_sigma.chi))
    # the host route: a plain function around the object -- the engine a small problem gets otherwise, no device call
    ReplicaEngineDouble.created, li_double.li_calls = [], 0
    host_sigma = product_sigma()
    host = run_product(problems[0], con, host_sigma, chi_constructor=lambda **kw: con(**kw))
    assert [e.replicas for e in ReplicaEngineDouble.created] == [0] and li_double.li_calls == 0
    assert np.abs(np.array(host.all_pulses) - np.array(results[0].all_pulses)).max() < 1e-12
    # two gates per problem: the batch calls the object on the host and says why
    two = dict(problems[0], objectives=list(problems[0]['objectives']) + list(problems[1]['objectives']))
    two['pulse_options'] = {**problems[0]['pulse_options'], **problems[1]['pulse_options']}
    li_double.li_calls = 0
    with caplog.at_level(logging.INFO, logger='krotov'):
        krotov_amd.optimize_pulses_batch([two], propagator=krotov_amd.propagators.expm, chi_constructor=con,
                                         sigma=[product_sigma()], iter_stop=1, info_hook=hook)
    assert li_double.li_calls == 0 and any('co-states on the host' in rec.getMessage() for rec in caplog.records)


# ---------------------------------------------------------------------------
# GPU: the kernel against the host constructor
# ---------------------------------------------------------------------------
def _engine(kind, K, N, B=0, cls=None, **kw):
    import scipy.sparse as sp

    from krotov_amd.engine import HipKrotovEngine

    cls = HipKrotovEngine if cls is None else cls
    rng = np.random.default_rng(1000 + 10 * K + N)
    if kind == 'uniform':  # every objective the same operator objects
        H0, H1 = configs.herm(rng, N, 1.0), configs.herm(rng, N, 0.5)
        ops = [[H0, H1]] * K
    elif kind == 'csr':
        ops = [[sp.csr_matrix(configs.herm(rng, N, 1.0)), sp.csr_matrix(configs.herm(rng, N, 0.5))] for _ in range(K)]
    else:
        ops = [[configs.herm(rng, N, 1.0), configs.herm(rng, N, 0.5)] for _ in range(K)]
    if B:
        return cls(ops, np.full((B, 4), 0.1), replicas=B, **kw)
    return cls(ops, np.full(4, 0.1), **kw)


GATES = (CNOT, SQRT_ISWAP, CZ)


def _case(N, M, per_gate, seed):
    """psi (4 M, N), the Bell states ((4, N) or (M, 4, N)), the target gates, and the host constructors' reference:
    ref(mode, w, scale) -> (chi un-normalised (4 M, N), J (M,))."""
    rng = np.random.default_rng(seed)
    bases = [frame(rng, N) for _ in range(M)] if per_gate and N > 4 else [frame(rng, N)] * M
    if per_gate and N == 4:  # (another orthonormal basis of the whole space per gate)
        bases = [np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0].T for _ in range(M)]
    psi = np.concatenate([states_of(rng, bases[g], noisy_gate(rng)) for g in range(M)])
    bell = np.array([bell_of(b) for b in bases]) if per_gate else bell_of(bases[0])
    gates = [GATES[g % 3] for g in range(M)] if per_gate else [CNOT] * M

    def ref(mode, w, scale):
        chi, J = [], []
        for g in range(M):
            con = constructor(mode, bases[g], w, gates[g])
            chi.append(scale * np.array(con(list(psi[4 * g:4 * g + 4]), None, None)))
            J.append(con.values[0])
        return np.concatenate(chi), np.array(J)

    def invariants():
        rows = np.array([[t[0].real, t[0].imag, t[1]] for t in (restated_target(g) for g in gates)])
        return rows if per_gate else rows[0]

    return psi, bell, ref, invariants()


KERNEL_CASES = {
    'uniform_K4_N4': ('uniform', 4, 4, 0, False),
    'dense_K8_N9': ('dense', 8, 9, 0, False),
    'dense_K4_N70': ('dense', 4, 70, 0, False),
    'csr_K4_N9': ('csr', 4, 9, 0, False),
    'replica_B3_N4': ('dense', 12, 4, 3, False),
    'replica_B3_N9': ('dense', 12, 9, 3, False),
    'replica_B3_N9_per_gate': ('dense', 12, 9, 3, True),
    'replica_B3_N4_per_gate': ('dense', 12, 4, 3, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KERNEL_CASES))
def test_kernel_vs_host_constructor(name):
    """chi_T x norm and J of ``kh_chi_local_invariants`` against the host constructor to 1e-12, both modes, w in
    {0, 0.3}; a second call and a gate moved to another place in the batch give the same bits."""
    kind, K, N, B, per_gate = KERNEL_CASES[name]
    M = K // 4
    psi, bell, ref, inv = _case(N, M, per_gate, seed=sum(map(ord, name)))
    scale = 1.0 if B else 1.0 / M
    eng = _engine(kind, K, N, B)
    try:
        for mode in MODES:
            for w in WEIGHTS:
                chi, norms, J = (x.cpu().numpy() for x in eng.chi_local_invariants(psi, bell, mode, inv, w, scale))
                want_chi, want_J = ref(mode, w, scale)
                errs = dict(chi=np.abs(chi * norms[:, None] - want_chi).max(), J=np.abs(J - want_J).max(),
                            norm=np.abs(np.linalg.norm(chi, axis=1) - 1).max())
                print("%s %s w=%.1f: %s" % (name, mode, w, ", ".join("%s %.2e" % kv for kv in errs.items())))
                assert all(err < TOL for err in errs.values()), (name, mode, w, errs)
                again = [x.cpu().numpy() for x in eng.chi_local_invariants(psi, bell, mode, inv, w, scale)]
                assert all(np.array_equal(a, b) for a, b in zip(again, (chi, norms, J)))
                if M > 1:  # gate g at place (g + 1) % M
                    roll = lambda x, per=1: np.roll(x, per, axis=0)  # noqa: E731
                    moved = eng.chi_local_invariants(roll(psi, 4), roll(bell) if per_gate else bell, mode,
                                                     roll(inv) if per_gate else inv, w, scale)
                    moved = [x.cpu().numpy() for x in moved]
                    assert np.array_equal(roll(chi, 4), moved[0]) and np.array_equal(roll(norms, 4), moved[1])
                    assert np.array_equal(roll(J), moved[2])
    finally:
        eng.close()


@pytest.mark.gpu
def test_inactive_replica_keeps_its_slices():
    import torch

    psi, bell, ref, inv = _case(9, 3, True, seed=11)
    eng = _engine('dense', 12, 9, B=3)
    try:
        for mode in MODES:
            full = [x.cpu().numpy() for x in eng.chi_local_invariants(psi, bell, mode, inv, 0.3, 1.0)]
            eng.set_active_replicas([1, 0, 1])
            out = (torch.full((12, 9), 7.25 - 3j, dtype=torch.complex128, device='cuda'),
                   torch.full((12,), -7.25, dtype=torch.float64, device='cuda'),
                   torch.full((3,), -7.25, dtype=torch.float64, device='cuda'))
            got = [x.cpu().numpy() for x in eng.chi_local_invariants(psi, bell, mode, inv, 0.3, 1.0, out=out)]
            eng.set_active_replicas(None)
            assert np.all(got[0][4:8] == 7.25 - 3j) and np.all(got[1][4:8] == -7.25) and got[2][1] == -7.25
            for rows, gates in ((slice(0, 4), 0), (slice(8, 12), 2)):
                assert np.array_equal(got[0][rows], full[0][rows]) and np.array_equal(got[1][rows], full[1][rows])
                assert got[2][gates] == full[2][gates]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['dense_K8_N9', 'dense_K4_N70', 'replica_B3_N9_per_gate'])
def test_kernel_on_guarded_buffers(name):
    """The same call with every tensor carved from one arena (tests/guarded.py): minimally aligned, between NaN guard
    bands.  Guards and inputs are bytewise unchanged, the results still the host constructor's."""
    import torch

    from guarded import GuardedEngine

    kind, K, N, B, per_gate = KERNEL_CASES[name]
    M = K // 4
    psi, bell, ref, inv = _case(N, M, per_gate, seed=5)
    scale = 1.0 if B else 1.0 / M
    eng = _engine(kind, K, N, B, cls=GuardedEngine)
    try:
        arena = eng.arena
        t = dict(psi=arena.carve('li_psi', psi.shape, torch.complex128), bell=arena.carve('li_bell', bell.shape, torch.complex128),
                 inv=arena.carve('li_inv', inv.shape, torch.float64))
        for key, host in (('psi', psi), ('bell', bell), ('inv', inv)):
            t[key].copy_(torch.from_numpy(np.ascontiguousarray(host)))
        arena.check_layout()
        arena.snapshot()
        for mode in MODES:
            chi, norms, J = eng.chi_local_invariants(t['psi'], t['bell'], mode, t['inv'], 0.3, scale)
            torch.cuda.synchronize()
            arena.verify('chi_local_invariants ' + mode)
            for x in (chi, norms, J):  # (the results are the engine's: in the arena, between guards)
                assert arena._where(x.data_ptr() - arena.base)[1] == 'inside'
            want_chi, want_J = ref(mode, 0.3, scale)
            assert np.abs(chi.cpu().numpy() * norms.cpu().numpy()[:, None] - want_chi).max() < TOL
            assert np.abs(J.cpu().numpy() - want_J).max() < TOL
    finally:
        eng.close()


@pytest.mark.gpu
def test_error_codes_cnot_and_singular_gates():
    from krotov_amd import _lib

    rng = np.random.default_rng(2)
    lib = _lib.load()
    # decided before any HIP call: NULL arguments, K not divisible by 4, engines of the wrong kind
    assert lib.kh_chi_local_invariants(None, None, None, 0, 0, None, 0, 0.0, 1.0, None, None, None, None) == _lib.KH_ERR_INVALID
    eng = _engine('dense', 4, 4)
    assert lib.kh_chi_local_invariants(eng._handle, None, None, 0, 0, None, 0, 0.0, 1.0, None, None, None, None) == _lib.KH_ERR_INVALID
    basis = frame(rng, 4)
    psi = states_of(rng, basis, noisy_gate(rng))
    with pytest.raises(ValueError):
        eng.chi_local_invariants(psi, bell_of(basis), 'LI')  # no invariants
    with pytest.raises(ValueError):
        eng.chi_local_invariants(psi, bell_of(basis)[:3], 'PE')
    # exactly CNOT (|G| = 0): finite
    exact = (BELL.conj() @ CNOT @ BELL.T).T @ bell_of(basis)
    for mode in MODES:
        chi, norms, J = (x.cpu().numpy() for x in eng.chi_local_invariants(exact, bell_of(basis), mode, [0.0, 0.0, 1.0]))
        assert np.isfinite(chi).all() and np.isfinite(norms).all() and abs(J[0]) < 1e-15
        # two equal final states: NaN in J, zero rows, norms 0
        same = psi.copy()
        same[2] = same[0]
        chi, norms, J = (x.cpu().numpy() for x in eng.chi_local_invariants(same, bell_of(basis), mode, [0.0, 0.0, 1.0]))
        assert np.isnan(J[0]) and not chi.any() and not norms.any()
    eng.close()
    odd = _engine('dense', 5, 4)
    with pytest.raises(_lib.KrotovHipError) as err:
        odd.chi_local_invariants(np.zeros((5, 4)), bell_of(basis), 'PE')
    assert err.value.code == _lib.KH_ERR_INVALID
    odd.close()
    d = 2
    liouville = _engine('dense', 4, d * d, is_super=True)
    ops = [[configs.herm(rng, d, 1.0), configs.herm(rng, d, 0.5)] for _ in range(4)]
    lindblad = type(liouville)(ops, np.full(4, 0.1), c_ops=[[configs.herm(rng, d, 0.1)]] * 4)
    # objectives of two dimensions (4, 4, 3, 3; the buffers at stride 4): kh_engine_create_mixed
    mixed = type(liouville)([[configs.herm(rng, n, 1.0), configs.herm(rng, n, 0.5)] for n in (4, 4, 3, 3)], np.full(4, 0.1))
    assert mixed.mixed and mixed.N == 4 and mixed.kernel == 'generic/mixed'
    for engine in (liouville, lindblad, mixed):
        with pytest.raises(_lib.KrotovHipError) as err:
            engine.chi_local_invariants(psi, bell_of(basis), 'PE')
        assert err.value.code == _lib.KH_ERR_UNSUPPORTED
        engine.close()
    # a replica engine whose K is divisible by 4 and whose K_r is not (B = 2, K_r = 6): a gate would span two replicas
    spanning = _engine('dense', 12, 4, B=2)
    assert spanning.K == 12 and spanning.K // spanning.replicas == 6
    with pytest.raises(_lib.KrotovHipError) as err:
        spanning.chi_local_invariants(np.zeros((12, 4)), bell_of(basis), 'PE')
    assert err.value.code == _lib.KH_ERR_INVALID and 'per replica' in str(err.value)
    spanning.close()


# ---------------------------------------------------------------------------
# GPU: end to end
# ---------------------------------------------------------------------------
E2E_NT = 41
AMPLITUDES = tuple(0.3 * (0.7 + 0.6 * x) for x in np.random.default_rng(41).random(3))  # B = 3 random guesses


def product_problem(nt, amplitude=0.3, mode='PE'):
    """(objectives, pulse_options, tlist, constructor) of ``nb07_spec`` through the package's own interface."""
    import krotov_amd

    spec = nb07_spec(nt, amplitude)
    basis = [np.eye(4, dtype=np.complex128)[j].reshape(-1, 1) for j in range(4)]
    H = [spec.H0[0], [spec.Hc[0][0], spec.controls[0]]]
    if mode == 'PE':
        objectives = krotov_amd.gate_objectives(basis, 'PE', H)
    else:
        objectives = krotov_amd.gate_objectives(basis, CNOT, H, local_invariants=True)
    pulse_options = {spec.controls[0]: dict(lambda_a=spec.lambda_a, update_shape=spec.update_shape)}
    return dict(objectives=objectives, pulse_options=pulse_options, tlist=spec.tlist), constructor(mode, basis)


def product_sigma():
    """The notebook's sigma class (cell 30, epsA = 0): Delta J_T from ``result.info_vals`` (the hook below)."""
    from krotov_amd.second_order import Sigma, numerical_estimate_A

    class _Sigma(Sigma):
        def __init__(self):
            self.A, self.history, self.chi = 0.0, [], []

        def __call__(self, t):
            return -max(0.0, 2 * self.A)

        def refresh(self, forward_states, forward_states0, chi_states, chi_norms, optimized_pulses, guess_pulses,
                    objectives, result):
            self.chi.append(np.array([chi_norms[k] * np.asarray(chi_states[k]).ravel() for k in range(len(objectives))]))
            self.A = numerical_estimate_A(forward_states, forward_states0, chi_states, chi_norms,
                                          result.info_vals[-1] - result.info_vals[-2])
            self.history.append(self.A)

    return _Sigma()


def run_product(problem, con, sigma, chi_constructor=None, iters=3):
    import krotov_amd

    return krotov_amd.optimize_pulses(
        problem['objectives'], problem['pulse_options'], problem['tlist'], propagator=krotov_amd.propagators.expm,
        chi_constructor=con if chi_constructor is None else chi_constructor, sigma=sigma, iter_stop=iters,
        store_all_pulses=True, info_hook=lambda **kw: con.J_T(kw['fw_states_T'], kw['objectives']))


def deviations(res, sigma, ref):
    """Largest deviation of pulses (relative to max(1, max|.|)), functional values and co-states from the oracle run,
    after iteration 1 and after the last one."""
    got = np.array([np.array(p) for p in res.all_pulses])
    scale = max(1.0, np.abs(ref['all_pulses']).max())
    first = max(np.abs(got[1] - ref['all_pulses'][1]).max() / scale, np.abs(sigma.chi[0] - ref['chi'][0]).max(),
                abs(res.info_vals[1] - ref['J'][1]))
    last = max(np.abs(got - ref['all_pulses']).max() / scale, max(np.abs(a - b).max() for a, b in zip(sigma.chi, ref['chi'])),
               np.abs(np.array(res.info_vals) - ref['J']).max())
    return first, last


# Measured on an MI355X (profiles/local_invariants.txt): after iteration 3 the pulses, co-states and functional values
# deviate from the oracle run by at most 1.13e-14 (PE), 2.78e-14 (LI towards CNOT) and 3.80e-15 (the three replicas of the
# batch); asserted at ten times the largest, never looser than 1e-9.
E2E_MEASURED = 2.78e-14
E2E_BOUND = min(TOL_REFERENCE, 10 * E2E_MEASURED)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_optimize_pulses_vs_oracle_and_host_route(mode, caplog):
    """Notebook 07's problem (and the local-invariants run towards CNOT), second order, 3 iterations on the device route;
    the constructor wrapped in a lambda takes the host route and gives the same results to 1e-12."""
    import logging

    from krotov_amd import _lib

    ref = oracle_run(mode, E2E_NT, 3)
    problem, con = product_problem(E2E_NT, mode=mode)
    _lib.load()
    _lib.forget_launched_kernels()
    sig = product_sigma()
    with caplog.at_level(logging.INFO, logger='krotov'):
        res = run_product(problem, con, sig)
    assert 'kh_chi_li_kernel<%d>' % MODES.index(mode) in _lib.kernel_instantiations(launched_only=True)
    assert not any('co-states on the host' in rec.getMessage() for rec in caplog.records)
    # .values: the kernel's J where the co-states were last formed, from the states after iteration 2
    assert con.values.shape == (1,) and abs(con.values[0] - res.info_vals[-2]) < TOL
    first, last = deviations(res, sig, ref)
    print("%s device route vs oracle: after iteration 1 %.2e, after iteration 3 %.2e" % (mode, first, last))
    assert res.iters == [0, 1, 2, 3] and first < TOL and last < E2E_BOUND
    # the A/B switch: a plain function around the object
    _lib.forget_launched_kernels()
    sig_host = product_sigma()
    host = run_product(problem, con, sig_host, chi_constructor=lambda **kw: con(**kw))
    assert not any(n.startswith('kh_chi_li_kernel') for n in _lib.kernel_instantiations(launched_only=True))
    d = max(np.abs(np.array(res.all_pulses) - np.array(host.all_pulses)).max(),
            max(np.abs(a - b).max() for a, b in zip(sig.chi, sig_host.chi)),
            np.abs(np.array(res.info_vals) - np.array(host.info_vals)).max())
    print("%s device route vs host route: %.2e" % (mode, d))
    assert d < TOL


@pytest.mark.gpu
def test_batch_of_random_guesses_vs_oracle_and_solo_runs():
    """``optimize_pulses_batch`` on B = 3 copies of notebook 07's problem that differ in the guess amplitude: every
    replica against its own oracle run, and bit for bit what ``optimize_pulses`` gives for it alone."""
    import krotov_amd
    from krotov_amd import _lib
    from krotov_amd.engine import LAST_ENGINE
    from test_replicas import _same_result

    built = [product_problem(E2E_NT, a) for a in AMPLITUDES]
    problems, con = [p for p, _ in built], built[0][1]
    hook = lambda **kw: con.J_T(kw['fw_states_T'], kw['objectives'])  # noqa: E731
    sigmas = [product_sigma() for _ in problems]
    _lib.load()
    _lib.forget_launched_kernels()
    results = krotov_amd.optimize_pulses_batch(problems, propagator=krotov_amd.propagators.expm, chi_constructor=con,
                                               sigma=sigmas, iter_stop=3, store_all_pulses=True, info_hook=hook)
    assert LAST_ENGINE().kernel == 'replica16/wave'
    assert 'kh_chi_li_kernel<0>' in _lib.kernel_instantiations(launched_only=True)
    assert con.values.shape == (3,)  # (one gate per replica, from the kernel's J)
    assert np.abs(con.values - [res.info_vals[-2] for res in results]).max() < TOL
    for b, (a, res, sig) in enumerate(zip(AMPLITUDES, results, sigmas)):
        first, last = deviations(res, sig, oracle_run('PE', E2E_NT, 3, a))
        print("replica %d (guess amplitude %.4f): after iteration 1 %.2e, after iteration 3 %.2e" % (b, a, first, last))
        assert first < TOL and last < E2E_BOUND
        # the batch's own promise, bit for bit: a replica's result depends neither on B nor on its place in the batch
        one_sigma = product_sigma()
        one = krotov_amd.optimize_pulses_batch([problems[b]], propagator=krotov_amd.propagators.expm, chi_constructor=con,
                                               sigma=[one_sigma], iter_stop=3, store_all_pulses=True, info_hook=hook)[0]
        _same_result(res, one)
        assert sig.history == one_sigma.history and all(np.array_equal(x, y) for x, y in zip(sig.chi, one_sigma.chi))
        # ... and is optimize_pulses on the problem alone (which runs it as a batch of one), bit for bit
        solo_sigma = product_sigma()
        solo = run_product(problems[b], con, solo_sigma)
        assert LAST_ENGINE().kernel == 'replica16/wave'
        _same_result(res, solo)
        assert sig.history == solo_sigma.history and all(np.array_equal(x, y) for x, y in zip(sig.chi, solo_sigma.chi))
    # the host route of the batch: the object behind a plain function, replica by replica
    sig_host = [product_sigma() for _ in problems]
    host = krotov_amd.optimize_pulses_batch(problems, propagator=krotov_amd.propagators.expm,
                                            chi_constructor=lambda **kw: con(**kw), sigma=sig_host, iter_stop=3,
                                            store_all_pulses=True, info_hook=hook)
    for res, seq in zip(results, host):
        assert np.abs(np.array(res.all_pulses) - np.array(seq.all_pulses)).max() < TOL
        assert np.abs(np.array(res.info_vals) - np.array(seq.info_vals)).max() < TOL


@pytest.mark.gpu
def test_batch_replica_equals_its_solo_run_bit_for_bit():
    """``results[b]`` of the batch against ``optimize_pulses(**problems[b])``, bit for bit: ``optimize_pulses`` runs a
    one-gate problem under the constructor object as a batch of one on a replica engine (``_one_gate_replica_form``),
    the kernels the batch runs it on.  (The one-wave ``mini`` kernels, which a problem of this size gets under any other
    ``chi_constructor``, round differently: against them the final states of the initial forward sweep differ in the
    last bit -- measured J 1.39e-16, co-states of iteration 1 3.87e-16, pulses after three iterations 5.55e-17.)"""
    import krotov_amd
    from krotov_amd.engine import LAST_ENGINE

    problem, con = product_problem(E2E_NT, AMPLITUDES[1])
    hook = lambda **kw: con.J_T(kw['fw_states_T'], kw['objectives'])  # noqa: E731
    sig_b, sig_s = product_sigma(), product_sigma()
    res = krotov_amd.optimize_pulses_batch([problem] * 1, propagator=krotov_amd.propagators.expm, chi_constructor=con,
                                           sigma=[sig_b], iter_stop=3, store_all_pulses=True, info_hook=hook)[0]
    solo = run_product(problem, con, sig_s)
    assert LAST_ENGINE().kernel == 'replica16/wave'
    d_J0 = abs(res.info_vals[0] - solo.info_vals[0])
    d_chi1 = np.abs(sig_b.chi[0] - sig_s.chi[0]).max()
    d_pulses = np.abs(np.array(res.all_pulses) - np.array(solo.all_pulses)).max()
    print("batch vs solo run: J after the initial forward sweep %.2e, co-states of iteration 1 %.2e, pulses %.2e" % (
        d_J0, d_chi1, d_pulses))
    assert d_J0 == 0 and d_chi1 == 0 and d_pulses == 0


@pytest.mark.gpu
def test_singular_gate_raises_from_the_driver():
    """Two equal initial states stay equal: U_B is singular at T, the kernel reports NaN and the driver raises the
    host constructor's ValueError."""
    import krotov_amd

    problem, con = product_problem(9)
    objs = problem['objectives']
    objs[2] = krotov_amd.Objective(initial_state=objs[0].initial_state, target='PE', H=objs[0].H)
    with pytest.raises(ValueError, match='linearly dependent'):  # (no hook: nothing evaluates J on the host)
        krotov_amd.optimize_pulses(objs, problem['pulse_options'], problem['tlist'], propagator=krotov_amd.propagators.expm,
                                   chi_constructor=con, sigma=product_sigma(), iter_stop=1)
