"""Final-time functionals and the chi boundary conditions derived from them.

Same names, signatures and values as ``krotov.functionals`` (reference
src/krotov/functionals.py:82-437): a ``chi_constructor`` receives
``fw_states_T``, ``objectives``, ``tau_vals`` and returns one co-state per
objective.  They run once per iteration on K states (O(K N) work).

On the device path the optimiser does not call the four constructors below: each
is ``chi_k = c_k target_k + d_k phi_k(T)`` with per-objective scalars
(:func:`chi_coefficients`) and is formed and normalised in HBM by
``kh_chi_boundary``.  :func:`chi_stacked` is the same thing as a (K, N) array
expression on the host; the list forms are what user code calls.

The two gate functionals that are not linear in the states -- the perfect-entangler functional and the distance in the
local invariants (:class:`PerfectEntanglerChi`, :class:`LocalInvariantsChi`; the reference leaves them to the
``weylchamber`` package) -- are objects: callable as a ``chi_constructor`` on any backend, and formed on the device by
``kh_chi_local_invariants`` where the optimiser recognises an instance.
"""
import logging

import numpy as np

from .second_order import _overlap

__all__ = [
    'f_tau',
    'F_ss',
    'J_T_ss',
    'chis_ss',
    'F_sm',
    'J_T_sm',
    'chis_sm',
    'F_re',
    'J_T_re',
    'chis_re',
    'J_T_hs',
    'chis_hs',
    'F_avg',
    'gate',
    'mapped_basis',
    'bell_basis',
    'local_invariants',
    'F_PE',
    'PerfectEntanglerChi',
    'LocalInvariantsChi',
    'make_PE_krotov_chi_constructor',
    'make_LI_krotov_chi_constructor',
]


def _weight(obj):
    return getattr(obj, 'weight', None)


def _taus(fw_states_T, objectives, tau_vals):
    if tau_vals is None:
        return [_overlap(obj.target, psi) for psi, obj in zip(fw_states_T, objectives)]
    return tau_vals


def f_tau(fw_states_T, objectives, tau_vals=None, **kwargs):
    """(1/K) sum_k w_k tau_k  (reference functionals.py:82-141); a tau that is
    None (no forward propagation yet) is skipped with a warning."""
    total = 0j
    for obj, tau in zip(objectives, _taus(fw_states_T, objectives, tau_vals)):
        if tau is None:
            logging.getLogger('krotov').warning("τ is None in f_tau")
            continue
        w = _weight(obj)
        total += tau if w is None else w * tau
    return total / len(objectives)


def F_ss(fw_states_T, objectives, tau_vals=None, **kwargs):
    """(1/K) sum_k w_k |tau_k|^2  (reference functionals.py:116-162)."""
    abssq = [abs(t) ** 2 for t in _taus(fw_states_T, objectives, tau_vals)]
    F = f_tau(fw_states_T, objectives, abssq)
    assert abs(complex(F).imag) < 1e-10
    return complex(F).real


def J_T_ss(fw_states_T, objectives, tau_vals=None, **kwargs):
    return 1 - F_ss(fw_states_T, objectives, tau_vals)


def F_sm(fw_states_T, objectives, tau_vals=None, **kwargs):
    return abs(f_tau(fw_states_T, objectives, tau_vals)) ** 2


def J_T_sm(fw_states_T, objectives, tau_vals=None, **kwargs):
    return 1 - F_sm(fw_states_T, objectives, tau_vals)


def F_re(fw_states_T, objectives, tau_vals=None, **kwargs):
    return complex(f_tau(fw_states_T, objectives, tau_vals)).real


def J_T_re(fw_states_T, objectives, tau_vals=None, **kwargs):
    return 1 - F_re(fw_states_T, objectives, tau_vals)


def J_T_hs(fw_states_T, objectives, tau_vals=None, **kwargs):
    """Hilbert-Schmidt distance functional (reference functionals.py:320-386)."""
    taus = _taus(fw_states_T, objectives, tau_vals)
    total = 0.0
    for rho, obj, tau in zip(fw_states_T, objectives, taus):
        w = _weight(obj)
        nr = complex(_overlap(rho, rho)).real
        nt = complex(_overlap(obj.target, obj.target)).real
        term = nr + nt - 2 * complex(tau).real
        total += term if w is None else w * term
    return total / (2 * len(objectives))


def chis_ss(fw_states_T, objectives, tau_vals):
    """chi_k = (tau_k / K) w_k target_k  (reference functionals.py:177-197)."""
    K = len(objectives)
    out = []
    for obj, tau in zip(objectives, tau_vals):
        w = _weight(obj)
        out.append((tau / K) * obj.target if w is None else (tau / K) * w * obj.target)
    return out


def chis_sm(fw_states_T, objectives, tau_vals):
    """chi_k = w_k / K^2 (sum_j w_j tau_j) target_k  (reference functionals.py:225-253)."""
    s = 0
    for obj, tau in zip(objectives, tau_vals):
        w = _weight(obj)
        s += tau if w is None else w * tau
    c = 1.0 / len(objectives) ** 2
    out = []
    for obj in objectives:
        w = _weight(obj)
        out.append(c * obj.target * s if w is None else c * w * obj.target * s)
    return out


def chis_re(fw_states_T, objectives, tau_vals):
    """chi_k = w_k / (2K) target_k  (reference functionals.py:293-317)."""
    c = 1.0 / (2 * len(objectives))
    out = []
    for obj in objectives:
        w = _weight(obj)
        out.append(c * obj.target if w is None else c * w * obj.target)
    return out


def chis_hs(fw_states_T, objectives, tau_vals):
    """chi_k = w_k / (2K) (rho_target_k - rho_k(T))  (reference functionals.py:389-437)."""
    c = 1.0 / (2 * len(objectives))
    out = []
    for obj, rho in zip(objectives, fw_states_T):
        w = _weight(obj)
        out.append(c * (obj.target - rho) if w is None else c * w * (obj.target - rho))
    return out


def chi_stacked(chi_constructor, targets, weights, fw_T, tau):
    """(K, N) array form of the four constructors above, or None for any other
    ``chi_constructor``.  ``targets``, ``fw_T``: (K, N); ``weights``: (K,) or
    None; ``tau``: (K,) complex.  Same operation order as the list forms."""
    K = targets.shape[0]
    w = np.ones(K) if weights is None else weights
    if chi_constructor is chis_re:
        return ((1.0 / (2 * K)) * w)[:, None] * targets
    if chi_constructor is chis_ss:
        return ((np.asarray(tau) / K) * w)[:, None] * targets
    if chi_constructor is chis_sm:
        s = 0
        for wk, t in zip(w, tau):
            s += wk * t
        return ((1.0 / K**2) * w)[:, None] * targets * s
    if chi_constructor is chis_hs:
        return ((1.0 / (2 * K)) * w)[:, None] * (targets - fw_T)
    return None


def chi_coefficients(chi_constructor, weights, tau, K):
    """Per-objective scalars ``(c, d)`` with ``chi_k = c_k target_k + d_k phi_k(T)``
    for the four constructors above (None for any other ``chi_constructor``):
    what the device-side co-state construction (``kh_chi_boundary``) needs from
    the host.  ``weights``: (K,) or None; ``tau``: (K,) complex or None."""
    w = np.ones(K) if weights is None else np.asarray(weights, dtype=np.float64)
    zero = np.zeros(K, dtype=np.complex128)
    if chi_constructor is chis_re:
        return ((1.0 / (2 * K)) * w).astype(np.complex128), zero
    if chi_constructor is chis_hs:
        c = ((1.0 / (2 * K)) * w).astype(np.complex128)
        return c, -c
    if tau is None or any(t is None for t in tau):
        return None
    tau = np.asarray(tau, dtype=np.complex128)
    if chi_constructor is chis_ss:
        return (tau / K) * w, zero
    if chi_constructor is chis_sm:
        s = 0
        for wk, t in zip(w, tau):
            s += wk * t
        return ((1.0 / K**2) * w) * s, zero
    return None


# ---------------------------------------------------------------------------
# gate analysis (reference functionals.py:440-641); not on the optimisation path
# ---------------------------------------------------------------------------
def _arr(x):
    return np.asarray(x.full() if hasattr(x, 'full') else x, dtype=np.complex128)


def mapped_basis(O, basis_states):
    """The states ``sum_i O[i, j] basis_states[i]`` for every column j of the gate ``O`` (reference
    functionals.py:614-641); a tuple, each state of the basis states' type."""
    O = _arr(O)
    return tuple(
        sum(complex(O[i, j]) * basis_states[i] for i in range(O.shape[0])) for j in range(O.shape[1])
    )


def gate(basis_states, fw_states_T):
    """The N x N matrix ``U[i, j] = <basis_states[i]|fw_states_T[j]>`` that maps the basis states to the
    propagated states (reference functionals.py:590-611; a NumPy array here, there is no Qobj to wrap it)."""
    N = len(basis_states)
    U = np.zeros((N, N), dtype=np.complex128)
    for j in range(N):
        for i in range(N):
            U[i, j] = _overlap(basis_states[i], fw_states_T[j])
    return U


def F_avg(fw_states_T, basis_states, gate, mapped_basis_states=None, prec=1e-5):
    """Average gate fidelity with respect to ``gate`` (N x N, in the logical subspace) from the propagated
    logical basis (reference functionals.py:440-587): for N propagated state vectors
    ``(|tr(O^+ U)|^2 + tr(O^+ U U^+ O)) / (N (N + 1))`` with U from :func:`gate`; for the N^2 propagated dyads
    ``rho_ij = DynMap[|phi_i><phi_j|]`` (density matrices, ordered i N + j) the Liouville-space sum
    ``sum_ij <O phi_i|rho_ij|O phi_j> + <O phi_i|rho_jj|O phi_i>`` over ``N (N + 1)``.  ``prec`` bounds the
    imaginary part that errors in the states may leave."""
    make_gate = globals()['gate']  # (the argument shadows the function of the same name, as in the reference)
    N = len(basis_states)
    O = _arr(gate)
    if O.shape != (N, N):
        raise ValueError("Shape of gate is incompatible with number of basis states")
    first = _arr(fw_states_T[0])
    is_operator = first.ndim == 2 and first.shape[0] == first.shape[1] and first.shape[0] > 1
    if is_operator:
        if len(fw_states_T) != N * N:
            raise ValueError(
                "Evaluating F_avg for density matrices requires %d states (forward-propagation of all dyadic "
                "combinations of %d basis states), not %d" % (N * N, N, len(fw_states_T)))
        if mapped_basis_states is None:
            mapped_basis_states = mapped_basis(O, basis_states)
        mapped = [_arr(v).reshape(-1) for v in mapped_basis_states]
        F = 0.0
        for j in range(N):
            rho_jj = _arr(fw_states_T[j * N + j])
            for i in range(N):
                rho_ij = _arr(fw_states_T[i * N + j])
                F += np.vdot(mapped[i], rho_ij @ mapped[j]) + np.vdot(mapped[i], rho_jj @ mapped[i])
    else:
        if len(fw_states_T) != N:
            raise ValueError(
                "Evaluating F_avg for hilbert space states requires %d states (forward-propagation of all basis "
                "states), not %d" % (N, len(fw_states_T)))
        U = make_gate(basis_states, fw_states_T)
        OdU = O.conj().T @ U
        F = abs(np.trace(OdU)) ** 2 + np.trace(OdU @ OdU.conj().T)
    F = complex(F)
    assert abs(F.imag) < prec, "%.2e > %.2e" % (F.imag, prec)
    return F.real / (N * (N + 1))


# ---------------------------------------------------------------------------
# local invariants of two-qubit gates: the perfect-entangler and the local-invariants functional
# (P. Watts et al., Phys. Rev. A 91, 062306 (2015); M. H. Goerz et al., Phys. Rev. A 91, 062307 (2015); the reference's
# notebook 07 and its how-tos take both from the weylchamber package)
# ---------------------------------------------------------------------------
# B_i = sum_j _BELL[i][j] |j> over the canonical basis |00>, |01>, |10>, |11>
_BELL = (
    (1.0, 0.0, 0.0, 1.0),
    (0.0, 1j, 1j, 0.0),
    (0.0, 1.0, -1.0, 0.0),
    (1j, 0.0, 0.0, -1j),
)
# |det U_B| at or below this x (||U_B||_F / 2)^4 counts as singular (host and kernel use the same test)
LI_SINGULAR_RTOL = 1.0e-10
LI_MODE_PE, LI_MODE_LI = 0, 1


def bell_basis(canonical_basis):
    """The four Bell states ``(|00> + |11>)/sqrt 2, i(|01> + |10>)/sqrt 2, (|01> - |10>)/sqrt 2, i(|00> - |11>)/sqrt 2``
    of the canonical basis ``|00>, |01>, |10>, |11>`` (any state type with ``+`` and scalar ``*``): the initial states
    of ``gate_objectives(gate='PE')`` / ``(..., local_invariants=True)`` (reference objectives.py:1035-1051)."""
    if len(canonical_basis) != 4:
        raise ValueError("Optimization towards a two-qubit gate requires 4 basis_states")
    b = canonical_basis
    return [
        (b[0] + b[3]) / np.sqrt(2),
        (1j * b[1] + 1j * b[2]) / np.sqrt(2),
        (b[1] - b[2]) / np.sqrt(2),
        (1j * b[0] - 1j * b[3]) / np.sqrt(2),
    ]


def _invariants_of_bell_gate(U_B):
    """(G, H, t, d, m, ||U_B||_F^2) of a 4 x 4 gate in the Bell basis: m = U_B^T U_B, t = tr m, d = det U_B,
    G = t^2 / (16 d), H = (t^2 - tr m^2) / (4 d); ``ValueError`` where U_B is singular (``LI_SINGULAR_RTOL``)."""
    m = U_B.T @ U_B
    t = np.trace(m)
    d = np.linalg.det(U_B)
    fro2 = float(np.sum(np.abs(U_B) ** 2))
    if not abs(d) > LI_SINGULAR_RTOL * (fro2 / 4.0) ** 2:  # (a NaN counts as singular)
        raise ValueError(
            "the propagated Bell states are linearly dependent (|det U_B| = %.3e <= %.0e (||U_B||_F / 2)^4): the local "
            "invariants are not defined" % (abs(d), LI_SINGULAR_RTOL))
    G = t * t / (16.0 * d)
    H = (t * t - np.trace(m @ m)) / (4.0 * d)
    return G, H, t, d, m, fro2


def local_invariants(U):
    """The local invariants ``(g1, g2, g3)`` of a 4 x 4 two-qubit gate given in the canonical basis: with U_B the gate
    in the Bell basis of :func:`bell_basis` and m = U_B^T U_B, ``g1 + i g2 = tr(m)^2 / (16 det U)`` and
    ``g3 = Re (tr(m)^2 - tr(m^2)) / (4 det U)``.  They do not change under ``k1 U k2`` with local k1, k2 and (the
    determinant in the denominators) not under a scaling of U."""
    U = _arr(U)
    if U.shape != (4, 4):
        raise ValueError("local_invariants needs a 4 x 4 gate, not shape %s" % (U.shape,))
    Q = np.array(_BELL, dtype=np.complex128).T / np.sqrt(2)  # columns: the Bell states
    G, H = _invariants_of_bell_gate(Q.conj().T @ U @ Q)[:2]
    return float(G.real), float(G.imag), float(H.real)


def F_PE(g1, g2, g3):
    """The perfect-entangler functional ``g3 sqrt(g1^2 + g2^2) - g1``: zero on the boundary of the polyhedron of perfect
    entanglers in the Weyl chamber, negative inside it, 2 for the identity."""
    return g3 * np.sqrt(g1 * g1 + g2 * g2) - g1


def _li_gate_terms(U_B, mode, target, w):
    """``(J, D)`` of one gate: the functional's value and ``D[i, k] = dJ / d conj(U_B[i, k])``.  ``mode``:
    ``LI_MODE_PE`` or ``LI_MODE_LI`` with ``target = (G_O, g3_O)``; ``w``: the unitarity weight."""
    G, H, t, d, m, fro2 = _invariants_of_bell_gate(U_B)
    inv_T = np.linalg.inv(U_B).T
    dG = (t / (4.0 * d)) * U_B - G * inv_T
    dH = (t * U_B - U_B @ m) / d - H * inv_T
    g3 = H.real
    if mode == LI_MODE_PE:
        absG = abs(G)
        F = g3 * absG - G.real
        J_G = (g3 * np.conj(G) / (2.0 * absG) if absG > 0.0 else 0.0) - 0.5  # (dG vanishes together with G)
        J_H = 0.5 * absG
    else:
        G_O, g3_O = target
        F = abs(G - G_O) ** 2 + (g3 - g3_O) ** 2
        J_G = np.conj(G - G_O)
        J_H = g3 - g3_O
    J = (1.0 - w) * F + w * (1.0 - fro2 / 4.0)
    D = (1.0 - w) * np.conj(J_G * dG + J_H * dH) - (w / 4.0) * U_B
    return float(J), D


class _LocalInvariantsFunctional:
    """What :class:`PerfectEntanglerChi` and :class:`LocalInvariantsChi` share.  Per gate (4 consecutive objectives
    whose initial states are the Bell states B_i of the canonical basis), with U_B[i, k] = <B_i|phi_k(T)>:

        J = (1 - w) F(U_B) + w (1 - tr(U_B^+ U_B) / 4),      chi_k = -(1/M) sum_i (dJ / d conj U_B[i, k]) |B_i>

    and the functional of M gates (``len(objectives) == 4 M``: an ensemble) is the mean of their J.  U_B counts as
    singular -- ``ValueError`` -- where ``|det U_B| <= 1e-10 (||U_B||_F / 2)^4`` (1e-10 for a gate of unitary scale).

    ``.values`` AND ``.J_T`` ARE NOT THE SAME MOMENT.  ``.values`` is the J of every gate at the last CONSTRUCTION OF THE
    CO-STATES -- a call of the object, or the kernel's output where the optimiser forms them on the device (both routes
    fill it) -- that is, of the states an iteration STARTS from: after ``optimize_pulses`` returns it holds J of the
    states before the last update, one iteration behind what an ``info_hook`` saw.  ``.J_T(fw_states_T, ...)`` evaluates
    the functional of the states it is given and leaves ``.values`` alone, so a hook cannot overwrite the per-gate
    (per-problem, in a batch) values of the run with those of the one problem it was called for.

    IN A BATCH (``optimize_pulses_batch``) ``.values`` holds, after the call returns, the J of every gate of every problem
    in problem order, whether the problems ran as one batch, in sub-batches or one after another; a problem frozen early
    keeps the J of its last co-states.  While a split or sequential batch is still running, a hook finds there the
    running part only -- the problems of the sub-batch on the device, or the one problem of the sequential loop."""

    mode = None

    def __init__(self, canonical_basis, unitarity_weight=0.0):
        w = float(unitarity_weight)
        if not 0.0 <= w <= 1.0:
            raise ValueError("unitarity_weight must be in [0, 1], not %r" % (unitarity_weight,))
        self.unitarity_weight = w
        self.canonical_basis = list(canonical_basis)
        self.bell = bell_basis(self.canonical_basis)
        self.target_invariants = (0j, 0.0)
        self.values = None
        self.__name__ = type(self).__name__  # (hooks that print ``chi_constructor.__name__``)

    def check_objectives(self, n, objectives=None):
        """``ValueError`` unless ``n`` states / objectives are whole gates without weights."""
        if objectives is not None:
            if len(objectives) != n:
                raise ValueError("%d states for %d objectives" % (n, len(objectives)))
            if any(_weight(obj) is not None for obj in objectives):
                raise ValueError("%s does not take weighted objectives (Objective.weight)" % type(self).__name__)
        if n == 0 or n % 4 != 0:
            raise ValueError("%s needs 4 objectives per gate (the four Bell states), not %d" % (type(self).__name__, n))

    def device_arguments(self, vector_of):
        """What ``kh_chi_local_invariants`` needs from this object, or None: ``(mode, bell (4, N), invariants (3,),
        unitarity_weight)`` with ``vector_of(state)`` the engine's row of a state (None: it does not fit)."""
        rows = [vector_of(b) for b in self.bell]
        if any(r is None for r in rows):
            return None
        G_O, g3_O = self.target_invariants
        return ('PE' if self.mode == LI_MODE_PE else 'LI', np.array(rows, dtype=np.complex128),
                np.array([G_O.real, G_O.imag, g3_O], dtype=np.float64), self.unitarity_weight)

    def set_device_values(self, J, active=None):
        """``.values`` from the J per gate the device formed (``active``: the gates it worked on, default all); a NaN
        there is a singular U_B: ``ValueError``, as on the host."""
        J = np.array(J, dtype=np.float64)
        live = J if active is None else J[np.asarray(active, dtype=bool)]
        if np.isnan(live).any():
            raise ValueError(
                "the propagated Bell states are linearly dependent (|det U_B| <= %.0e (||U_B||_F / 2)^4): the local "
                "invariants are not defined" % LI_SINGULAR_RTOL)
        self.values = J

    def _gates(self, fw_states_T, objectives):
        n = len(fw_states_T)
        self.check_objectives(n, objectives)
        out = []
        for g in range(n // 4):
            U_B = np.empty((4, 4), dtype=np.complex128)
            for k in range(4):
                for i in range(4):
                    ov = _overlap(self.bell[i], fw_states_T[4 * g + k])
                    if ov is None:
                        raise ValueError("the propagated states do not match the canonical basis")
                    U_B[i, k] = ov
            out.append(U_B)
        return out

    def __call__(self, fw_states_T, objectives, tau_vals=None):
        gates = self._gates(fw_states_T, objectives)
        M = len(gates)
        values, chis = [], []
        for U_B in gates:
            J, D = _li_gate_terms(U_B, self.mode, self.target_invariants, self.unitarity_weight)
            values.append(J)
            for k in range(4):
                chis.append(sum(complex(-D[i, k] / M) * self.bell[i] for i in range(4)))
        self.values = np.array(values)
        return chis

    def J_T(self, fw_states_T, objectives=None, tau_vals=None, **kwargs):
        """The functional's value (raw: negative inside the polyhedron of perfect entanglers), the mean over the gates;
        usable as ``J_T`` of ``krotov_amd.info_hooks.print_table`` and for the Delta J_T of ``Sigma.refresh``."""
        gates = self._gates(fw_states_T, objectives)
        values = []
        for U_B in gates:
            G, H, _, _, _, fro2 = _invariants_of_bell_gate(U_B)
            if self.mode == LI_MODE_PE:
                F = H.real * abs(G) - G.real
            else:
                F = abs(G - self.target_invariants[0]) ** 2 + (H.real - self.target_invariants[1]) ** 2
            values.append(float((1.0 - self.unitarity_weight) * F + self.unitarity_weight * (1.0 - fro2 / 4.0)))
        return float(np.mean(values))


class PerfectEntanglerChi(_LocalInvariantsFunctional):
    """``chi_constructor`` for the optimisation towards an arbitrary perfect entangler, for objectives from
    ``gate_objectives(canonical_basis, 'PE', H)``: F = g3 |G| - g1 with G = g1 + i g2 (:func:`F_PE`,
    :func:`local_invariants`), not linear in the states -- use the second-order update (``sigma=``).
    ``unitarity_weight`` w in [0, 1] adds the loss of population from the logical subspace.  ``.J_T(fw_states_T, ...)``
    is the value, ``.values`` the J of every gate when the co-states were last formed -- by a call of the object or, where
    the optimiser forms them on the device, from the kernel's output."""

    mode = LI_MODE_PE


class LocalInvariantsChi(_LocalInvariantsFunctional):
    """``chi_constructor`` for the optimisation towards ``gate`` (4 x 4, canonical basis) up to single-qubit gates, for
    objectives from ``gate_objectives(canonical_basis, gate, H, local_invariants=True)``:
    F = |G - G_O|^2 + (g3 - g3_O)^2 with (G_O, g3_O) the invariants of ``gate``.  Otherwise as
    :class:`PerfectEntanglerChi`."""

    mode = LI_MODE_LI

    def __init__(self, gate, canonical_basis, unitarity_weight=0.0):
        super().__init__(canonical_basis, unitarity_weight)
        g1, g2, g3 = local_invariants(gate)
        self.target_invariants = (complex(g1, g2), g3)


def make_PE_krotov_chi_constructor(canonical_basis, unitarity_weight=0):
    """:class:`PerfectEntanglerChi` under the name the reference's notebook 07 imports from ``weylchamber``."""
    return PerfectEntanglerChi(canonical_basis, unitarity_weight)


def make_LI_krotov_chi_constructor(gate, canonical_basis, unitarity_weight=0):
    """:class:`LocalInvariantsChi` under its ``weylchamber`` name."""
    return LocalInvariantsChi(gate, canonical_basis, unitarity_weight)
