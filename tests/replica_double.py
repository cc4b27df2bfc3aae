"""Oracle-backed stand-in for a *replica* ``HipKrotovEngine`` (TESTS ONLY): ``OracleEngineDouble`` that understands
``replicas=``.  Every sweep runs replica by replica on a plain ``OracleEngineDouble`` of that replica's operators and
time steps, so a replica's numbers are, bit for bit, those of the double that ``optimize_pulses`` would create for it
alone; the active mask and the in-place output buffers follow ``kh_set_active_replicas`` (include/krotov_hip.h)."""
import numpy as np
import torch

from oracle_engine_double import OracleEngineDouble


class ReplicaEngineDouble(OracleEngineDouble):
    created = []  # (every engine made since the test cleared the list: replicas, kernel)

    def __init__(self, ops, dt, is_super=False, replicas=None, **kw):
        dt = np.asarray(dt, dtype=np.float64)
        self.replicas = int(replicas) if replicas else 0
        if not self.replicas:
            super().__init__(ops, dt, is_super=is_super, **kw)
            ReplicaEngineDouble.created.append(self)
            return
        B = self.replicas
        assert len(ops) % B == 0
        if dt.ndim == 1:
            dt = np.broadcast_to(dt, (B, len(dt)))
        assert dt.shape[0] == B
        self.K, self.L = len(ops), len(ops[0]) - 1
        self.Kr = self.K // B
        self.subs = [OracleEngineDouble(ops[b * self.Kr:(b + 1) * self.Kr], dt[b], is_super=is_super) for b in range(B)]
        self.N, self.nt = self.subs[0].N, self.subs[0].nt
        self.is_super = bool(is_super)
        self.device = torch.device('cpu')
        self.kernel = 'replica16/wave'
        self.mask = [1] * B
        self.sweeps = []  # (name, mask) of every sweep
        ReplicaEngineDouble.created.append(self)

    def set_active_replicas(self, mask=None):
        assert self.replicas
        self.mask = [1] * self.replicas if mask is None else [1 if x else 0 for x in mask]
        assert len(self.mask) == self.replicas

    def _rows(self, b):
        return slice(b * self.Kr, (b + 1) * self.Kr)

    def _buffer(self, t, shape, dtype):
        if t is None:
            return torch.full(shape, float('nan'), dtype=dtype)
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype
        return t

    def forward(self, pulses, init, store=False, out=None):
        if not self.replicas:
            return super().forward(pulses, init, store=store)
        assert not store
        pulses = self.dev(pulses, torch.float64)
        init = self.dev(init, torch.complex128)
        assert tuple(pulses.shape) == (self.replicas, self.L, self.nt - 1)
        psi_T = self._buffer(out, (self.K, self.N), torch.complex128)
        self.sweeps.append(('forward', list(self.mask)))
        for b, sub in enumerate(self.subs):
            if self.mask[b]:
                psi_T[self._rows(b)] = sub.forward(pulses[b], init[self._rows(b)])
        return psi_T

    def backward(self, chi_T, pulses, out=None):
        if not self.replicas:
            return super().backward(chi_T, pulses, out=out)
        chi_T = self.dev(chi_T, torch.complex128)
        pulses = self.dev(pulses, torch.float64)
        store = self._buffer(out, (self.K, self.nt, self.N), torch.complex128)
        self.sweeps.append(('backward', list(self.mask)))
        for b, sub in enumerate(self.subs):
            if self.mask[b]:
                store[self._rows(b)] = sub.backward(chi_T[self._rows(b)], pulses[b])
        return store

    def forward_update(self, chi_store, chi_norms, init, guess, shape, lambdas, out=None):
        if not self.replicas:
            return super().forward_update(chi_store, chi_norms, init, guess, shape, lambdas)
        chi_store = self.dev(chi_store, torch.complex128)
        chi_norms = self.dev(chi_norms, torch.float64)
        init = self.dev(init, torch.complex128)
        guess, shape = self.dev(guess, torch.float64), self.dev(shape, torch.float64)
        lambdas = self.dev(lambdas, torch.float64)
        assert tuple(guess.shape) == tuple(shape.shape) == (self.replicas, self.L, self.nt - 1)
        assert tuple(lambdas.shape) == (self.replicas, self.L)
        out = (None, None, None) if out is None else out
        opt = self._buffer(out[0], (self.replicas, self.L, self.nt - 1), torch.float64)
        psi_T = self._buffer(out[1], (self.K, self.N), torch.complex128)
        g_a = self._buffer(out[2], (self.replicas, self.L), torch.float64)
        self.sweeps.append(('update', list(self.mask)))
        for b, sub in enumerate(self.subs):
            if self.mask[b]:
                rows = self._rows(b)
                opt[b], psi_T[rows], g_a[b] = sub.forward_update(
                    chi_store[rows], chi_norms[rows], init[rows], guess[b], shape[b], lambdas[b])
        return opt, psi_T, g_a

    def tau(self, targets, psi_T):
        if not self.replicas:
            return super().tau(targets, psi_T)
        targets, psi_T = self.dev(targets, torch.complex128), self.dev(psi_T, torch.complex128)
        return torch.cat([sub.tau(targets[self._rows(b)], psi_T[self._rows(b)]) for b, sub in enumerate(self.subs)])

    def chi_boundary(self, targets, psi_T, c, d):
        if not self.replicas:
            return super().chi_boundary(targets, psi_T, c, d)
        parts = [sub.chi_boundary(targets[self._rows(b)], psi_T[self._rows(b)], c[self._rows(b)], d[self._rows(b)])
                 for b, sub in enumerate(self.subs)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
