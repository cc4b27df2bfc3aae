"""``ReplicaEngineDouble`` with the second-order update (TESTS ONLY): ``forward(store=True)`` and
``set_second_order_replicas`` as ``HipKrotovEngine`` has them on a replica engine.  Every sweep still runs replica by
replica on that replica's own ``OracleEngineDouble`` -- the second-order one through its ``set_second_order`` with the
replica's sigma row and its slices of the two trajectory buffers -- so a replica's numbers are, bit for bit, those of
the double ``optimize_pulses(sigma=)`` would create for it alone."""
import numpy as np
import torch

from replica_double import ReplicaEngineDouble


class ReplicaEngineDoubleSO(ReplicaEngineDouble):
    _so_rep = None

    def forward(self, pulses, init, store=False, out=None):
        if not self.replicas or not store:
            return super().forward(pulses, init, store=store, out=out)
        pulses = self.dev(pulses, torch.float64)
        init = self.dev(init, torch.complex128)
        assert tuple(pulses.shape) == (self.replicas, self.L, self.nt - 1)
        out = (None, None) if out is None else out
        psi_T = self._buffer(out[0], (self.K, self.N), torch.complex128)
        states = self._buffer(out[1], (self.K, self.nt, self.N), torch.complex128)
        self.sweeps.append(('forward', list(self.mask)))
        for b, sub in enumerate(self.subs):
            if self.mask[b]:
                psi_T[self._rows(b)], states[self._rows(b)] = sub.forward(pulses[b], init[self._rows(b)], store=True)
        return psi_T, states

    def set_second_order_replicas(self, fw_prev=None, fw_store=None, sigma_vals=None):
        assert self.replicas, "KH_ERR_UNSUPPORTED: not a replica engine"
        if fw_prev is None and fw_store is None and sigma_vals is None:
            self._so_rep = None
            return
        sig = self.dev(sigma_vals, torch.float64)
        if tuple(sig.shape) != (self.replicas, self.nt - 1):
            raise ValueError("expected shape %s, got %s" % ((self.replicas, self.nt - 1), tuple(sig.shape)))
        for buf in (fw_prev, fw_store):
            assert tuple(buf.shape) == (self.K, self.nt, self.N) and buf.dtype == torch.complex128
        assert fw_prev.data_ptr() != fw_store.data_ptr()
        self._so_rep = (fw_prev, fw_store, sig.clone())
        self.so_calls = getattr(self, 'so_calls', 0) + 1

    def forward_update(self, chi_store, chi_norms, init, guess, shape, lambdas, out=None):
        if not self.replicas or self._so_rep is None:
            return super().forward_update(chi_store, chi_norms, init, guess, shape, lambdas, out=out)
        fw_prev, fw_store, sig = self._so_rep
        try:
            for b, sub in enumerate(self.subs):
                # (views: the sub-engine's sweep writes replica b's trajectory in place; an inactive one is not run)
                sub.set_second_order(fw_prev[self._rows(b)], fw_store[self._rows(b)], sig[b].numpy().copy())
            return super().forward_update(chi_store, chi_norms, init, guess, shape, lambdas, out=out)
        finally:
            for sub in self.subs:
                sub.set_second_order()
