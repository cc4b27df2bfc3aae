"""Guarded, minimally aligned caller buffers for the engine (pure torch; works on CPU tensors too).

The parity tests hand the library freshly allocated torch tensors: 512-byte aligned, padded by the caching allocator and
surrounded by whatever else the pool holds.  A write past a documented extent, a read past it whose value meets a
zero-padded state, an access that assumes more alignment than the element type has, or a sweep that changes one of its
inputs passes all of them.  Here every tensor an engine sees lives in ONE allocation (``GuardedArena``):

* it starts at the smallest alignment the memory contract of include/krotov_hip.h grants -- complex128 at an address
  = 16 (mod 32), float64 at 8 (mod 16), int32 at 4 (mod 8);
* it has a guard band on both sides of at least max(4096 B, the bytes of its trailing-two-dimensions plane), so that a
  row or plane index that is off by one still lands in a guard (``guard_bytes``; a condition, asserted for every carved
  tensor by ``check_layout``);
* the guards hold one 8-byte pattern (``GUARD_WORD``) that reads as a quiet NaN in either half of a complex number --
  except those next to an int32 array (CSR ``indptr`` / ``indices``), which hold zero words: an index read from there
  stays an in-arena read (of row / column 0), and the NaN guards of the neighbouring ``data`` array make it visible;
* ``verify`` compares, bytewise and on the device, every guard with its pattern and every tensor that the call was not
  allowed to write with what it held at the last ``snapshot()`` (or at the last verified write).

``GuardedEngine`` places what the engine itself allocates (operators, CSR arrays, ``expect`` operators, the persistent
buffers of the per-interval form, the results of ``tau`` / ``chi_boundary``) in the arena through the two seams of
``HipKrotovEngine`` (``_upload``, ``_empty``); ``GuardedDevice`` carves the tensors of ``test_engine_reuse.Device`` and
verifies after every sweep.  Reads whose value is discarded cannot be seen this way."""
import bisect
import struct

import numpy as np

from krotov_amd.engine import HipKrotovEngine
from test_engine_reuse import Device

GUARD_WORD = 0x7ff8dead7ff8beef  # both 32-bit halves start 0x7ff8: a quiet NaN as a double, whichever half is read first
GUARD_BYTES = struct.pack('<Q', GUARD_WORD)
MIN_GUARD = 4096
ALIGN = {'complex128': 16, 'float64': 8, 'int32': 4}  # the element type's own alignment: address = ALIGN (mod 2 ALIGN)


def _dtype_name(dtype):
    return str(dtype).replace('torch.', '')


def guard_bytes(shape, itemsize):
    """The least guard band of a tensor: max(4096 B, bytes of its trailing-two-dimensions plane)."""
    plane = int(np.prod(tuple(shape)[-2:], dtype=np.int64)) * itemsize if len(shape) else itemsize
    return max(MIN_GUARD, plane)


def _up(x, m):
    return (x + m - 1) // m * m


def arena_bytes(tensors):
    """An arena size that holds ``tensors``, (shape, torch dtype) each, whatever the base address."""
    import torch

    total = 0
    for shape, dtype in tensors:
        itemsize = torch.empty((), dtype=dtype).element_size()
        total += int(np.prod(tuple(shape), dtype=np.int64)) * itemsize + 2 * guard_bytes(shape, itemsize) + 128
    return total


def upload_shapes(ops):
    """(shape, dtype) of every tensor ``HipKrotovEngine`` uploads for the operator lists ``ops``: every distinct object
    once, a sparse one as the CSR triples of itself and of its adjoint."""
    import scipy.sparse as sp
    import torch

    seen, out = set(), []
    for row in ops:
        for op in row or []:
            if op is None or id(op) in seen:
                continue
            seen.add(id(op))
            if sp.issparse(op):
                m = sp.csr_matrix(op)
                m.sum_duplicates()
                out += [((m.shape[0] + 1,), torch.int32), ((m.nnz,), torch.int32), ((m.nnz,), torch.complex128)] * 2
            else:
                out.append((tuple(np.shape(op)), torch.complex128))
    return out


def own_shapes(K, N, L, nt):
    """The persistent buffers of ``forward_update_sharded``."""
    import torch

    c128, f64 = torch.complex128, torch.float64
    return [((K,), f64), ((K, N), c128), ((L, nt - 1), f64), ((L, nt - 1), f64), ((L,), f64), ((L, nt - 1), f64), ((K, N), c128),
            ((L,), f64), ((L,), f64), ((1,), torch.int32)]


def caller_shapes(K, N, L, nt, B=0):
    """The tensors of ``test_engine_reuse.Device`` and the three arrays of a parametrization."""
    import torch
    import types

    stub = types.SimpleNamespace(K=K, N=N, L=L, nt=nt, device=torch.device('cpu'))
    return [(tuple(x.shape), x.dtype) for x in Device(stub, B=B).t.values()] + [((L, nt - 1), torch.float64)] * 3


HEADROOM = 4 << 20  # for what a test carves besides (expectation operators, the inputs of tau and chi_boundary)


def engine_arena_bytes(ops, dt, c_ops=None, replicas=0):
    """The arena of a ``GuardedEngine``: its uploads, its own buffers, the caller's tensors and ``HEADROOM``."""
    K, L, nt = len(ops), len(ops[0]) - 1, np.shape(dt)[-1] + 1
    N = max(HipKrotovEngine._dims_of(ops))
    N = N * N if c_ops is not None else N
    return arena_bytes(upload_shapes(list(ops) + list(c_ops or [])) + own_shapes(K, N, L, nt)
                       + caller_shapes(K, N, L, nt, int(replicas or 0))) + HEADROOM + 16 * N * N * 16


class GuardViolation(AssertionError):
    pass


class GuardedArena:
    """One ``uint8`` allocation of ``nbytes`` on ``device``; ``carve`` hands out contiguous views of it."""

    def __init__(self, device, nbytes):
        import torch

        self.torch = torch
        nbytes = _up(int(nbytes), 8)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        assert self.base % 8 == 0
        self.buf.view(torch.int64).fill_(struct.unpack('<q', GUARD_BYTES)[0])
        self.pattern = self.buf.clone()    # what every guard byte must hold
        self.expected = self.buf.clone()   # what every byte must hold at the next verify
        self.is_guard = torch.ones(nbytes, dtype=torch.bool, device=device)
        self.cursor = 0
        self.entries = {}                  # name -> dict(view, lo, hi, before, after, role, shape, dtype)
        self._starts, self._spans = [], []  # sorted spans (lo, hi, name, side) of every byte handed out so far

    # -- layout --------------------------------------------------------------------------------------------------
    def carve(self, name, shape, dtype, role='input'):
        """A contiguous, zero-filled view of ``shape`` and ``dtype`` (complex128, float64 or int32) at the least
        alignment, between two guard bands.  ``role``: 'input', 'output' (documentation) or 'scratch' -- a buffer the
        engine owns and may write in any call (its guards are checked, its content is not)."""
        torch = self.torch
        assert name not in self.entries, name
        align = ALIGN[_dtype_name(dtype)]
        shape = tuple(int(n) for n in shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        g = _up(guard_bytes(shape, itemsize), 2 * align)
        before = self.cursor
        lo = before + g
        lo += (align - (self.base + lo)) % (2 * align)
        hi = lo + nbytes
        after = _up(hi, 8) + g
        if after > self.buf.numel():
            raise MemoryError("GuardedArena: %s %s does not fit (%d of %d bytes used)" % (name, shape, before, self.buf.numel()))
        if _dtype_name(dtype) == 'int32':  # zero words around index arrays
            for x in (self.buf, self.pattern, self.expected):
                x[before:lo].zero_()
                x[hi:after].zero_()
        view = self.buf[lo:hi].view(dtype).view(shape) if nbytes else torch.empty(shape, dtype=dtype, device=self.buf.device)
        self.is_guard[lo:hi] = False
        self.buf[lo:hi].zero_()
        self.expected[lo:hi].zero_()
        self.cursor = after
        self.entries[name] = dict(view=view, lo=lo, hi=hi, before=before, after=after, role=role, shape=shape, dtype=dtype)
        for span in ((before, lo, name, 'before'), (lo, hi, name, 'inside'), (hi, after, name, 'after')):
            self._starts.append(span[0])
            self._spans.append(span)
        return view

    def check_layout(self):
        """The conditions of the layout, for every carved tensor (host code): alignment residues, guard sizes, order."""
        end = 0
        for name, e in self.entries.items():
            align = ALIGN[_dtype_name(e['dtype'])]
            itemsize = self.torch.empty((), dtype=e['dtype']).element_size()
            assert e['before'] == end and e['before'] < e['lo'] <= e['hi'] < e['after'] <= self.buf.numel(), name
            assert (self.base + e['lo']) % (2 * align) == align, (name, 'alignment')
            if e['hi'] > e['lo']:
                assert e['view'].data_ptr() == self.base + e['lo'] and e['view'].is_contiguous(), name
            need = guard_bytes(e['shape'], itemsize)
            assert e['lo'] - e['before'] >= need and e['after'] - e['hi'] >= need, (name, 'guard', need)
            end = e['after']
        return True

    # -- content -------------------------------------------------------------------------------------------------
    def _span_of(self, x):
        """Byte range of a contiguous (sub-)view of a carved tensor, or of the tensor of that name."""
        if isinstance(x, str):
            e = self.entries[x]
            return e['lo'], e['hi']
        assert x.is_contiguous()
        lo = x.data_ptr() - self.base
        hi = lo + x.numel() * x.element_size()
        assert 0 <= lo <= hi <= self.buf.numel(), "not a view of the arena"
        return lo, hi

    def accept(self, *written):
        """What the named tensors (or contiguous sub-views of carved tensors) hold now is what they are expected to hold."""
        for x in written:
            if not isinstance(x, str) and x.numel() == 0:
                continue
            lo, hi = self._span_of(x)
            assert not self.is_guard[lo:hi].any(), "a guard is never accepted"
            self.expected[lo:hi].copy_(self.buf[lo:hi])

    def snapshot(self):
        """Every tensor's present content is what ``verify`` compares with from here on (the guards stay the pattern)."""
        self.expected.copy_(self.torch.where(self.is_guard, self.pattern, self.buf))

    def _where(self, offset):
        i = bisect.bisect_right(self._starts, offset) - 1
        lo, hi, name, side = self._spans[i] if i >= 0 else (0, 0, None, None)
        if name is None or offset >= hi:
            return 'unused arena memory', 'behind', offset - self.cursor
        return name, side, offset - lo

    def verify(self, step, outputs=()):
        """Every guard byte holds its pattern and every tensor outside ``outputs`` (names or contiguous sub-views; the
        'scratch' tensors count as outputs of every call) is bytewise what it was at the last ``snapshot()`` or accepted
        write.  Returns nothing; raises ``GuardViolation`` naming tensor, side, first changed byte offset and step."""
        torch = self.torch
        self.accept(*outputs, *(n for n, e in self.entries.items() if e['role'] == 'scratch'))
        if torch.equal(self.buf, self.expected):
            return None
        first = int((self.buf != self.expected).nonzero()[0])
        changed = int((self.buf != self.expected).sum())
        name, side, off = self._where(first)
        what = {'before': 'the guard before %s' % name, 'after': 'the guard after %s' % name,
                'inside': '%s, which is no output of this call,' % name, 'behind': name}[side]
        got, want = bytes(self.buf[first:first + 8].cpu().tolist()), bytes(self.expected[first:first + 8].cpu().tolist())
        raise GuardViolation("%s: %s changed: first at byte offset %d of it (%d bytes in the arena differ; holds %s, expected %s)"
                             % (step, what, off, changed, got.hex(), want.hex()))


# ---------------------------------------------------------------------------------------------------------------------
# the engine and the tensors of test_engine_reuse on an arena
# ---------------------------------------------------------------------------------------------------------------------
class GuardedEngine(HipKrotovEngine):
    """``HipKrotovEngine`` whose own tensors (``_upload``, ``_empty``) live in ``self.arena``; verified right after
    creation (which reads the operators: adjoint staging, the self-adjointness and defect kernels) and after every call
    that changes the engine's form -- a refusal included."""

    def __init__(self, ops, dt, *args, **kwargs):
        import torch

        device = kwargs.get('device')
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.arena = GuardedArena(device, engine_arena_bytes(ops, dt, kwargs.get('c_ops'), kwargs.get('replicas')))
        self._carved = 0
        self.active = None
        super().__init__(ops, dt, *args, **kwargs)
        torch.cuda.synchronize(self.device)
        self.arena.verify('engine creation')

    def _name(self, kind):
        self._carved += 1
        return '%s%d' % (kind, self._carved)

    def _upload(self, host_array):
        import torch

        host = torch.from_numpy(host_array)
        t = self.arena.carve(self._name('upload'), host.shape, host.dtype, 'input')
        t.copy_(host)
        self.arena.accept(t)
        return t

    def _empty(self, shape, dtype):
        return self.arena.carve(self._name('engine'), shape, dtype, 'scratch')

    def _verified(self, what, call):
        import torch

        try:
            return call()
        finally:
            torch.cuda.synchronize(self.device)
            self.arena.verify(what)

    def set_active_replicas(self, mask=None):
        out = self._verified('set_active_replicas', lambda: super(GuardedEngine, self).set_active_replicas(mask))
        self.active = None if mask is None else [bool(x) for x in mask]
        return out

    def set_second_order(self, *args, **kwargs):
        return self._verified('set_second_order', lambda: super(GuardedEngine, self).set_second_order(*args, **kwargs))

    def set_second_order_replicas(self, *args, **kwargs):
        return self._verified('set_second_order_replicas',
                              lambda: super(GuardedEngine, self).set_second_order_replicas(*args, **kwargs))

    def set_parametrization(self, *args, **kwargs):
        return self._verified('set_parametrization', lambda: super(GuardedEngine, self).set_parametrization(*args, **kwargs))

    def set_update_workgroups(self, *args, **kwargs):
        return self._verified('set_update_workgroups', lambda: super(GuardedEngine, self).set_update_workgroups(*args, **kwargs))

    def set_row_split(self, *args, **kwargs):
        return self._verified('set_row_split', lambda: super(GuardedEngine, self).set_row_split(*args, **kwargs))


class GuardedDevice(Device):
    """``test_engine_reuse.Device`` with every tensor carved from the engine's arena: ``snapshot()`` after ``put`` and
    ``put_second_order``, ``verify`` after every sweep with that sweep's outputs (``store`` only while second order is
    on; on a replica engine only the active replicas' slices).  ``extra``: further tensors (name -> (shape, dtype)), e.g.
    the ``u_guess`` / ``dfdu`` / ``u_opt`` of a parametrization; ``update_outputs``: names the update sweeps write
    besides their own."""
    OUTPUTS = ('opt', 'psi_T', 'g_a', 'fw_T', 'states', 'chi', 'store')

    def __init__(self, eng, B=0, extra=None):
        super().__init__(eng, B)
        self.arena = eng.arena
        self.B = B
        self.t = {name: self.arena.carve(name, x.shape, x.dtype, 'output' if name in self.OUTPUTS else 'input')
                  for name, x in self.t.items()}
        for name, (shape, dtype) in (extra or {}).items():
            self.t[name] = self.arena.carve(name, shape, dtype, 'input')
        self.ptrs = self._ptrs()
        self.update_outputs = ()
        self.calls = 0
        self.arena.check_layout()
        self.arena.snapshot()

    def put(self, s):
        super().put(s)
        self.arena.snapshot()

    def put_second_order(self, prev, sigma_vals):
        super().put_second_order(prev, sigma_vals)
        self.arena.snapshot()

    def put_extra(self, **host):
        for name, x in host.items():
            self._copy(name, x)
        self.arena.snapshot()

    def _written(self, names):
        """The slices of the tensors ``names`` that the engine may write: all of them, or the active replicas' rows."""
        active = getattr(self.eng, 'active', None)
        if not self.B or active is None:
            return [self.t[n] for n in names]
        out = []
        for n in names:
            x = self.t[n]
            per = x.shape[0] // self.B  # (rows per replica: K_r of a state tensor, 1 of a pulse-like one)
            out += [x[b * per:(b + 1) * per] for b in range(self.B) if active[b]]
        return out

    def _guarded(self, what, names, call):
        self.calls += 1
        step = 'call %d (%s)' % (self.calls, what)
        try:
            return call()
        finally:
            self.torch.cuda.synchronize(self.eng.device)
            self.arena.verify(step, self._written(names))

    def forward(self, fill=True):
        return self._guarded('forward', ('fw_T', 'states'), lambda: super(GuardedDevice, self).forward(fill))

    def backward(self, fill=True):
        return self._guarded('backward', ('chi',), lambda: super(GuardedDevice, self).backward(fill))

    def _update_names(self):
        return ('opt', 'psi_T', 'g_a') + (('store',) if self.second_order else ()) + tuple(self.update_outputs)

    def update(self, fill=True):
        return self._guarded('update', self._update_names(), lambda: super(GuardedDevice, self).update(fill))

    def sharded(self, graph_chunk, chi=None):
        # (its results come back in tensors of the engine's own: of the caller's, only the second-order store and a
        # parametrization's u_opt are written)
        return self._guarded('update per interval', self._update_names()[3:],
                             lambda: super(GuardedDevice, self).sharded(graph_chunk, chi))
