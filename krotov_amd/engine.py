"""Python handle on the HIP Krotov engine (thin layer over the C ABI).

PyTorch-ROCm is used for device memory and streams only: every array the
engine touches is a ``torch`` tensor in HBM whose ``data_ptr()`` is handed to
``libkrotov_hip.so``; all arithmetic happens in the HIP kernels.

The three sweeps map onto the reference's three ``parallel_map`` dispatches
(reference src/krotov/optimize.py:302-313, 413-425, 444-501).
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .sharding import run_update_loop

__all__ = ['HipKrotovEngine', 'LAST_ENGINE', 'auto_row_split']

_last_engine = None


def _is_sparse(op):
    return op is not None and hasattr(op, 'tocsr') and hasattr(op, 'nnz')


def LAST_ENGINE():
    """The most recently created engine (for benchmarks and tests that need the per-launch timings or the
    kernel family of an engine built inside optimize_pulses).  Held strongly until the next engine is created:
    nothing in a :class:`~krotov_amd.result.Result` is guaranteed to keep it alive."""
    return _last_engine


def auto_row_split(num_cus, K, N):
    """``row_split='auto'``: the largest power of two <= min(num_cus // K, chunks // 8, 64) with chunks = ceil(N / 64), and
    1 where N <= 4096.  The ``chunks // 8`` term (at least 512 rows per part) and the N floor are PLACEHOLDERS: they are
    to be replaced by what ``scripts/perf_ellsplit.py`` measures (``profiles/ellsplit.txt``), which has
    not been recorded yet."""
    if N <= 4096 or K < 1:
        return 1
    cap = min(num_cus // K, ((N + 63) // 64) // 8, 64)
    S = 1
    while 2 * S <= cap:
        S *= 2
    return S


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError(
            "krotov_amd: no HIP device visible (torch.cuda.is_available() is False); "
            "the engine has no CPU fallback"
        )


class HipKrotovEngine:
    """K objectives x N-dimensional states x L controls on one GPU.

    Args:
        ops: list (K) of lists ``[H0, H_1, ..., H_L]`` of (N, N) complex arrays
            (NumPy or torch); ``None`` where a control does not occur in an
            objective.  Entries that are the *same object* are uploaded once
            and shared on the device.
        dt: (nt-1,) interval lengths.
        is_super: operators are Liouvillians acting on column-stacked vec(rho); a bool, or one bool per objective.

    Objectives may differ in dimension (every operator of objective k is N_k x N_k) and in kind (``is_super`` per
    objective).  Then the engine is a *mixed* one (``kh_engine_create_mixed``, kernel family ``"generic/mixed"``):
    ``dims`` lists N_k, ``N`` is the stride max N_k of every (K, N) / (K, nt, N) array the sweeps take and return,
    objective k uses the first N_k entries of its rows and the engine writes zeros behind them (see
    :func:`krotov_amd.mixed.layout`).  Dense operators only.  When every objective has the same dimension and kind the
    engine is the uniform one, as before.
        op_norms: optional (K, 1+L) spectral-norm bounds (true upper bounds; a loose one only costs series terms);
            computed on the host with ``numpy.linalg.norm(., 2)`` per distinct operator when omitted.  ``'frobenius'``:
            the library gets no bounds (a NULL ``op_norms``) and computes Frobenius norms itself (on the device; Lindblad
            form: on the host); ``self.op_norms`` then holds the host's ``numpy.linalg.norm(., 'fro')`` of every operator
            (0 for an absent one).  Sparse operators: ``kh_problem_csr.op_norms`` is required, so ``'frobenius'`` raises
            ``ValueError`` before anything touches the GPU.
        tol: truncation tolerance of the series per sub-step (``<= 0`` or NaN: 2^-53).
        device: torch device (default: current CUDA/HIP device).
        c_ops: Lindblad form (``kh_engine_create_lindblad``, kernel family ``"lindblad/matrix"``): list (K) of lists of
            (d, d) Lindblad operators (``None`` / shorter lists where an objective has fewer; ``[]`` for none).  ``ops``
            then holds d x d Hamiltonian parts, the states are density matrices column-stacked to N = d*d as for
            ``is_super`` (which is implied), and every sweep equals -- to rounding -- the one of an ``is_super`` engine on
            ``liouvillian(H, c_ops)``, whose d^2 x d^2 operators are never built.  d <= 32, at most 4 Lindblad operators
            and 4 controls (``KrotovHipError`` with ``KH_ERR_UNSUPPORTED`` beyond); first-order update on one GPU only.
            ``op_norms``: (K, 1+L+n_c) bounds for (H0, H_l, C_j).
        row_split: sparse engines in the form with global vectors (``"ellglobal/csr"``) only: the rows of every
            objective on this many workgroups (``"ellsplit/csr"``, :meth:`set_row_split`) -- an int, ``'auto'``
            (:func:`auto_row_split`) or ``None``: one workgroup per objective, as before.
        replicas: B > 0 makes a *replica engine* (``kh_engine_create_replicas``, kernel family ``"replica16/wave"``): the K
            objectives are B independent problems of K_r = K / B objectives each (objectives b K_r ... (b + 1) K_r - 1
            belong to replica b), every sweep is one launch over the batch.  ``dt`` is then (nt-1,) for all replicas or
            (B, nt-1); the sweeps take pulses, shapes and return optimized pulses as (B, L, nt-1), ``lambdas`` and
            ``g_a`` as (B, L); states keep their (K, ...) shapes.  Dense operators, one kind, N <= 16, K_r <= 8,
            1 <= L <= 4, first order (``KrotovHipError`` with ``KH_ERR_UNSUPPORTED`` beyond).
    """

    def __init__(self, ops, dt, is_super=False, op_norms=None, device=None, tol=0.0, theta_max=0.0, c_ops=None,
                 row_split=None, replicas=None):
        frobenius = isinstance(op_norms, str)
        if frobenius and op_norms != 'frobenius':
            raise ValueError("op_norms: an array of bounds, None or 'frobenius'")
        if frobenius and any(_is_sparse(op) for row in ops for op in row):
            raise ValueError("op_norms='frobenius': sparse operators need norm bounds (kh_problem_csr.op_norms is required)")
        _require_gpu()
        self._lib = _lib.load()
        self.replicas = int(replicas) if replicas else 0
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.K = len(ops)
        self.L = len(ops[0]) - 1
        kinds = [bool(x) for x in is_super] if isinstance(is_super, (list, tuple, np.ndarray)) else [bool(is_super)] * self.K
        if len(kinds) != self.K:
            raise ValueError("is_super: %d entries for %d objectives" % (len(kinds), self.K))
        dt = np.ascontiguousarray(np.asarray(dt, dtype=np.float64))
        if self.replicas:
            if self.K % self.replicas != 0:
                raise ValueError("%d objectives are not %d replicas of equal size" % (self.K, self.replicas))
            if dt.ndim == 1:
                dt = np.ascontiguousarray(np.broadcast_to(dt, (self.replicas, len(dt))))
            if dt.ndim != 2 or dt.shape[0] != self.replicas:
                raise ValueError("dt must be (nt-1,) or (replicas, nt-1)")
        elif dt.ndim != 1:
            raise ValueError("dt must be (nt-1,)")
        self.nt = dt.shape[-1] + 1
        self._dt = dt
        self._handle = ctypes.c_void_p()
        self._op_tensors = {}
        # the tensors the library points at while a variant of the update sweep is set (set_second_order*,
        # set_parametrization, set_nonlinear), and forward_update_sharded's persistent buffers
        self._so = self._par = self._nl = self._sh = None
        for k, row in enumerate(ops):
            if len(row) != 1 + self.L:
                raise ValueError("objective %d has %d operators, expected %d" % (k, len(row), 1 + self.L))
        dims = self._dims_of(ops)
        self.lindblad = c_ops is not None
        if self.lindblad:
            if len(set(dims)) > 1 or len(c_ops) != self.K:
                raise ValueError("Lindblad form: one dimension d for all objectives and one c_ops list per objective")
            if any(_is_sparse(op) for row in list(ops) + [list(r or []) for r in c_ops] for op in row):
                raise ValueError("Lindblad form: dense d x d operators only")
            self.d = dims[0]
            dims = [self.d * self.d] * self.K
            kinds = [True] * self.K
        self.mixed = len(set(dims)) > 1 or len(set(kinds)) > 1
        if self.replicas and (self.lindblad or self.mixed or row_split is not None or
                              any(_is_sparse(op) for row in ops for op in row)):
            raise _lib.KrotovHipError("replica engines take dense operators of one dimension and one kind (no c_ops, no "
                                      "sparse operators, no row split)", _lib.KH_ERR_UNSUPPORTED)
        self.dims = dims
        self.kinds = kinds
        self.N = max(dims)
        self.is_super = kinds if self.mixed else kinds[0]
        sparse = any(_is_sparse(op) for row in ops for op in row)
        if self.mixed and sparse:
            raise ValueError("objectives of different dimension or kind need dense operators: "
                             "sparse (CSR) operators take one dimension and one kind for all objectives")
        with torch.cuda.device(self.device):
            if self.lindblad:
                norms = self._create_lindblad(ops, c_ops, dt, op_norms, tol, theta_max)
            elif sparse:
                norms = self._create_sparse(ops, dt, op_norms, tol, theta_max)
            else:
                norms = self._create_dense(ops, dt, op_norms, tol, theta_max)
        self.op_norms = norms.reshape(self.K, -1)
        self.kernel = self._lib.kh_engine_kernel(self._handle).decode()
        self.row_split = 1
        if self.kernel == 'ellsplit/csr':  # (KH_KERNEL=ellsplit: the library chose KH_ELL_SPLIT or 'auto')
            self.row_split = int(os.environ.get('KH_ELL_SPLIT', '0')) or auto_row_split(self._num_cus(), self.K, self.N)
        if row_split is not None:
            try:
                self.set_row_split(row_split)
            except Exception:
                self.close()
                raise
        # optional per-launch timing with HIP events on the launch stream
        self.profile = os.environ.get('KH_PROFILE', '0') == '1'
        self._events = {'forward': [], 'backward': [], 'update': []}
        global _last_engine
        _last_engine = self

    @staticmethod
    def _dims_of(ops):
        """N_k of every objective: the size of its operators, which must all agree."""
        dims = []
        for k, row in enumerate(ops):
            n = None
            for op in row:
                if op is None:
                    continue
                shape = tuple(op.shape) if hasattr(op, 'shape') else np.shape(op)
                if len(shape) != 2 or shape[0] != shape[1]:
                    raise ValueError("operators must be square matrices")
                if n is None:
                    n = shape[0]
                elif shape[0] != n:
                    raise ValueError("objective %d: all its operators must have the same dimension" % k)
            if n is None:
                raise ValueError("objective %d has no operators" % k)
            dims.append(int(n))
        return dims

    def _check_dim(self, shape):
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("operators must be square matrices")

    def _norms(self, norms, op_norms):
        if op_norms is not None:
            norms = np.ascontiguousarray(np.asarray(op_norms, dtype=np.float64).reshape(-1))
            if norms.size != self.K * (1 + self.L):
                raise ValueError("op_norms must have K*(1+L) entries")
        return norms

    def _create_dense(self, ops, dt, op_norms, tol, theta_max):
        """Dense row-major operators; each distinct object is uploaded once."""
        frobenius = isinstance(op_norms, str)
        n_ops = self.K * (1 + self.L)
        ptrs = (ctypes.c_void_p * n_ops)()
        norms = np.zeros(n_ops, dtype=np.float64)
        norms_cache = {}
        for k, row in enumerate(ops):
            for j, op in enumerate(row):
                idx = k * (1 + self.L) + j
                if op is None:
                    ptrs[idx] = None
                    continue
                key = id(op)
                if key not in self._op_tensors:
                    host = op.detach().cpu().numpy() if isinstance(op, torch.Tensor) else np.asarray(op)
                    host = np.ascontiguousarray(host, dtype=np.complex128)
                    self._check_dim(host.shape)
                    t = self._upload(host)
                    self._op_tensors[key] = (t, op)  # keep `op` alive: id() stays unique
                    norms_cache[key] = float(np.linalg.norm(host, 'fro' if frobenius else 2)) if host.size else 0.0
                ptrs[idx] = self._op_tensors[key][0].data_ptr()
                norms[idx] = norms_cache[key]
        if not frobenius:
            norms = self._norms(norms, op_norms)
        pr = _lib.kh_problem()
        pr.K, pr.N, pr.L, pr.nt = self.K, self.N, self.L, self.nt
        pr.is_super = 1 if (not self.mixed and self.is_super) else 0
        pr.dt = dt.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        pr.ops = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        pr.op_norms = None if frobenius else norms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        pr.tol = float(tol)
        pr.theta_max = float(theta_max)
        if self.replicas:
            pr.dt = None  # (every replica's own steps: dt is (B, nt-1))
            _lib.check(self._lib.kh_engine_create_replicas(
                ctypes.byref(pr), self.replicas, dt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(self._handle)))
        elif self.mixed:
            dims = (ctypes.c_int32 * self.K)(*self.dims)
            kinds = (ctypes.c_int32 * self.K)(*[1 if x else 0 for x in self.kinds])
            _lib.check(self._lib.kh_engine_create_mixed(ctypes.byref(pr), dims, kinds, ctypes.byref(self._handle)))
        else:
            _lib.check(self._lib.kh_engine_create(ctypes.byref(pr), ctypes.byref(self._handle)))
        return norms

    def _create_lindblad(self, ops, c_ops, dt, op_norms, tol, theta_max):
        """d x d Hamiltonian parts and Lindblad operators, each distinct object uploaded once.  Norm bounds: the 2-norm;
        for a Hermitian Hamiltonian part half the spread of its spectrum (the commutator does not see H -> H - c)."""
        rows = [list(r) if r is not None else [] for r in c_ops]
        self.n_c = n_c = max([len(r) for r in rows] + [0])
        stride = 1 + self.L + n_c
        n_ops, n_cops = self.K * (1 + self.L), self.K * n_c
        ptrs = (ctypes.c_void_p * n_ops)()
        cptrs = (ctypes.c_void_p * max(n_cops, 1))()
        norms = np.zeros(self.K * stride, dtype=np.float64)
        norms_cache = {}
        frobenius = isinstance(op_norms, str)

        def upload(op, hamiltonian):
            key = id(op)
            if key not in self._op_tensors:
                host = op.detach().cpu().numpy() if isinstance(op, torch.Tensor) else np.asarray(op)
                host = np.ascontiguousarray(host, dtype=np.complex128)
                if host.shape != (self.d, self.d):
                    raise ValueError("Lindblad form: every operator must be %d x %d" % (self.d, self.d))
                self._op_tensors[key] = (self._upload(host), op)
                if frobenius:
                    norms_cache[key] = float(np.linalg.norm(host, 'fro'))
                elif hamiltonian and np.array_equal(host, host.conj().T):
                    ev = np.linalg.eigvalsh(host)
                    norms_cache[key] = 0.5 * float(ev[-1] - ev[0])
                else:
                    norms_cache[key] = float(np.linalg.norm(host, 2))
            return self._op_tensors[key][0].data_ptr(), norms_cache[key]

        for k in range(self.K):
            for j, op in enumerate(ops[k]):
                if op is not None:
                    ptrs[k * (1 + self.L) + j], norms[k * stride + j] = upload(op, True)
            for j, op in enumerate(rows[k]):
                if op is not None:
                    cptrs[k * n_c + j], norms[k * stride + 1 + self.L + j] = upload(op, False)
        if op_norms is not None and not frobenius:
            norms = np.ascontiguousarray(np.asarray(op_norms, dtype=np.float64).reshape(-1))
            if norms.size != self.K * stride:
                raise ValueError("op_norms must have K*(1+L+n_c) entries")
        pr = _lib.kh_problem_lindblad()
        pr.K, pr.d, pr.L, pr.nt, pr.n_c = self.K, self.d, self.L, self.nt, n_c
        pr.dt = dt.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        pr.ops = ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
        pr.c_ops = ctypes.cast(cptrs, ctypes.POINTER(ctypes.c_void_p))
        pr.op_norms = None if frobenius else norms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        pr.tol = float(tol)
        pr.theta_max = float(theta_max)
        _lib.check(self._lib.kh_engine_create_lindblad(ctypes.byref(pr), ctypes.byref(self._handle)))
        return norms

    def _create_sparse(self, ops, dt, op_norms, tol, theta_max):
        """``scipy.sparse`` operators (any mix with dense ones, which are converted):
        CSR arrays of every distinct operator and of its conjugate transpose go to
        the device once; spectral norms are bounded by sqrt(||A||_1 ||A||_inf)."""
        import scipy.sparse as sp

        n_ops = self.K * (1 + self.L)
        fw = (_lib.kh_csr * n_ops)()
        bw = (_lib.kh_csr * n_ops)()
        norms = np.zeros(n_ops, dtype=np.float64)
        cache = {}

        def upload(mat):
            mat = sp.csr_matrix(mat, dtype=np.complex128)
            mat.sum_duplicates()
            arrays = (
                self._upload(np.ascontiguousarray(mat.indptr, dtype=np.int32)),
                self._upload(np.ascontiguousarray(mat.indices, dtype=np.int32)),
                self._upload(np.ascontiguousarray(mat.data, dtype=np.complex128)),
            )
            return arrays, int(mat.nnz)

        def fill(slot, arrays, nnz):
            slot.nnz = nnz
            slot.indptr, slot.indices, slot.data = (a.data_ptr() for a in arrays)

        for k, row in enumerate(ops):
            for j, op in enumerate(row):
                idx = k * (1 + self.L) + j
                if op is None:
                    continue
                key = id(op)
                if key not in cache:
                    mat = sp.csr_matrix(op.detach().cpu().numpy() if isinstance(op, torch.Tensor) else op)
                    self._check_dim(mat.shape)
                    a_fw, nnz = upload(mat)
                    a_bw, _ = upload(mat.conj().T)
                    bound = float(np.sqrt(abs(mat).sum(axis=0).max() * abs(mat).sum(axis=1).max())) if nnz else 0.0
                    cache[key] = (a_fw, a_bw, nnz, bound)
                    self._op_tensors[key] = ((a_fw, a_bw), op)
                a_fw, a_bw, nnz, bound = cache[key]
                fill(fw[idx], a_fw, nnz)
                fill(bw[idx], a_bw, nnz)
                norms[idx] = bound
        norms = self._norms(norms, op_norms)
        pr = _lib.kh_problem_csr()
        pr.K, pr.N, pr.L, pr.nt = self.K, self.N, self.L, self.nt
        pr.is_super = 1 if self.is_super else 0  # (never mixed: refused above)
        pr.dt = dt.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        pr.ops = fw
        pr.ops_adj = bw
        pr.op_norms = norms.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        pr.tol = float(tol)
        pr.theta_max = float(theta_max)
        _lib.check(self._lib.kh_engine_create_csr(ctypes.byref(pr), ctypes.byref(self._handle)))
        return norms

    def _timed(self, name):
        """Context manager recording HIP events around a launch when profiling."""
        eng = self

        class _T:
            def __enter__(self_t):
                if eng.profile:
                    self_t.a = torch.cuda.Event(enable_timing=True)
                    self_t.b = torch.cuda.Event(enable_timing=True)
                    self_t.a.record(torch.cuda.current_stream(eng.device))

            def __exit__(self_t, *exc):
                if eng.profile:
                    self_t.b.record(torch.cuda.current_stream(eng.device))
                    eng._events[name].append((self_t.a, self_t.b))
                return False

        return _T()

    def kernel_times_ms(self, reset=True):
        """Per-launch durations (ms) measured by HIP events since the last reset."""
        torch.cuda.synchronize(self.device)
        out = {k: [a.elapsed_time(b) for a, b in v] for k, v in self._events.items()}
        if reset:
            self._events = {k: [] for k in self._events}
        return out

    # -- helpers -----------------------------------------------------------
    def close(self):
        if getattr(self, '_handle', None) is not None and self._handle.value:
            self._lib.kh_engine_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # The two places where the engine itself makes device tensors that a kernel gets the address of (a subclass may
    # place them elsewhere: tests/guarded.py).  Memory contract: include/krotov_hip.h.
    def _upload(self, host_array):
        """A contiguous host array (operator, CSR array) as a device tensor."""
        return torch.from_numpy(host_array).to(self.device)

    def _empty(self, shape, dtype):
        """An uninitialised device tensor the engine keeps or returns."""
        return torch.empty(shape, dtype=dtype, device=self.device)

    def dev(self, x, dtype):
        """Contiguous tensor of ``dtype`` on the engine's device."""
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(np.asarray(x)), dtype=dtype).to(self.device).contiguous()

    def _c(self, x, shape):
        t = self.dev(x, torch.complex128)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (shape, tuple(t.shape)))
        return t

    def _f(self, x, shape):
        t = self.dev(x, torch.float64)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (shape, tuple(t.shape)))
        return t

    # -- sweeps ------------------------------------------------------------
    def _pulse_shape(self):
        """(L, nt-1), or (B, L, nt-1) on a replica engine."""
        return (self.replicas, self.L, self.nt - 1) if self.replicas else (self.L, self.nt - 1)

    def _out(self, t, shape, dtype, name='output buffer'):
        """``t`` as an output buffer (written in place: a contiguous tensor of this shape, dtype and device), or a new one."""
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous()
                or t.device != self.device):
            raise ValueError("%s must be a contiguous %s %s tensor on %s" % (name, tuple(shape), dtype, self.device))
        return t

    def set_active_replicas(self, mask=None):
        """Replica engines: the following sweeps work on the replicas whose ``mask`` entry (B of them) is non-zero, or on
        all of them (``None``).  An inactive replica's slices of every output buffer keep what they held
        (``kh_set_active_replicas``); ``KrotovHipError`` (``KH_ERR_UNSUPPORTED``) on any other engine."""
        if mask is None:
            _lib.check(self._lib.kh_set_active_replicas(self._handle, None))
            return
        mask = [1 if x else 0 for x in np.asarray(mask).reshape(-1)]
        if self.replicas and len(mask) != self.replicas:
            raise ValueError("mask: %d entries for %d replicas" % (len(mask), self.replicas))
        _lib.check(self._lib.kh_set_active_replicas(self._handle, (ctypes.c_int32 * len(mask))(*mask)))

    def replica_occupancy(self):
        """Workgroups of the replica update kernel one compute unit holds at once (``kh_replica_occupancy``)."""
        n = ctypes.c_int32(0)
        _lib.check(self._lib.kh_replica_occupancy(self._handle, ctypes.byref(n)))
        return int(n.value)

    def forward(self, pulses, init, store=False, out=None):
        """Propagate ``init`` (K, N) over the grid under ``pulses`` (L, nt-1) -- replica engines: (B, L, nt-1).

        Returns ``psi_T`` or ``(psi_T, states)`` with states (K, nt, N).  ``out``: ``psi_T`` (``store``: the pair) to
        write into instead of new tensors.
        """
        pulses = self._f(pulses, self._pulse_shape())
        init = self._c(init, (self.K, self.N))
        out_T, out_states = (out if store else (out, None)) if out is not None else (None, None)
        psi_T = self._out(out_T, (self.K, self.N), torch.complex128)
        states = self._out(out_states, (self.K, self.nt, self.N), torch.complex128) if store else None
        with self._timed('forward'):
            _lib.check(self._lib.kh_forward_store(
                self._handle, pulses.data_ptr(), init.data_ptr(),
                states.data_ptr() if store else None, psi_T.data_ptr(), self._stream()))
        return (psi_T, states) if store else psi_T

    def backward(self, chi_T, pulses, out=None):
        """Backward sweep storing chi(t_n); returns (K, nt, N).  ``pulses``: (L, nt-1) -- replica engines: (B, L, nt-1)."""
        pulses = self._f(pulses, self._pulse_shape())
        chi_T = self._c(chi_T, (self.K, self.N))
        out = self._out(out, (self.K, self.nt, self.N), torch.complex128)
        with self._timed('backward'):
            _lib.check(self._lib.kh_backward_store(
                self._handle, chi_T.data_ptr(), pulses.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def backward_source(self, chi_T, pulses, src_store, chi_norms=None, out=None):
        """Backward sweep with a source term (``kh_backward_store_source``; state-dependent constraints):
        ``chi[n] = V_n (chi[n+1] + h_n W[n+1]) + h_n W[n]``, ``h_n = dt_n / 2 / chi_norms[k]``, with ``src_store`` the
        (K, nt, N) device tensor W (read-only; it must not be ``out``) and ``chi_norms`` the (K,) norms taken out of
        ``chi_T`` (``None``: 1).  Returns (K, nt, N).  ``KrotovHipError`` (``KH_ERR_UNSUPPORTED``) on replica,
        Lindblad-form and mixed engines."""
        pulses = self._f(pulses, self._pulse_shape())
        chi_T = self._c(chi_T, (self.K, self.N))
        src_store = self._c(src_store, (self.K, self.nt, self.N))
        norms = None if chi_norms is None else self._f(chi_norms, (self.K,))
        out = self._out(out, (self.K, self.nt, self.N), torch.complex128)
        with self._timed('backward'):
            _lib.check(self._lib.kh_backward_store_source(
                self._handle, chi_T.data_ptr(), pulses.data_ptr(), src_store.data_ptr(),
                None if norms is None else norms.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def apply_store(self, ops, factors, in_store, out=None):
        """``out[k][n] = factors[n] * ops[k] @ in_store[k][n]`` for a whole (K, nt, N) stored trajectory
        (``kh_apply_store``).  ``ops``: K operators of the states' dimension -- arrays, tensors or Qobj-like objects, every
        distinct object uploaded once and kept; ``None`` writes exact zeros for that objective.  ``factors``: (nt,) real,
        or ``None``.  ``KrotovHipError`` (``KH_ERR_UNSUPPORTED``) on mixed and Lindblad-form engines."""
        from ._ingest import to_dense

        ops = list(ops)
        if len(ops) != self.K:
            raise ValueError("ops: %d operators for %d objectives" % (len(ops), self.K))
        cache = self.__dict__.setdefault('_apply_ops', {})
        ptrs = np.zeros(self.K, dtype=np.int64)
        for k, op in enumerate(ops):
            if op is None:
                continue
            if id(op) not in cache:
                host = op.detach().cpu().numpy() if isinstance(op, torch.Tensor) else to_dense(op)
                host = np.ascontiguousarray(host, dtype=np.complex128)
                if host.shape != (self.N, self.N):
                    raise ValueError("ops[%d] has shape %s, expected %s" % (k, host.shape, (self.N, self.N)))
                cache[id(op)] = (self._upload(host), op)  # keep `op` alive: id() stays unique
            ptrs[k] = cache[id(op)][0].data_ptr()
        key = ptrs.tobytes()
        if self.__dict__.get('_apply_table_key') != key:  # (the same operators call after call: one table)
            # (as 8-byte words of the upload seam's element types: complex128, float64, int32)
            self._apply_table, self._apply_table_key = self._upload(ptrs.view(np.float64)), key
        in_store = self._c(in_store, (self.K, self.nt, self.N))
        fac = None if factors is None else self._f(factors, (self.nt,))
        out = self._out(out, (self.K, self.nt, self.N), torch.complex128)
        _lib.check(self._lib.kh_apply_store(
            self._handle, self._apply_table.data_ptr(), None if fac is None else fac.data_ptr(), in_store.data_ptr(),
            out.data_ptr(), self._stream()))
        return out

    def set_second_order(self, fw_prev=None, fw_store=None, sigma_vals=None):
        """Switch the following update sweeps to the second-order update
        (``fw_prev``, ``fw_store``: (K, nt, N) device tensors; ``sigma_vals``:
        sigma at the nt-1 interval mid-points), or back to first order (no
        arguments)."""
        self._set_second_order(self._lib.kh_set_second_order, (self.nt - 1,), fw_prev is None, fw_prev, fw_store, sigma_vals)

    def _set_second_order(self, fn, sigma_shape, off, fw_prev, fw_store, sigma_vals):
        """``fn`` (``kh_set_second_order`` or ``kh_set_second_order_replicas``) with the three device tensors, or with
        none (``off``)."""
        if off:
            _lib.check(fn(self._handle, None, None, None))
            self._so = None
            return
        if fw_prev is None or fw_store is None or sigma_vals is None:
            raise ValueError("fw_prev, fw_store and sigma_vals must be given together (or none of them)")
        fw_prev = self._c(fw_prev, (self.K, self.nt, self.N))
        fw_store = self._out(fw_store, (self.K, self.nt, self.N), torch.complex128, name='fw_store')
        sig = self._f(sigma_vals, sigma_shape)
        _lib.check(fn(self._handle, fw_prev.data_ptr(), fw_store.data_ptr(), sig.data_ptr()))
        self._so = (fw_prev, fw_store, sig)  # keep the tensors alive while the engine points at them

    def set_parametrization(self, kind=None, a=None, b=None, u_guess=None, dfdu=None, u_opt=None):
        """Switch the following update sweeps to pulse parametrizations eps_l = f_l(u_l) (``kh_set_parametrization``):
        ``kind``, ``a``, ``b``: (L,) host arrays (``enum kh_par_kind`` and its parameters); ``u_guess``, ``dfdu``:
        (L, nt-1) u under the guess pulses and f'(u_guess); ``u_opt``: (L, nt-1) float64 device tensor the sweep writes
        u_new to (its ``opt`` holds f(u_new)).  No arguments (``kind=None``): off again.  ``KrotovHipError``
        (``KH_ERR_UNSUPPORTED``) on replica, Lindblad-form and sharded engines."""
        if kind is None:
            self._par = None
            _lib.check(self._lib.kh_set_parametrization(self._handle, None, None, None, None, None, None))
            return
        L = self.L
        kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(L)
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(L)
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(L)
        if self.replicas or u_guess is None or dfdu is None or u_opt is None:
            # (the library's own answer, before any shape is looked at: KH_ERR_UNSUPPORTED on a replica engine, whose
            # pulses have another shape; KH_ERR_INVALID for a missing array)
            _lib.check(self._lib.kh_set_parametrization(self._handle, kind.ctypes.data, a.ctypes.data, b.ctypes.data,
                                                        None, None, None))
            return
        u_guess = self._f(u_guess, (L, self.nt - 1))
        dfdu = self._f(dfdu, (L, self.nt - 1))
        u_opt = self._out(u_opt, (L, self.nt - 1), torch.float64, name='u_opt')
        _lib.check(self._lib.kh_set_parametrization(
            self._handle, kind.ctypes.data, a.ctypes.data, b.ctypes.data, u_guess.data_ptr(), dfdu.data_ptr(),
            u_opt.data_ptr()))
        self._par = (u_guess, dfdu, u_opt)  # keep the tensors alive while the engine points at them

    def set_nonlinear(self, term_control=None, term_power=None, dcde=None):
        """Switch the following update sweeps to non-linear controls (``kh_set_nonlinear``): the engine's L operator slots
        are terms ``eps_c^p H_j``.  ``term_control``, ``term_power``: (L,) host arrays, the control (0 .. C-1, C its
        largest entry + 1) and the power (1 .. 4) of every term; ``dcde``: (L, nt-1) ``p eps_guess^(p-1)`` under the
        guess pulses.  While set, :meth:`forward_update` and :meth:`forward_update_sharded` take ``guess``, ``shape``
        and ``lambdas`` with C rows and return ``opt`` and ``g_a`` with C rows; every other sweep keeps taking L rows
        of term coefficients.  No arguments: off again.  ``KrotovHipError``: ``KH_ERR_UNSUPPORTED`` on replica,
        Lindblad-form and sharded engines, ``KH_ERR_INVALID`` for a bad table or next to a parametrization."""
        if term_control is None:
            self._nl = None
            _lib.check(self._lib.kh_set_nonlinear(self._handle, 0, None, None, None))
            return
        L = self.L
        ctrl = np.ascontiguousarray(term_control, dtype=np.int32).reshape(L)
        power = np.ascontiguousarray(term_power, dtype=np.int32).reshape(L)
        C = int(ctrl.max()) + 1 if L else 0
        if self.replicas or dcde is None:  # (the library's own answer, as set_parametrization)
            _lib.check(self._lib.kh_set_nonlinear(self._handle, C, ctrl.ctypes.data, power.ctypes.data, None))
            return
        dcde = self._f(dcde, (L, self.nt - 1))
        _lib.check(self._lib.kh_set_nonlinear(self._handle, C, ctrl.ctypes.data, power.ctypes.data, dcde.data_ptr()))
        self._nl = (C, dcde)  # keep the tensor alive while the engine points at it

    def _update_rows(self):
        """Rows of the update sweeps' pulse-like arrays: the controls of :meth:`set_nonlinear`, else L."""
        return self._nl[0] if self._nl is not None else self.L

    def set_second_order_replicas(self, fw_prev=None, fw_store=None, sigma_vals=None):
        """Replica engines: switch the following update sweeps to the second-order update with one sigma row per
        replica (``fw_prev``, ``fw_store``: (K, nt, N) device tensors; ``sigma_vals``: (B, nt-1), sigma_b at replica
        b's interval mid-points), or back to first order (no arguments).  ``kh_set_second_order_replicas``;
        ``KrotovHipError`` (``KH_ERR_UNSUPPORTED``) on any other engine."""
        fn = self._lib.kh_set_second_order_replicas
        off = fw_prev is None and fw_store is None and sigma_vals is None
        if not off and not self.replicas:  # (the library's own answer, before any shape is looked at)
            _lib.check(fn(self._handle, None, None, None))
        self._set_second_order(fn, (self.replicas, self.nt - 1), off, fw_prev, fw_store, sigma_vals)

    def set_update_workgroups(self, max_workgroups=0):
        """Run the following single-launch update sweeps on at most ``max_workgroups`` workgroups (0: the engine's own
        choice again); returns the grid the next sweep will use (``kh_set_update_workgroups``).  Raises
        ``KrotovHipError`` (``KH_ERR_UNSUPPORTED``) for kernel families without such a form."""
        import ctypes

        chosen = ctypes.c_int32(0)
        _lib.check(self._lib.kh_set_update_workgroups(self._handle, int(max_workgroups), ctypes.byref(chosen)))
        return int(chosen.value)

    def _num_cus(self):
        return torch.cuda.get_device_properties(self.device).multi_processor_count

    def set_row_split(self, workgroups_per_objective):
        """Spread every objective's rows over this many workgroups in both sweeps (``kh_set_row_split``; kernel family
        ``"ellsplit/csr"``), or ``'auto'`` (:func:`auto_row_split`); 1 restores ``"ellglobal/csr"`` exactly.  Only sparse
        engines in the form with global vectors take it: ``KrotovHipError`` (``KH_ERR_UNSUPPORTED``) otherwise.  Returns
        the factor in force."""
        S = workgroups_per_objective
        if S == 'auto':
            S = auto_row_split(self._num_cus(), self.K, self.N)
            if S == 1 and self.kernel not in ('ellglobal/csr', 'ellsplit/csr'):
                return 1
        _lib.check(self._lib.kh_set_row_split(self._handle, int(S)))
        self.row_split = int(S)
        self.kernel = self._lib.kh_engine_kernel(self._handle).decode()
        return self.row_split

    def forward_update(self, chi_store, chi_norms, init, guess, shape, lambdas, out=None):
        """Forward sweep with sequential update; returns ``(opt, psi_T, g_a)``.  Replica engines: ``guess``, ``shape`` and
        ``opt`` are (B, L, nt-1), ``lambdas`` and ``g_a`` (B, L).  ``out``: ``(opt, psi_T, g_a)`` tensors to write into."""
        per_control = (self.replicas, self.L) if self.replicas else (self._update_rows(),)
        pulse_shape = self._pulse_shape() if self.replicas else (self._update_rows(), self.nt - 1)
        chi_store = self._c(chi_store, (self.K, self.nt, self.N))
        chi_norms = self._f(chi_norms, (self.K,))
        init = self._c(init, (self.K, self.N))
        guess = self._f(guess, pulse_shape)
        shape = self._f(shape, pulse_shape)
        lambdas = self._f(lambdas, per_control)
        out = (None, None, None) if out is None else out
        opt = self._out(out[0], pulse_shape, torch.float64)
        psi_T = self._out(out[1], (self.K, self.N), torch.complex128)
        g_a = self._out(out[2], per_control, torch.float64)
        with self._timed('update'):
            _lib.check(self._lib.kh_forward_update(
                self._handle, chi_store.data_ptr(), chi_norms.data_ptr(), init.data_ptr(), guess.data_ptr(),
                shape.data_ptr(), lambdas.data_ptr(), opt.data_ptr(), psi_T.data_ptr(), g_a.data_ptr(),
                self._stream()))
        return opt, psi_T, g_a

    def forward_update_sharded(self, chi_store, chi_norms, init, guess, shape, lambdas, all_reduce,
                               graph_chunk=None):
        """The same sweep cut at the cross-objective sum: after every interval
        ``all_reduce(partial)`` (in place, L doubles on the device) must return
        the sum over all ranks -- ``torch.distributed.all_reduce`` on the
        ``nccl`` (= RCCL over xGMI) backend.

        With ``graph_chunk`` > 0 (default: env ``KH_GRAPH_CHUNK``, 64) a block of
        that many intervals -- all-reduce + ``kh_update_step_dev`` each -- is
        captured once as a HIP graph and replayed, so the host issues one graph
        launch per block instead of three launches per interval.  The interval
        index lives in device memory, which makes every replay identical; replays
        past the last interval are no-ops.  ``graph_chunk=0`` runs the plain loop.
        """
        if graph_chunk is None:
            graph_chunk = int(os.environ.get('KH_GRAPH_CHUNK', '64'))
        nt, K, N = self.nt, self.K, self.N
        L = self._update_rows()  # (non-linear controls: C rows of eps; the interval's sums stay one per term)
        # persistent buffers: stable addresses let the captured graph be reused
        b = self._sh
        if b is None or b['rows'] != L:
            c128, f64 = torch.complex128, torch.float64
            b = self._sh = dict(
                chi_norms=self._empty((K,), f64), init=self._empty((K, N), c128), guess=self._empty((L, nt - 1), f64),
                shape=self._empty((L, nt - 1), f64), lambdas=self._empty((L,), f64), opt=self._empty((L, nt - 1), f64),
                psi_T=self._empty((K, N), c128), g_a=self._empty((L,), f64), partial=self._empty((self.L,), f64).zero_(),
                n_dev=self._empty((1,), torch.int32).zero_(),
                graph=None, graph_key=None, rows=L,
            )
        chi_store = self._c(chi_store, (K, nt, N))
        b['chi_norms'].copy_(self._f(chi_norms, (K,)))
        b['init'].copy_(self._c(init, (K, N)))
        b['guess'].copy_(self._f(guess, (L, nt - 1)))
        b['shape'].copy_(self._f(shape, (L, nt - 1)))
        b['lambdas'].copy_(self._f(lambdas, (L,)))
        chi_norms, init, guess, shape, lambdas = b['chi_norms'], b['init'], b['guess'], b['shape'], b['lambdas']
        opt, psi_T, g_a, partial, n_dev = b['opt'], b['psi_T'], b['g_a'], b['partial'], b['n_dev']
        lib, h, eng = self._lib, self._handle, self

        def step_dev():
            _lib.check(lib.kh_update_step_dev(
                h, n_dev.data_ptr(), partial.data_ptr(), chi_store.data_ptr(), chi_norms.data_ptr(),
                shape.data_ptr(), lambdas.data_ptr(), opt.data_ptr(), g_a.data_ptr(), partial.data_ptr(),
                eng._stream()))

        class _Stepper:
            """kh_update_begin / kh_update_step / kh_update_end of the C ABI."""

            def begin(self_s):
                _lib.check(lib.kh_update_begin(
                    h, chi_store.data_ptr(), chi_norms.data_ptr(), init.data_ptr(), guess.data_ptr(),
                    opt.data_ptr(), g_a.data_ptr(), partial.data_ptr(), eng._stream()))
                return partial

            def step(self_s, n, D):
                _lib.check(lib.kh_update_step(
                    h, n, D.data_ptr(), chi_store.data_ptr(), chi_norms.data_ptr(), shape.data_ptr(),
                    lambdas.data_ptr(), opt.data_ptr(), g_a.data_ptr(), partial.data_ptr(), eng._stream()))
                return partial

            def end(self_s):
                _lib.check(lib.kh_update_end(h, psi_T.data_ptr(), eng._stream()))

        with self._timed('update'):
            done = False
            # (second order: kh_update_step_dev bakes the trajectory / sigma pointers of kh_set_second_order
            # into the captured launches, and those buffers are swapped every iteration -- no replay there)
            # (non-linear controls: the weights' tensor of set_nonlinear is a new one every iteration, too)
            if graph_chunk > 0 and nt - 1 > 2 * graph_chunk and self._so is None and self._nl is None:
                try:
                    stepper = _Stepper()
                    stepper.begin()
                    n_dev.zero_()
                    # first interval eagerly: also warms up the communicator outside the capture
                    all_reduce(partial)
                    step_dev()
                    key = (chi_store.data_ptr(), graph_chunk)
                    if b['graph'] is None or b['graph_key'] != key:
                        torch.cuda.synchronize(self.device)
                        g = torch.cuda.CUDAGraph()
                        # the capture itself runs the block once, but on a scratch copy of
                        # nothing: captured work is only recorded, not executed
                        with torch.cuda.graph(g):
                            for _ in range(graph_chunk):
                                all_reduce(partial)
                                step_dev()
                        b['graph'], b['graph_key'] = g, key
                    replays = (nt - 2 + graph_chunk - 1) // graph_chunk
                    for _ in range(replays):
                        b['graph'].replay()
                    stepper.end()
                    done = True
                except Exception as exc:  # capture unsupported: plain loop below
                    import warnings

                    warnings.warn("krotov_amd: graph capture of the sharded sweep failed (%s); "
                                  "falling back to per-interval launches" % exc)
                    b['graph'] = None
                    torch.cuda.synchronize(self.device)
            if not done:
                run_update_loop(_Stepper(), nt - 1, all_reduce)
        return opt.clone(), psi_T.clone(), g_a.clone()

    def enable_p2p(self, group, rounds=8):
        """Set up the device-side exchange across the ranks of ``group`` (one per
        GPU of a node): allocate this rank's window, trade IPC handles, map the
        peers' windows and run the in-kernel self-test.  Collective.  Returns True
        when EVERY rank passed -- only then does :meth:`forward_update` include the
        cross-GPU stage; otherwise the engine stays on the per-interval RCCL path."""
        import torch.distributed as dist

        world, rank = dist.get_world_size(group), dist.get_rank(group)
        lib, h = self._lib, self._handle

        def all_ok(ok):
            flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
            return bool(flag.item())

        def stage(name, ok):
            """Collective verdict of one set-up stage; on failure every rank remembers which stage failed and -- where
            it was this rank -- the library's own words (``p2p_why``: printed by ``bench.py --gpus N``)."""
            mine_failed = not ok
            if all_ok(ok):
                return True
            self.p2p_why = "peer windows not used: %s failed%s" % (
                name, (" on this rank (%s)" % lib.kh_last_error().decode('utf-8', 'replace')) if mine_failed else " on another rank")
            lib.kh_p2p_disable(h)
            return False

        self.p2p_why = None
        handle = (ctypes.c_ubyte * 64)()
        ok = lib.kh_p2p_create_window(h, world, rank, handle) == 0
        mine = torch.tensor(list(bytes(handle)), dtype=torch.uint8, device=self.device)
        gathered = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine, group=group)
        if not stage('kh_p2p_create_window', ok):
            return False
        blob = b''.join(bytes(g.cpu().numpy().tobytes()) for g in gathered)
        buf = (ctypes.c_ubyte * len(blob)).from_buffer_copy(blob)
        ok = lib.kh_p2p_open_peers(h, buf) == 0
        if not stage('kh_p2p_open_peers (hipIpcOpenMemHandle)', ok):
            return False
        torch.cuda.synchronize(self.device)
        dist.barrier(group=group)  # every window exists and is mapped before anyone writes
        ok = lib.kh_p2p_selftest(h, int(rounds), self._stream()) == 0
        if not stage('kh_p2p_selftest (in-kernel exchange over the windows)', ok):
            return False
        return True

    def disable_p2p(self):
        self._lib.kh_p2p_disable(self._handle)

    def p2p_stats(self):
        """``kh_p2p_stats``: us per interval workgroup 0 waited inside its GPU / across the GPUs in the last sharded
        single-launch update sweep, us per round of the set-up self-test, ranks."""
        buf = (ctypes.c_double * 4)()
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.kh_p2p_stats(self._handle, buf))
        return dict(local_wait_us=buf[0], cross_gpu_wait_us=buf[1], selftest_round_us=buf[2], ranks=int(buf[3]))

    def tau(self, targets, psi_T):
        targets = self._c(targets, (self.K, self.N))
        psi_T = self._c(psi_T, (self.K, self.N))
        out = self._empty((self.K,), torch.complex128)
        _lib.check(self._lib.kh_tau(self._handle, targets.data_ptr(), psi_T.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def expect(self, states, e_ops, out=None):
        """Expectation values of a stored trajectory on the device (``kh_expect``): ``states`` is the ``(K, nt, N)``
        tensor :meth:`forward` returns with ``store=True``; ``e_ops`` a list of ``n_e`` operators applied to every
        objective, or a list of K such lists (``None``: skipped, exact zeros) -- arrays, tensors or Qobj-like objects,
        every distinct object uploaded once.  Hilbert-space engines take N x N operators and give
        ``<psi_k(t_n)|O|psi_k(t_n)>``; Liouville-space ones (``is_super``, Lindblad form) take d x d operators, N = d*d,
        and give ``tr(O rho_k(t_n))``.  Returns a ``(n_e, K, nt)`` complex128 tensor.  A wrong operator shape raises
        ``ValueError`` before any launch; mixed engines raise ``KrotovHipError`` (``KH_ERR_UNSUPPORTED``)."""
        from ._ingest import to_dense

        e_ops = list(e_ops)
        per_objective = len(e_ops) > 0 and all(isinstance(row, (list, tuple)) for row in e_ops)
        rows = [list(row) for row in e_ops] if per_objective else [e_ops] * self.K
        if len(rows) != self.K:
            raise ValueError("e_ops: %d operator lists for %d objectives" % (len(rows), self.K))
        n_e = len(rows[0])
        if n_e < 1 or any(len(row) != n_e for row in rows):
            raise ValueError("e_ops: every objective needs the same number (>= 1) of operators")
        if self.mixed:
            side = None  # (refused by the library below, whatever the shapes)
        else:
            side = int(round(np.sqrt(self.N))) if self.is_super else self.N
            if side * side != self.N and self.is_super:
                raise ValueError("Liouville-space engine with N = %d, which is not a square" % self.N)
        uploaded = {}
        table = (ctypes.c_void_p * (self.K * n_e))()
        for k, row in enumerate(rows):
            for i, op in enumerate(row):
                if op is None:
                    table[k * n_e + i] = None
                    continue
                key = id(op)
                if key not in uploaded:
                    host = op.detach().cpu().numpy() if isinstance(op, torch.Tensor) else to_dense(op)
                    host = np.ascontiguousarray(host, dtype=np.complex128)
                    if side is not None and host.shape != (side, side):
                        raise ValueError("e_ops[%d] of objective %d has shape %s, expected %s" % (
                            i, k, host.shape, (side, side)))
                    uploaded[key] = (self._upload(host), op)  # keep `op` alive: id() stays unique
                table[k * n_e + i] = uploaded[key][0].data_ptr()
        if tuple(states.shape) != (self.K, self.nt, self.N) or states.dtype != torch.complex128 \
                or not states.is_contiguous() or states.device != self.device:
            raise ValueError("states must be a contiguous (K, nt, N) = %s complex128 tensor on %s" % (
                (self.K, self.nt, self.N), self.device))
        if out is None:
            out = torch.empty((n_e, self.K, self.nt), dtype=torch.complex128, device=self.device)
        elif tuple(out.shape) != (n_e, self.K, self.nt) or out.dtype != torch.complex128 or not out.is_contiguous():
            raise ValueError("out must be a contiguous (n_e, K, nt) complex128 tensor")
        _lib.check(self._lib.kh_expect(self._handle, states.data_ptr(), table, n_e, out.data_ptr(), self._stream()))
        # the table and the operators until the stream has passed the launch (the next call replaces them)
        self._expect_keep = (table, uploaded)
        return out

    def chi_boundary(self, targets, psi_T, c, d):
        """Normalised boundary co-states ``(c_k target_k + d_k psi_k(T)) / ||.||`` and
        their norms, ``(K, N)`` and ``(K,)`` device tensors (kh_chi_boundary)."""
        targets = self._c(targets, (self.K, self.N))
        psi_T = self._c(psi_T, (self.K, self.N))
        c = self._c(c, (self.K,))
        d = self._c(d, (self.K,))
        chi = self._empty((self.K, self.N), torch.complex128)
        norms = self._empty((self.K,), torch.float64)
        _lib.check(self._lib.kh_chi_boundary(
            self._handle, targets.data_ptr(), psi_T.data_ptr(), c.data_ptr(), d.data_ptr(), chi.data_ptr(),
            norms.data_ptr(), self._stream()))
        return chi, norms

    def chi_local_invariants(self, psi_T, bell, mode, invariants=None, unitarity_weight=0.0, scale=1.0, out=None):
        """Normalised boundary co-states, their norms and the value J per gate of the perfect-entangler (``mode`` 'PE')
        or local-invariants ('LI') functional (``kh_chi_local_invariants``; krotov_amd/functionals.py:
        ``PerfectEntanglerChi``, ``LocalInvariantsChi``): ``(K, N)``, ``(K,)`` and ``(K / 4,)`` device tensors.
        ``bell``: the Bell states, ``(4, N)`` for all gates or ``(K / 4, 4, N)``; ``invariants`` ('LI'):
        ``(Re G_O, Im G_O, g3_O)`` of the target gate, ``(3,)`` or ``(K / 4, 3)``; ``scale``: the 1/M of an ensemble
        mean.  ``out``: the three tensors to write into -- on a replica engine an inactive replica's slices keep what
        they held.  A singular gate gives zero rows, norms 0 and J = NaN."""
        M = max(1, self.K // 4)  # (K not divisible by 4: the library refuses, KH_ERR_INVALID)
        modes = {'PE': 0, 'LI': 1, 0: 0, 1: 1}
        if mode not in modes:
            raise ValueError("mode must be 'PE' or 'LI', not %r" % (mode,))
        psi_T = self._c(psi_T, (self.K, self.N))
        bell = self.dev(bell, torch.complex128)
        if tuple(bell.shape) not in ((4, self.N), (M, 4, self.N)):
            raise ValueError("bell: expected shape %s or %s, got %s" % ((4, self.N), (M, 4, self.N), tuple(bell.shape)))
        inv = None
        if modes[mode] == 1:
            if invariants is None:
                raise ValueError("mode 'LI' needs the invariants (Re G_O, Im G_O, g3_O) of the target gate")
            inv = self.dev(invariants, torch.float64)
            if tuple(inv.shape) not in ((3,), (M, 3)):
                raise ValueError("invariants: expected shape (3,) or %s, got %s" % ((M, 3), tuple(inv.shape)))
        if out is None:
            chi = self._empty((self.K, self.N), torch.complex128)
            norms = self._empty((self.K,), torch.float64)
            J = self._empty((M,), torch.float64)
        else:
            chi = self._out(out[0], (self.K, self.N), torch.complex128)
            norms = self._out(out[1], (self.K,), torch.float64)
            J = self._out(out[2], (M,), torch.float64)
        _lib.check(self._lib.kh_chi_local_invariants(
            self._handle, psi_T.data_ptr(), bell.data_ptr(), int(bell.dim() == 3), modes[mode],
            None if inv is None else inv.data_ptr(), int(inv is not None and inv.dim() == 2), float(unitarity_weight),
            float(scale), chi.data_ptr(), norms.data_ptr(), J.data_ptr(), self._stream()))
        return chi, norms, J

    def pulse_gradient(self, fw_store, chi_store, chi_norms, pulses, out=None, per_objective=None):
        """The exact gradient of the time-discretised J_T for the pulse values (``kh_pulse_gradient``,
        krotov_amd/csrc/kh_grad.h): ``fw_store`` and ``chi_store`` are the ``(K, nt, N)`` stores of :meth:`forward`
        (``store=True``) and :meth:`backward` under the same ``pulses`` (L, nt-1), ``chi_norms`` the ``(K,)`` norms
        taken out of the boundary co-states (``None``: 1).  Returns the ``(L, nt-1)`` float64 gradient; ``out`` /
        ``per_objective``: buffers for it and for the ``(K, L, nt-1)`` terms of the sum over the objectives (``None``:
        a workspace of the library).  Dense uniform engines with 1 <= L <= 4 and N <= 96; ``KrotovHipError``
        (``KH_ERR_UNSUPPORTED``) beyond."""
        shape = (self.K, self.nt, self.N)
        for name, t in (('fw_store', fw_store), ('chi_store', chi_store)):
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.complex128
                    or not t.is_contiguous() or t.device != self.device):
                raise ValueError("%s must be a contiguous (K, nt, N) = %s complex128 tensor on %s" % (name, shape, self.device))
        pulses = self._f(pulses, (self.L, self.nt - 1))
        norms = None if chi_norms is None else self._f(chi_norms, (self.K,))
        out = self._out(out, (self.L, self.nt - 1), torch.float64)
        if per_objective is not None:
            per_objective = self._out(per_objective, (self.K, self.L, self.nt - 1), torch.float64)
        _lib.check(self._lib.kh_pulse_gradient(
            self._handle, fw_store.data_ptr(), chi_store.data_ptr(), None if norms is None else norms.data_ptr(),
            pulses.data_ptr(), out.data_ptr(), None if per_objective is None else per_objective.data_ptr(), self._stream()))
        return out

    def check(self):
        """Synchronise and raise if an in-kernel exchange timed out."""
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.kh_check(self._handle))

    def stats(self):
        buf = (ctypes.c_double * 4)()
        torch.cuda.synchronize(self.device)
        _lib.check(self._lib.kh_last_stats(self._handle, buf))
        return dict(matvecs=buf[0], intervals=buf[1], workgroups=buf[2])
