// The body of the generic plain sweeps (kh_generic.h: kh_gen_sweep_store, kh_gen_sweep_store_src), included into each of
// them so that the sweep without a source compiles to exactly the code it had as a function of its own (see
// kh_gen_update.inc).  Expects MIXED, SRC (constant expressions), the kernel's arguments p, mx, pulses, state_in, store,
// state_out, direction and sa (KhSrcArgs; read only where SRC).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KhGenLds s = kh_gen_carve(smem, p.N, p.csr == nullptr);
    const int tid = threadIdx.x, NS = p.N, L = p.L, nt = p.nt;
    double matvecs = 0.0;
    for (int k = blockIdx.x; k < p.K; k += gridDim.x) {
        const cplx *const *ops_k = p.ops + (size_t)k * (1 + L);
        const double *norms_k = p.op_norms + (size_t)k * (1 + L);
        const int N = MIXED ? mx.dims[k] : NS;
        const double fre = MIXED ? mx.f[k].x : p.fre, fim = MIXED ? mx.f[k].y : p.fim;
        // SRC: W of this objective and the norm taken out of chi_k(T)
        const cplx *src_k = SRC ? sa.src + (size_t)k * nt * NS : nullptr;
        const double chi_nrm = (SRC && sa.chi_norms != nullptr) ? sa.chi_norms[k] : 1.0;
        for (int i = tid; i < N; i += KH_GEN_THREADS) s.acc[i] = state_in[(size_t)k * NS + i];
        __syncthreads();
        if (store != nullptr) {
            const int idx0 = direction > 0 ? 0 : nt - 1;
            kh_gen_put<MIXED>(store + ((size_t)k * nt + idx0) * NS, s.acc, N, NS);
        }
        for (int step = 0; step < nt - 1; ++step) {
            const int n = direction > 0 ? step : nt - 2 - step;
            // (the interval's pulse values in LDS, thread l fetching control l: up to KH_GEN_MAX_L of them; the previous
            // step's readers are behind the barrier that ends its last term)
            if (tid < L) s.eps[tid] = pulses[(size_t)tid * (nt - 1) + n];
            const double hn = SRC ? 0.5 * p.dt[n] / chi_nrm : 0.0;
            if (SRC) {
                // chi[n+1] + h_n W[n+1]: element i is this thread's in kh_gen_put above too, and every writer of s.acc
                // in the series is behind the barrier that ends its last term
                for (int i = tid; i < N; i += KH_GEN_THREADS) {
                    const cplx wv = src_k[(size_t)(n + 1) * NS + i];
                    s.acc[i].x = fma(hn, wv.x, s.acc[i].x);
                    s.acc[i].y = fma(hn, wv.y, s.acc[i].y);
                }
            }
            __syncthreads();
            matvecs += kh_gen_expm_action(p, N, fre, fim, ops_k, p.csr ? p.csr + (size_t)k * (1 + L) : nullptr, norms_k,
                                          s.eps, p.dt[n], s);
            if (SRC) {
                // ... + h_n W[n], once per interval (not per sub-step of the series); read back by this thread only
                for (int i = tid; i < N; i += KH_GEN_THREADS) {
                    const cplx wv = src_k[(size_t)n * NS + i];
                    s.acc[i].x = fma(hn, wv.x, s.acc[i].x);
                    s.acc[i].y = fma(hn, wv.y, s.acc[i].y);
                }
            }
            if (store != nullptr) {
                const int idx = direction > 0 ? n + 1 : n;
                kh_gen_put<MIXED>(store + ((size_t)k * nt + idx) * NS, s.acc, N, NS);
            }
        }
        if (state_out != nullptr) kh_gen_put<MIXED>(state_out + (size_t)k * NS, s.acc, N, NS);
        __syncthreads();
    }
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
