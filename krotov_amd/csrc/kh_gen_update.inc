// The body of the generic update kernels (kh_generic.h: kh_gen_forward_update, kh_gen_forward_update_par), included into
// each of them so that the unparametrized kernel compiles to exactly the code it had as a function of its own (see
// kh_tile64_update.inc).  Expects MIXED, PAR, NL (constant expressions), the kernel's arguments p, u, ex, mx, pa (KhParArgs;
// read only where PAR) and na (KhNlArgs; read only where NL).
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (u.n_dev != nullptr) {
        u.n_begin = *u.n_dev;
        u.n_end = u.n_begin + 1;
        if (u.n_begin >= p.nt - 1) return;  // replay past the last interval: nothing to do
    }
    const KhGenLds s = kh_gen_carve(smem, p.N, p.csr == nullptr);
    double *D_sh = s.D;  // all LDS in the dynamic region (keeps its base 16-byte aligned)
    int *ok_sh_p = s.ok;
    const int tid = threadIdx.x, NS = p.N, L = p.L, nt = p.nt;
    const int wave = tid >> 6, lane = tid & 63;
    double matvecs = 0.0;
    if (tid < L) s.ga[tid] = 0.0;  // (thread l keeps control l's scalars: eps, g_a, partial sum -- all in LDS)

    // One objective per workgroup and the sums on the adjoint side (no stage of the sweep then needs the state in global
    // memory): the running state stays in s.acc from interval to interval -- read once, written back once -- instead of
    // a global round trip in front of and behind every step.
    const bool resident = !MIXED && (int)gridDim.x >= p.K && u.adj_store != nullptr;
    if (resident && (int)blockIdx.x < p.K) {
        for (int i = tid; i < NS; i += KH_GEN_THREADS) s.acc[i] = u.phi[(size_t)blockIdx.x * NS + i];
        __syncthreads();
    }
    // partial sums of the first interval handled by this launch
    if (u.internal_exchange || u.n_begin == u.n_end) {
        // (stepwise mode enters with the partials of n_begin already reduced in D_in,
        //  except for the begin call n_begin == n_end == 0 which only emits them)
        if (u.n_begin < nt - 1) kh_gen_partials<MIXED>(p, u, mx, u.n_begin, s, resident);
    }
    if (!u.internal_exchange && u.n_begin == u.n_end) {
        if (tid < L) u.wg_partial[(size_t)blockIdx.x * L + tid] = u.n_begin < nt - 1 ? s.part[tid] : 0.0;
        return;
    }
    for (int n = u.n_begin; n < u.n_end; ++n) {
        // ---- cross-objective sum D_l (optimize.py:470) ----
        if (u.internal_exchange) {
            if (wave == 0) {
                bool ok;
                if (L <= KH_MAX_L) {
                    double part[KH_MAX_L], D[KH_MAX_L];
#pragma unroll
                    for (int l = 0; l < KH_MAX_L; ++l) part[l] = l < L ? s.part[l] : 0.0;
                    ok = kh_exchange<KH_MAX_L>(ex, n, blockIdx.x, L, lane, part, D);
                    if (lane == 0)
                        for (int l = 0; l < L; ++l) D_sh[l] = D[l];
                } else {
                    // more controls than a polling round keeps in registers: published at once (two granules per control
                    // and lane: 2 L <= 64), gathered in groups of KH_MAX_L.  One GPU only (the host sees to it: with more
                    // than KH_MAX_L controls a sharded run takes the all-reduce per interval, kh_p2p_create_window).
                    kh_exchange_publish(ex, n, blockIdx.x, L, lane, s.part);
                    ok = true;
                    for (int l0 = 0; l0 < L && ok; l0 += KH_MAX_L) {
                        double D[KH_MAX_L];
                        if (ex.G == 1) {
#pragma unroll
                            for (int l = 0; l < KH_MAX_L; ++l) D[l] = l0 + l < L ? s.part[l0 + l] : 0.0;
                        } else {
                            ok = kh_gather_range<KH_MAX_L, KH_GATHER_CHUNKS>(ex, n & 1, L, l0, (unsigned)(n + 1), lane, D);
                        }
                        if (lane == 0)
                            for (int l = 0; l < KH_MAX_L && l0 + l < L; ++l) D_sh[l0 + l] = D[l];
                    }
                }
                if (lane == 0) *ok_sh_p = ok ? 1 : 0;
            }
            __syncthreads();
            if (!*ok_sh_p) return;
        } else {
            if (tid < L) D_sh[tid] = u.D_in[tid];
            __syncthreads();
        }
        // ---- pulse update (optimize.py:471-477): thread l takes control l ----
        const double dt = p.dt[n];
        if constexpr (NL) {
            // non-linear controls: thread c takes control c -- the weighted sum over its terms, the update of eps_c, then
            // eps_c^p_j (repeated products) into every slot j of the control
            if (tid < na.C) {
                const int c = tid;
                double d1 = 0.0;
                for (int j = 0; j < L; ++j)
                    if (na.ctrl[j] == c) d1 += na.dcde[(size_t)j * (nt - 1) + n] * D_sh[j];
                const double S = u.shape[(size_t)c * (nt - 1) + n];
                const double lam = u.lambda[c];
                const double e = u.guess[(size_t)c * (nt - 1) + n] + (S / lam) * d1;
                s.ga[c] += (S / lam) * (d1 * d1) * dt;
                if (blockIdx.x == 0) u.opt[(size_t)c * (nt - 1) + n] = e;
                for (int j = 0; j < L; ++j) {
                    if (na.ctrl[j] != c) continue;
                    double v = e;
                    for (int q = 1; q < na.power[j]; ++q) v *= e;
                    s.eps[j] = v;
                }
            }
        } else if (tid < L) {
            const int l = tid;
            const double S = u.shape[(size_t)l * (nt - 1) + n];
            const double lam = u.lambda[l];
            double d1 = D_sh[l];
            if constexpr (PAR) d1 *= pa.dfdu[(size_t)l * (nt - 1) + n];  // dH/du = f'(u_guess) dH/d eps
            double e = u.guess[(size_t)l * (nt - 1) + n] + (S / lam) * d1;  // (PAR: u_new; `guess` holds u_guess)
            if constexpr (PAR) {
                if (blockIdx.x == 0) pa.u_opt[(size_t)l * (nt - 1) + n] = e;
                e = kh_par_eps(pa.kind[l], pa.a[l], pa.b[l], e);
            }
            s.eps[l] = e;
            s.ga[l] += (S / lam) * (d1 * d1) * dt;
            if (blockIdx.x == 0) u.opt[(size_t)l * (nt - 1) + n] = e;
        }
        __syncthreads();
        // ---- propagate every local objective over interval n (optimize.py:479-491) ----
        for (int k = blockIdx.x; k < p.K; k += gridDim.x) {
            const cplx *const *ops_k = p.ops + (size_t)k * (1 + L);
            const double *norms_k = p.op_norms + (size_t)k * (1 + L);
            const int N = MIXED ? mx.dims[k] : NS;
            const double fre = MIXED ? mx.f[k].x : p.fre, fim = MIXED ? mx.f[k].y : p.fim;
            if (!resident) {
                for (int i = tid; i < N; i += KH_GEN_THREADS) s.acc[i] = u.phi[(size_t)k * NS + i];
                __syncthreads();
            }
            if (u.fw_store != nullptr && n == 0) kh_gen_put<MIXED>(u.fw_store + (size_t)k * nt * NS, s.acc, N, NS);
            matvecs += kh_gen_expm_action(p, N, fre, fim, ops_k, p.csr ? p.csr + (size_t)k * (1 + L) : nullptr, norms_k,
                                          s.eps, dt, s);
            if (!resident || n + 1 == u.n_end) kh_gen_put<MIXED>(u.phi + (size_t)k * NS, s.acc, N, NS);
            if (u.fw_store != nullptr) kh_gen_put<MIXED>(u.fw_store + ((size_t)k * nt + n + 1) * NS, s.acc, N, NS);
            __syncthreads();
        }
        // ---- partial sums of the next interval ----
        if (n + 1 < nt - 1) {
            // phi written above by this same workgroup: visible after the barrier
            kh_gen_partials<MIXED>(p, u, mx, n + 1, s, resident);
            matvecs += (double)L;
        }
    }
    if (!u.internal_exchange && u.n_end < nt - 1 && tid < L) u.wg_partial[(size_t)blockIdx.x * L + tid] = s.part[tid];
    if (blockIdx.x == 0 && tid < (NL ? na.C : L)) u.g_a[tid] = (u.internal_exchange ? 0.0 : u.g_a[tid]) + s.ga[tid];
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
