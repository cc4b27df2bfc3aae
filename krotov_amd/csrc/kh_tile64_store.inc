// The body of the register-tile plain sweeps (kh_tile64.h: kh_tile_sweep_store, kh_tile_sweep_store_src), included into
// each of them so that the sweep without a source compiles to exactly the code it had as a function of its own (see
// kh_tile64_update.inc).  Expects RPT, LT, SRC (constant expressions), the kernel's arguments p, pulses, state_in, store,
// state_out, direction and sa (KhSrcArgs; read only where SRC).
//
// SRC (backward only): the co-state equation with a source, trapezoid in the source and the engine's own step V_n,
//     chi[n] = V_n (chi[n+1] + h_n W[n+1]) + h_n W[n],   h_n = dt_n / 2 / ||chi_k(T)||
// The vector an interval starts from (chi[n] + h_{n-1} W[n]) and the one that is stored (chi[n]) differ, so the stored
// one is staged in a buffer of its own (sbuf, by step parity: wave 0 may still read the one of step s while the writers of
// step s + 1 fill the other), and ONE barrier per interval orders both writes against their readers.
    __shared__ __attribute__((aligned(16))) cplx buf[2][KH_TILE_N];
    __shared__ __attribute__((aligned(16))) cplx sbuf[SRC ? 2 : 1][SRC ? KH_TILE_N : 1];
    __shared__ __attribute__((aligned(16))) double inv_sh[KH_MAX_DEGREE + 2];
    __shared__ __attribute__((aligned(16))) double deg_sh[KH_MAX_DEGREE + 2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool writer = KhTile<RPT>::writer(lane);
    if (tid <= KH_MAX_DEGREE) {
        deg_sh[tid] = p.q2_theta[tid];
    }
    const int N = p.N, nt = p.nt;
    double matvecs = 0.0;
    for (int k = blockIdx.x; k < p.K; k += gridDim.x) {
        const cplx *const *ops_k = p.ops + (size_t)k * (1 + LT);
        const double *norms_k = p.op_norms + (size_t)k * (1 + LT);
        KhTileOps<RPT, LT, KhTileLds<RPT, LT>::STORE> h;
        h.load(ops_k, N, wave, lane, kh_tile_dyn_lds, tid);
        double nrm[1 + LT];
#pragma unroll
        for (int o = 0; o <= LT; ++o) nrm[o] = norms_k[o];

        cplx state[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int row = KhTile<RPT>::row(wave, lane, r);
            state[r] = row < N ? state_in[(size_t)k * N + row] : c_make(0.0, 0.0);
        }
        // SRC: this lane's rows of W at the time point the coming interval ends at, and the norm taken out of chi_k(T)
        const cplx *src_k = SRC ? sa.src + (size_t)k * nt * N : nullptr;
        const double chi_nrm = (SRC && sa.chi_norms != nullptr) ? sa.chi_norms[k] : 1.0;
        cplx w[RPT];
        if (SRC) {
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const int row = KhTile<RPT>::row(wave, lane, r);
                w[r] = row < N ? src_k[(size_t)(nt - 1) * N + row] : c_make(0.0, 0.0);
            }
        }
        __syncthreads();  // previous objective's readers are done with buf
        int cur = 0;
        if (SRC) {
            // chi(T) is stored as it is; the first interval starts from chi(T) + h W[nt-1]
            const double hn = nt > 1 ? 0.5 * p.dt[nt - 2] / chi_nrm : 0.0;
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                if (writer) sbuf[1][KhTile<RPT>::row(wave, lane, r)] = state[r];
                state[r].x = fma(hn, w[r].x, state[r].x);
                state[r].y = fma(hn, w[r].y, state[r].y);
            }
        }
        if (writer) {
#pragma unroll
            for (int r = 0; r < RPT; ++r) buf[0][KhTile<RPT>::row(wave, lane, r)] = state[r];
        }
        __syncthreads();
        if (store != nullptr && wave == 0 && lane < N)
            store[((size_t)k * nt + (direction > 0 ? 0 : nt - 1)) * N + lane] = SRC ? sbuf[1][lane] : buf[0][lane];

        // per-interval scalars are fetched one interval ahead (their load
        // latency would otherwise sit on the critical path of every interval)
        const int n0 = direction > 0 ? 0 : nt - 2;
        double eps_next[LT], dt_next = p.dt[n0];
#pragma unroll
        for (int l = 0; l < LT; ++l) eps_next[l] = pulses[(size_t)l * (nt - 1) + n0];
        int m_hint = 12;
        for (int step = 0; step < nt - 1; ++step) {
            const int n = direction > 0 ? step : nt - 2 - step;
            double eps[LT];
            double theta = nrm[0];
            const double dt = dt_next;
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                eps[l] = eps_next[l];
                theta += fabs(eps[l]) * nrm[1 + l];
            }
            if (step + 1 < nt - 1) {
                const int nn = direction > 0 ? n + 1 : n - 1;
                dt_next = p.dt[nn];
#pragma unroll
                for (int l = 0; l < LT; ++l) eps_next[l] = pulses[(size_t)l * (nt - 1) + nn];
            }
            if (SRC) {
                // W[n], needed behind the series of this interval: in flight while it runs
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    const int row = KhTile<RPT>::row(wave, lane, r);
                    w[r] = row < N ? src_k[(size_t)n * N + row] : c_make(0.0, 0.0);
                }
            }
            int nsub, m;
            kh_degree_lookup(theta * dt, deg_sh, p.theta_max, p.inv_theta_max, m_hint, &nsub, &m);
            if (m != m_hint || step == 0) kh_tile_load_ratios(p, inv_sh, m, tid);  // (workgroup-uniform, rare)
            m_hint = m;
            cplx a[RPT][8];
            h.build(eps, a);
            matvecs += kh_tile_expm_action<RPT>(a, state, buf, inv_sh, cur, p.fre, p.fim, dt, nsub, m, wave, lane);
            if (SRC) {
                // chi[n] = V_n (...) + h_n W[n] -> sbuf (stored below); chi[n] + h_{n-1} W[n] -> buf[cur], what the next
                // interval starts from.  Nobody reads buf[cur] or sbuf[step & 1] now: the series' last barrier is behind
                // every reader of buf, the barrier of the previous interval behind the reader of this sbuf.
                const double hn = 0.5 * dt / chi_nrm;
                const double hp = step + 1 < nt - 1 ? 0.5 * dt_next / chi_nrm : 0.0;
#pragma unroll
                for (int r = 0; r < RPT; ++r) {
                    const int row = KhTile<RPT>::row(wave, lane, r);
                    state[r].x = fma(hn, w[r].x, state[r].x);
                    state[r].y = fma(hn, w[r].y, state[r].y);
                    if (writer) sbuf[step & 1][row] = state[r];
                    if (step + 1 < nt - 1) {
                        state[r].x = fma(hp, w[r].x, state[r].x);
                        state[r].y = fma(hp, w[r].y, state[r].y);
                    }
                    if (writer) buf[cur][row] = state[r];
                }
                __syncthreads();
                if (store != nullptr && wave == 0 && lane < N)
                    store[((size_t)k * nt + n) * N + lane] = sbuf[step & 1][lane];
                continue;
            }
            // buf[cur] now holds the new state: stream it to HBM, one coalesced 1 KiB store
            if (store != nullptr && wave == 0 && lane < N)
                store[((size_t)k * nt + (direction > 0 ? n + 1 : n)) * N + lane] = buf[cur][lane];
        }
        if (state_out != nullptr && wave == 0 && lane < N) state_out[(size_t)k * N + lane] = buf[cur][lane];
    }
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
