// The body of the register-tile update kernels (kh_tile64.h: kh_tile_forward_update, kh_tile_forward_update_par), included
// into each of them: the two share every line, and the unparametrized kernel, which sits at the register limit, must
// compile to exactly the code it had as a function of its own -- a shared device function, even a forced-inline one, moved
// its register allocation.  Expects RPT, LT, SO, SINGLE, PAR, NL (constant expressions), the kernel's arguments p, u, ex, pa
// (KhParArgs; read only where PAR) and na (KhNlArgs; read only where NL: the LT slots are then the terms eps_c(l)^p_l H_l).
    if (u.n_dev != nullptr) {  // graph-replayed stepwise mode: interval index from device memory
        u.n_begin = *u.n_dev;
        u.n_end = u.n_begin + 1;
        if (u.n_begin >= p.nt - 1) return;
    }
    constexpr int WAVES = KhTile<RPT>::WAVES;
    __shared__ __attribute__((aligned(16))) cplx buf[2][KH_TILE_N];
    __shared__ __attribute__((aligned(16))) double red[2][WAVES][LT][2];  // double-buffered on interval parity
    __shared__ __attribute__((aligned(16))) double D_sh[2][LT + 1];       // the reduced sums, by interval parity
    __shared__ __attribute__((aligned(16))) double ok_sh[2][LT];          // ... and whether their gather came back
    __shared__ __attribute__((aligned(16))) double inv_sh[KH_MAX_DEGREE + 2];
    __shared__ __attribute__((aligned(16))) double deg_sh[KH_MAX_DEGREE + 2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, cg = KhTileLanes::cg(lane);
    const bool writer = KhTile<RPT>::writer(lane);
    if (tid <= KH_MAX_DEGREE) {
        deg_sh[tid] = p.q2_theta[tid];
    }
    const int N = p.N, nt = p.nt;
    const int k = blockIdx.x;
    double matvecs = 0.0;

    const cplx *const *ops_k = p.ops + (size_t)k * (1 + LT);
    const double *norms_k = p.op_norms + (size_t)k * (1 + LT);
    // (PAR: f and its operands take the registers that let SINGLE park nothing with three controls)
    KhTileOps<RPT, LT, (SINGLE && !PAR) ? KhTileLds<RPT, LT>::UPDATE_SINGLE : KhTileLds<RPT, LT>::UPDATE> h;
    h.load(ops_k, N, wave, lane, kh_tile_dyn_lds, tid);
    double nrm[1 + LT];
#pragma unroll
    for (int o = 0; o <= LT; ++o) nrm[o] = kh_uniform(norms_k[o]);
    // dH/d eps_l is the forward control operator itself (mu.py:123-134): h[1+l] serves both
    const double chi_norm = kh_uniform(u.chi_norms[k]);

    cplx state[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int row = KhTile<RPT>::row(wave, lane, r);
        state[r] = row < N ? u.phi[(size_t)k * N + row] : c_make(0.0, 0.0);
    }
    int cur = 0;
    if (writer) {
#pragma unroll
        for (int r = 0; r < RPT; ++r) buf[0][KhTile<RPT>::row(wave, lane, r)] = state[r];
    }
    __syncthreads();

    double g_a_loc[LT];
#pragma unroll
    for (int l = 0; l < LT; ++l) g_a_loc[l] = 0.0;

    // chi_k(t_n) rows for this lane, fetched one interval ahead; second order: also the rows of the
    // state propagated under the guess pulses and 0.5 sigma_n / ||chi|| (optimize.py:468-469)
    cplx chi[RPT], prev[RPT];
    double hs = 0.0;
#pragma unroll
    for (int r = 0; r < RPT; ++r) prev[r] = c_make(0.0, 0.0);
    auto load_chi = [&](int n) {
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int row = KhTile<RPT>::row(wave, lane, r);
            chi[r] = row < N ? u.chi_store[((size_t)k * nt + n) * N + row] : c_make(0.0, 0.0);
            if constexpr (SO) prev[r] = row < N ? u.fw_prev[((size_t)k * nt + n) * N + row] : c_make(0.0, 0.0);
        }
        if constexpr (SO) hs = 0.5 * u.sigma[n] / chi_norm;
    };

    // wave-level pieces of  chi_norm * Im(mu <chi(t_n) | H_l phi>)  -> red[par][wave]; phi in buf[cur]
    // The broadcast vector is read ONCE for all L controls, and no product is summed over its row: chi (and the
    // second-order bra) is replicated over the row's 8 lanes, so every lane multiplies its own 8-column share with the
    // bra and ONE 64-lane sum per control (on the matrix core) adds shares and rows together.
    auto partial_pieces = [&](int par) {
        cplx xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = buf[cur][cg + 8 * j];
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            cplx y[RPT];
            h.matvec_part(1 + l, xv, y);
            cplx ov = c_make(0.0, 0.0);
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                // second order: the bra is chi + hs (phi - phi_prev)
                cplx bra = chi[r];
                if constexpr (SO)
                    bra = c_make(fma(hs, state[r].x - prev[r].x, chi[r].x),
                                 fma(hs, state[r].y - prev[r].y, chi[r].y));
                c_fma_conj(ov, bra, y[r]);
            }
            // Im(mu <bra | H_l phi>) needs only one real combination: reduce that, not both parts
            const double v = sum64_mfma(u.mu_re * ov.y + u.mu_im * ov.x);
            if (lane == 0) red[par][wave][l][0] = v;
        }
        matvecs += LT;
    };
    // after a barrier: the workgroup's partial sums, same value in every thread
    auto partial_total = [&](int par, double (&part)[LT]) {
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            double acc = 0.0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) acc += red[par][w][l][0];
            part[l] = chi_norm * acc;
        }
    };

    const bool emit_only = (!u.internal_exchange && u.n_begin == u.n_end);
    if ((u.internal_exchange || emit_only) && u.n_begin < nt - 1) {
        load_chi(u.n_begin);
        partial_pieces(u.n_begin & 1);
    }
    __syncthreads();
    if (emit_only) {
        double part[LT];
        partial_total(u.n_begin & 1, part);
        if (tid == 0)
            for (int l = 0; l < LT; ++l) u.wg_partial[(size_t)k * LT + l] = part[l];
        return;
    }

    // per-interval scalars, fetched one interval ahead
    // (wave-uniform values are kept in scalar registers: with L = 3, 4 the per-control scalars
    // would otherwise cost ~60 VGPRs next to the operator tiles)
    // (NL: term l reads the row of its control c(l) -- every per-term array below then holds its control's value, and no
    // array is indexed by a run-time control number; nl_same[l]: the terms of the same control as a bit mask, l's bit set)
    int nl_row[LT], nl_pow[LT], nl_same[LT];
    if constexpr (NL) {
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            nl_row[l] = __builtin_amdgcn_readfirstlane(na.ctrl[l]);
            nl_pow[l] = __builtin_amdgcn_readfirstlane(na.power[l]);
        }
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            nl_same[l] = 0;
#pragma unroll
            for (int i = 0; i < LT; ++i) nl_same[l] |= (nl_row[i] == nl_row[l]) ? (1 << i) : 0;
        }
    }
    double dt_next = kh_uniform(p.dt[u.n_begin]), guess_next[LT], shape_next[LT], lam[LT];
#pragma unroll
    for (int l = 0; l < LT; ++l) {
        const int row = NL ? nl_row[l] : l;
        guess_next[l] = kh_uniform(u.guess[(size_t)row * (nt - 1) + u.n_begin]);
        shape_next[l] = kh_uniform(u.shape[(size_t)row * (nt - 1) + u.n_begin]);
        lam[l] = kh_uniform(u.lambda[row]);
    }
    // (PAR: `guess` is u_guess; the derivative travels with it, the kind and its two parameters stay for the sweep)
    double dfdu_next[LT], par_a[LT], par_b[LT];
    int par_kind[LT];
    // (NL: the same three arrays carry the terms' weights w_l = d(eps^p_l)/d eps at the guess)
    if constexpr (NL) {
#pragma unroll
        for (int l = 0; l < LT; ++l) dfdu_next[l] = kh_uniform(na.dcde[(size_t)l * (nt - 1) + u.n_begin]);
    }
    if constexpr (PAR) {
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            dfdu_next[l] = kh_uniform(pa.dfdu[(size_t)l * (nt - 1) + u.n_begin]);
            par_kind[l] = __builtin_amdgcn_readfirstlane(pa.kind[l]);
            par_a[l] = kh_uniform(pa.a[l]);
            par_b[l] = kh_uniform(pa.b[l]);
        }
    }
    int m_hint = 12;

    for (int n = u.n_begin; n < u.n_end; ++n) {
        const int par = n & 1;
        if (n + 1 < nt - 1) load_chi(n + 1);  // lands while this interval is processed
        // ---- cross-objective sum (optimize.py:470) ----
        if (SINGLE || u.internal_exchange) {
            constexpr int CH = RPT == 2 ? KH_GATHER_CHUNKS_WIDE : KH_GATHER_CHUNKS;  // (256-thread workgroups run two per CU)
            if (LT > 1 && LT <= WAVES && (SINGLE || (ex.world == 1 && ex.G > 1))) {
                // several controls, one GPU: wave 0 publishes all of them, wave l gathers control l -- L polling
                // rounds side by side instead of one wave polling 8 L granules per lane (measured: the exchange cost
                // 2.4 us per interval at L = 2 and 4.1 us at L = 4 against 1.25 us with one control)
                if (wave == 0) {
                    double part[LT];
                    partial_total(par, part);
                    kh_exchange_publish(ex, n, k, LT, lane, part);
                }
                if (wave < LT) {
                    double Dl = 0.0;
                    const bool ok = kh_gather_one<CH>(ex, par, LT, wave, (unsigned)(n + 1), lane, Dl);
                    if (lane == 0) {
                        D_sh[par][wave] = Dl;
                        ok_sh[par][wave] = ok ? 1.0 : 0.0;
                    }
                }
            } else if (wave == 0) {
                double part[LT];
                partial_total(par, part);
                double D[LT];
                const bool ok = kh_exchange<LT, CH, !SINGLE>(ex, n, k, LT, lane, part, D);
                if (lane == 0) {
#pragma unroll
                    for (int l = 0; l < LT; ++l) {
                        D_sh[par][l] = D[l];
                        ok_sh[par][l] = ok ? 1.0 : 0.0;
                    }
                }
            }
        } else if (tid == 0) {
            for (int l = 0; l < LT; ++l) {
                D_sh[par][l] = u.D_in[l];
                ok_sh[par][l] = 1.0;
            }
        }
        // scalars of this interval (prefetched) and prefetch of the next
        const double dt = dt_next;
        double guess[LT], shape[LT];
#pragma unroll
        for (int l = 0; l < LT; ++l) {
            guess[l] = guess_next[l];
            shape[l] = shape_next[l];
        }
        double dt_ld = 0.0, guess_ld[LT], shape_ld[LT];  // in flight across the barrier
        double dfdu[LT], dfdu_ld[LT];
        if constexpr (PAR || NL) {
#pragma unroll
            for (int l = 0; l < LT; ++l) dfdu[l] = dfdu_next[l];
        }
        if (n + 1 < nt - 1) {
            dt_ld = p.dt[n + 1];
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                const int row = NL ? nl_row[l] : l;
                guess_ld[l] = u.guess[(size_t)row * (nt - 1) + n + 1];
                shape_ld[l] = u.shape[(size_t)row * (nt - 1) + n + 1];
                if constexpr (PAR) dfdu_ld[l] = pa.dfdu[(size_t)l * (nt - 1) + n + 1];
                if constexpr (NL) dfdu_ld[l] = na.dcde[(size_t)l * (nt - 1) + n + 1];
            }
        }
        __syncthreads();
        {
            bool all_ok = true;
#pragma unroll
            for (int l = 0; l < LT; ++l) all_ok = all_ok && ok_sh[par][l] != 0.0;
            if (!all_ok) return;
        }
        // ---- pulse update (optimize.py:471-477) ----
        double eps[LT];
        double theta = nrm[0];
        if constexpr (NL) {
            // D_c = sum_{j in c} w_j D_j, formed once per term of the control (same terms, same order: the same value);
            // eps_c written from every term of the control (the same value), g_a from its first term
            double wd[LT];
#pragma unroll
            for (int l = 0; l < LT; ++l) wd[l] = dfdu[l] * D_sh[par][l];
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                double d1 = 0.0;
#pragma unroll
                for (int i = 0; i < LT; ++i) d1 += ((nl_same[l] >> i) & 1) ? wd[i] : 0.0;
                const double step = shape[l] / lam[l];
                const double e = kh_uniform(guess[l] + step * d1);
                g_a_loc[l] = kh_uniform(g_a_loc[l] + step * (d1 * d1) * dt);
                if (k == 0 && tid == 0) u.opt[(size_t)nl_row[l] * (nt - 1) + n] = e;
                double c = e;  // eps_c^p_l by repeated multiplication
#pragma unroll
                for (int q = 1; q < 4; ++q) c = q < nl_pow[l] ? c * e : c;
                eps[l] = kh_uniform(c);
                theta += fabs(eps[l]) * nrm[1 + l];
            }
        }
#pragma unroll
        for (int l = 0; !NL && l < LT; ++l) {
            double d1 = D_sh[par][l];
            if constexpr (PAR) d1 *= dfdu[l];  // dH/du = f'(u_guess) dH/d eps
            const double step = shape[l] / lam[l];
            eps[l] = kh_uniform(guess[l] + step * d1);
            g_a_loc[l] = kh_uniform(g_a_loc[l] + step * (d1 * d1) * dt);
            if constexpr (PAR) {
                // eps[l] is u_new here: stored, then the interval is propagated with f(u_new)
                if (k == 0 && tid == 0) pa.u_opt[(size_t)l * (nt - 1) + n] = eps[l];
                eps[l] = kh_uniform(kh_par_eps(par_kind[l], par_a[l], par_b[l], eps[l]));
            }
            theta += fabs(eps[l]) * nrm[1 + l];
        }
        if (!NL && k == 0 && tid == 0) {
#pragma unroll
            for (int l = 0; l < LT; ++l) u.opt[(size_t)l * (nt - 1) + n] = eps[l];
        }
        // ---- propagate over interval n with the updated pulse (optimize.py:479-491) ----
        int nsub, m;
        kh_degree_lookup(theta * dt, deg_sh, p.theta_max, p.inv_theta_max, m_hint, &nsub, &m);
        if (m != m_hint || n == u.n_begin) kh_tile_load_ratios(p, inv_sh, m, tid);  // (workgroup-uniform, rare)
        m_hint = m;
        cplx a[RPT][8];
        h.build(eps, a);
        if constexpr (SO) {
            if (wave == 0 && lane < N) u.fw_store[((size_t)k * nt + n) * N + lane] = buf[cur][lane];
        }
        matvecs += kh_tile_expm_action<RPT>(a, state, buf, inv_sh, cur, p.fre, p.fim, dt, nsub, m, wave, lane);
        if (n + 1 < nt - 1) {
            dt_next = kh_uniform(dt_ld);
#pragma unroll
            for (int l = 0; l < LT; ++l) {
                guess_next[l] = kh_uniform(guess_ld[l]);
                shape_next[l] = kh_uniform(shape_ld[l]);
                if constexpr (PAR || NL) dfdu_next[l] = kh_uniform(dfdu_ld[l]);
            }
        }
        // ---- partial sums of the next interval (state is in buf[cur], barrier passed) ----
        if (n + 1 < nt - 1) {
            partial_pieces((n + 1) & 1);
            __syncthreads();  // every wave's piece is in red[] before wave 0 totals it
        }
    }
    // running state back to the engine workspace (final states / next launch)
    if (wave == 0 && lane < N) {
        u.phi[(size_t)k * N + lane] = buf[cur][lane];
        if constexpr (SO) u.fw_store[((size_t)k * nt + u.n_end) * N + lane] = buf[cur][lane];
    }
    if (!u.internal_exchange && u.n_end < nt - 1) {
        double part[LT];
        partial_total(u.n_end & 1, part);
        if (tid == 0)
            for (int l = 0; l < LT; ++l) u.wg_partial[(size_t)k * LT + l] = part[l];
    }
    if constexpr (NL) {
        if (k == 0 && tid == 0)
            for (int l = 0; l < LT; ++l)
                if ((nl_same[l] & ((1 << l) - 1)) == 0)  // (the control's first term)
                    u.g_a[nl_row[l]] = (u.internal_exchange ? 0.0 : u.g_a[nl_row[l]]) + g_a_loc[l];
    }
    if (!NL && k == 0 && tid == 0)
        for (int l = 0; l < LT; ++l) u.g_a[l] = (u.internal_exchange ? 0.0 : u.g_a[l]) + g_a_loc[l];
    if (tid == 0 && p.stats != nullptr) atomicAdd(p.stats, matvecs);
