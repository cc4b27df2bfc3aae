// Host-only check of kh_engine_create_replicas' argument handling (no device needed: every case returns before the first
// HIP call).  Meant for a sanitizer build of the host code, on a machine without a GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//         krotov_amd/csrc/krotov_hip.hip scripts/replica_args_check.cpp -o /tmp/replica_args_check && /tmp/replica_args_check
#include <cstdio>
#include <vector>

#include "krotov_hip.h"

static int failures = 0;
static void expect(const char *what, int got, int want) {
    if (got != want) {
        std::printf("FAIL %s: %d, expected %d (%s)\n", what, got, want, kh_last_error());
        ++failures;
    }
}

int main() {
    kh_engine *e = nullptr;
    expect("null problem", kh_engine_create_replicas(nullptr, 2, nullptr, &e), KH_ERR_INVALID);
    const int nt = 6;
    std::vector<double> dt(nt - 1, 0.1), dt_rep(3 * (nt - 1), 0.2);
    kh_cdouble blob[4] = {};
    auto problem = [&](int K, int N, int L, std::vector<const kh_cdouble *> &ops) {
        ops.assign((size_t)K * (1 + L), blob);
        kh_problem p = {};
        p.K = K, p.N = N, p.L = L, p.nt = nt;
        p.dt = dt.data();
        p.ops = ops.data();
        return p;
    };
    std::vector<const kh_cdouble *> ops;
    kh_problem p = problem(6, 4, 1, ops);
    expect("null out", kh_engine_create_replicas(&p, 2, nullptr, nullptr), KH_ERR_INVALID);
    expect("K not divisible", kh_engine_create_replicas(&p, 4, nullptr, &e), KH_ERR_INVALID);
    expect("no replicas", kh_engine_create_replicas(&p, 0, nullptr, &e), KH_ERR_INVALID);
    dt_rep[2 * (nt - 1) + 4] = -1.0;  // the last entry of the last replica's row
    expect("bad dt in the table", kh_engine_create_replicas(&p, 3, dt_rep.data(), &e), KH_ERR_INVALID);
    dt_rep[2 * (nt - 1) + 4] = 0.2;
    p.dt = nullptr;  // (allowed with a table) -- then the limits
    p.N = 17;
    expect("N = 17 with a table", kh_engine_create_replicas(&p, 3, dt_rep.data(), &e), KH_ERR_UNSUPPORTED);
    p = problem(18, 4, 1, ops);
    expect("K_r = 9", kh_engine_create_replicas(&p, 2, nullptr, &e), KH_ERR_UNSUPPORTED);
    p = problem(4, 4, 5, ops);
    expect("L = 5", kh_engine_create_replicas(&p, 2, nullptr, &e), KH_ERR_UNSUPPORTED);
    p = problem(4, 4, 0, ops);
    expect("L = 0", kh_engine_create_replicas(&p, 2, nullptr, &e), KH_ERR_UNSUPPORTED);
    p = problem(4, 4, 2, ops);
    ops[3] = nullptr;  // objective 1 has no drift
    expect("no drift", kh_engine_create_replicas(&p, 2, nullptr, &e), KH_ERR_INVALID);
    expect("mask on no engine", kh_set_active_replicas(nullptr, nullptr), KH_ERR_INVALID);
    expect("second order on no engine", kh_set_second_order_replicas(nullptr, nullptr, nullptr, nullptr), KH_ERR_INVALID);
    std::printf(failures ? "%d check(s) failed\n" : "all argument checks passed\n", failures);
    return failures ? 1 : 0;
}
