// Micro-benchmark behind DESIGN.md section 3.3 ("would an XCD-local exchange help the update sweep?"): the per-interval
// sum over 512 workgroups (two per CU, 512 threads each, as kh_q2_forward_update runs), iterated with a data
// dependency from one sum to the next publication, in two forms:
//   FLAT  every workgroup publishes one epoch-tagged granule and gathers all 512 (agent scope, memory side) -- what
//         the kernels do (kh_common.h);
//   XCD   two stages: the 64 workgroups of an XCD (blockIdx % 8, checked against XCC_ID) exchange through their L2
//         (workgroup-scope stores, agent-scope loads), every member forms the XCD's sum, member 0 publishes it (a slot
//         per XCD, each in its own 128-byte line; all 64 members storing the same value to one slot costs 13 us: the
//         stores of 512 CUs to one line are serialised at the memory side) and all gather the 8 XCD sums.
// Both end with the same LDS broadcast + barrier.  Prints ns per exchange.  (`ubench_exchange xcd`)
//
// Second table (the default; DESIGN.md section 3.3, "slot layout"): the FLAT form as the library runs it on the headline
// -- 256 workgroups of 512 threads, one per CU, a double published as two epoch-tagged 8-byte granules, wave 0 gathering
// workgroups lane + 64 c with two 8-byte loads each -- over the layout of the slot array:
//   W      writers per 128-byte line, 8 / 4 / 2 / 1: the slot stride is 128 / W bytes (the library's layout before: 8);
//   form   two 8-byte stores from lanes 0 and 1, or ONE 16-byte store from lane 0 (the reader checks both tags, so a
//          torn 16-byte store is harmless);
//   map    which workgroups share a line: consecutive ids (eight XCDs' L2s write to a line), or ids congruent mod 8
//          (the writers of a line sit on one XCD);
//   delay  the head start between the store and the first poll, in s_sleep units of 64 cycles.
// A third table scans the delay in single units around the best of the second, and adds the form of the poll: two
// 8-byte loads per slot, or one 16-byte load (half the load instructions of a polling round).
// Prints us per exchange on top of the work: median and range (max - min) over the repeats.
// Build: hipcc --offload-arch=gfx950 -O3 scripts/ubench_exchange.hip -o build/ubench_exchange
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <algorithm>

typedef unsigned long long u64;
#define WGS 512
#define THREADS 512

__device__ __forceinline__ unsigned int xcc_id() { return __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 0xf; }

__device__ __forceinline__ float wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// (payload: a float in the low half of the granule; the tag in the high half)
__device__ __forceinline__ u64 pack(unsigned int epoch, float v) { return ((u64)epoch << 32) | __float_as_uint(v); }

template <int MODE, int SLEEP>
__global__ void __launch_bounds__(THREADS) k(u64 *flat, u64 *local, u64 *cross, int iters, float *out, int *misplaced,
                                              int work, int d1, int d2) {
    __shared__ float red[8];
    __shared__ float total;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wg = blockIdx.x, grp = wg & 7, member = wg >> 3;
    if (tid == 0 && xcc_id() != (unsigned)grp) atomicAdd(misplaced, 1);
    float mine = 1.0f + 1e-3f * wg;
    for (int it = 1; it <= iters; ++it) {
        const int par = it & 1;
        float sum;
        for (int w = 0; w < work; ++w) __builtin_amdgcn_s_sleep(1);  // the interval's products (no memory traffic)
        if (MODE == 3) {
            sum = mine;
        } else if (MODE == 0) {
            if (tid == 0) __hip_atomic_store(flat + par * WGS + wg, pack(it, mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            u64 g;
            for (int w = 0; w < d1; ++w) __builtin_amdgcn_s_sleep(1);
            do {
                g = __hip_atomic_load(flat + par * WGS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (SLEEP && (unsigned int)(g >> 32) != (unsigned int)it) __builtin_amdgcn_s_sleep(1);
            } while ((unsigned int)(g >> 32) != (unsigned int)it);
            const float s = wave_sum(__uint_as_float((unsigned int)g));
            if (lane == 0) red[wave] = s;
            __syncthreads();
            if (tid == 0) total = ((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]));
            __syncthreads();
            sum = total;
        } else {
            if (wave == 0) {
                if (lane == 0) {
                    if (MODE == 1)
                        __hip_atomic_store(local + (par * 8 + grp) * 64 + member, pack(it, mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else
                        __hip_atomic_store(local + (par * 8 + grp) * 64 + member, pack(it, mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                u64 g;
                for (int w = 0; w < d1; ++w) __builtin_amdgcn_s_sleep(1);
                do {
                    g = __hip_atomic_load(local + (par * 8 + grp) * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (SLEEP && (unsigned int)(g >> 32) != (unsigned int)it) __builtin_amdgcn_s_sleep(1);
                } while ((unsigned int)(g >> 32) != (unsigned int)it);
                const float sg = wave_sum(__uint_as_float((unsigned int)g));
                if (lane == 0 && member == 0) __hip_atomic_store(cross + (par * 8 + grp) * 16, pack(it, sg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                float v = 0.0f;
                for (int w = 0; w < d2; ++w) __builtin_amdgcn_s_sleep(1);
                if (lane < 8) {
                    do {
                        g = __hip_atomic_load(cross + (par * 8 + lane) * 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (SLEEP && (unsigned int)(g >> 32) != (unsigned int)it) __builtin_amdgcn_s_sleep(1);
                    } while ((unsigned int)(g >> 32) != (unsigned int)it);
                    v = __uint_as_float((unsigned int)g);
                }
                const float s = wave_sum(v);
                if (lane == 0) total = s;
            }
            __syncthreads();
            sum = total;
            __syncthreads();
        }
        mine = 1.0f + 1e-9f * sum + 1e-3f * wg;  // (the next publication depends on the sum)
    }
    if (tid == 0) out[wg] = mine;
}

template <int MODE, int SLEEP>
static float run(u64 *flat, u64 *local, u64 *cross, float *out, int *misplaced, int work, int d1, int d2, int *mis) {
    const int iters = 20000;
    float ms = 0.0f;
    for (int rep = 0; rep < 2; ++rep) {
        hipMemset(flat, 0, 2 * WGS * 8);
        hipMemset(local, 0, 2 * 8 * 64 * 8);
        hipMemset(cross, 0, 2 * 8 * 16 * 8);
        hipMemset(misplaced, 0, 4);
        hipEvent_t a, b;
        hipEventCreate(&a);
        hipEventCreate(&b);
        hipEventRecord(a);
        void *args[] = {&flat, &local, &cross, (void *)&iters, &out, &misplaced, &work, &d1, &d2};
        const hipError_t err = hipLaunchCooperativeKernel((const void *)k<MODE, SLEEP>, dim3(WGS), dim3(THREADS), args, 0, 0);
        if (err != hipSuccess) {
            printf("launch failed: %s\n", hipGetErrorString(err));
            return -1.0f;
        }
        hipEventRecord(b);
        hipEventSynchronize(b);
        hipEventElapsedTime(&ms, a, b);
    }
    hipMemcpy(mis, misplaced, 4, hipMemcpyDeviceToHost);
    return ms * 1e6f / iters;
}

// ---- slot layouts of the flat form --------------------------------------------------------------------------------
#define LWGS 256        // one workgroup per CU
#define LSLOTS (2 * 512 * 16)  // granules: two parities, up to 512 slots of a whole line
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// slot of a workgroup: consecutive ids, or (PERM) the ids congruent mod 8 -- one XCD's -- next to each other
__device__ __forceinline__ int slot_of(int wg, int perm, int rows) { return perm ? (wg & 7) * rows + (wg >> 3) : wg; }

__global__ void __launch_bounds__(THREADS) k_layout(u64 *slots, int iters, double *out, unsigned int *failed, int work,
                                                    int delay, int stride, int one_store, int perm, int exchange, int wide_load) {
    __shared__ double total;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wg = blockIdx.x, G = gridDim.x;
    const int rows = (G + 7) / 8;
    const size_t par_stride = (size_t)8 * rows * stride;  // (8 * rows >= G slots per parity)
    double mine = 1.0 + 1e-3 * wg;
    for (int it = 1; it <= iters; ++it) {
        const int par = it & 1;
        for (int w = 0; w < work; ++w) __builtin_amdgcn_s_sleep(1);  // the interval's products (no memory traffic)
        if (!exchange) {
            if (tid == 0) total = mine;
        } else if (wave == 0) {
            const u64 bits = (u64)__double_as_longlong(mine);
            const u64 tag = (u64)(unsigned int)it << 32;
            u64 *g = slots + par * par_stride + (size_t)slot_of(wg, perm, rows) * stride;
            if (one_store) {
                if (lane == 0) {
                    const u32x4 v = {(unsigned int)(bits >> 32), (unsigned int)it, (unsigned int)bits, (unsigned int)it};
                    // (agent scope as the 8-byte atomic stores compile: write-through to the memory side)
                    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(g), "v"(v) : "memory");
                }
            } else if (lane < 2) {
                const u64 half = lane ? (bits & 0xffffffffull) : (bits >> 32);
                __hip_atomic_store(g + lane, tag | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            for (int w = 0; w < delay; ++w) __builtin_amdgcn_s_sleep(1);
            u64 a[4], b[4];
            unsigned int spins = 0;
            bool gave_up = false;
            for (;;) {
                bool ok = true;
if (wide_load) {
                    const u64 *q[4];
                    u32x4 v[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {  // (a lane without a workgroup reads slot 0 and drops it)
                        const int src = lane + 64 * c < G ? lane + 64 * c : 0;
                        q[c] = slots + par * par_stride + (size_t)slot_of(src, perm, rows) * stride;
                    }
                    asm volatile(
                        "global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\t"
                        "global_load_dwordx4 %2, %6, off sc1\n\tglobal_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                        : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
                        : "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3])
                        : "memory");
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        a[c] = ((u64)v[c].y << 32) | v[c].x;
                        b[c] = ((u64)v[c].w << 32) | v[c].z;
                        if (lane + 64 * c >= G) a[c] = b[c] = tag;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int src = lane + 64 * c;
                        if (src < G) {
                            const u64 *q = slots + par * par_stride + (size_t)slot_of(src, perm, rows) * stride;
                            a[c] = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            b[c] = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        } else {
                            a[c] = b[c] = tag;
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) ok = ok && (a[c] >> 32) == (tag >> 32) && (b[c] >> 32) == (tag >> 32);
                if (__all(ok)) break;
                __builtin_amdgcn_s_sleep(1);
                // bounded: a lost store must end the run, not hang the device
                if ((++spins & 255u) == 0 &&
                    (spins > (1u << 22) || __hip_atomic_load(failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
                    if (lane == 0) __hip_atomic_store(failed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    gave_up = true;
                    break;
                }
            }
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc += __longlong_as_double((long long)(((a[c] & 0xffffffffull) << 32) | (b[c] & 0xffffffffull)));
            acc = wave_sum_f64(acc);
            if (lane == 0) total = gave_up ? -1.0 : acc;
        }
        __syncthreads();
        const double sum = total;
        __syncthreads();
        if (sum < 0.0) break;  // (uniform over the workgroup; the sums are positive)
        mine = 1.0 + 1e-9 * sum + 1e-3 * wg;  // (the next publication depends on the sum)
    }
    if (tid == 0) out[wg] = mine;
}

struct Stat {
    double med, range;
    bool ok;
};
static Stat run_layout(u64 *slots, double *out, unsigned int *failed, int work, int delay, int W, int one_store, int perm,
                       int exchange, int reps, int wide_load = 0) {
    const int iters = 4000;
    int stride = 16 / W;  // granules of 8 bytes per slot
    double ns[16];
    Stat st = {0.0, 0.0, true};
    for (int rep = 0; rep < reps + 1; ++rep) {  // (the first run warms up)
        hipMemset(slots, 0, sizeof(u64) * LSLOTS);
        hipMemset(failed, 0, 4);
        hipEvent_t a, b;
        hipEventCreate(&a);
        hipEventCreate(&b);
        hipEventRecord(a);
        void *args[] = {&slots, (void *)&iters, &out, &failed, &work, &delay, &stride, &one_store, &perm, &exchange, &wide_load};
        const hipError_t err = hipLaunchCooperativeKernel((const void *)k_layout, dim3(LWGS), dim3(THREADS), args, 0, 0);
        if (err != hipSuccess) {
            printf("launch failed: %s\n", hipGetErrorString(err));
            st.ok = false;
            return st;
        }
        hipEventRecord(b);
        hipEventSynchronize(b);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, a, b);
        hipEventDestroy(a);
        hipEventDestroy(b);
        unsigned int f = 0;
        hipMemcpy(&f, failed, 4, hipMemcpyDeviceToHost);
        if (f != 0u) st.ok = false;
        double first = 0.0;
        hipMemcpy(&first, out, 8, hipMemcpyDeviceToHost);
        // workgroup 0 ends at 1 + 1e-9 * (sum of 1 + 1e-3 wg + O(1e-7)): a dropped or doubled slot shows in the 7th digit
        const double want = 1.0 + 1e-9 * (LWGS + 1e-3 * (LWGS - 1) * LWGS / 2.0);
        if (exchange && !(first > want - 1e-13 && first < want + 1e-13 * LWGS)) st.ok = false;
        if (rep > 0) ns[rep - 1] = ms * 1e6 / iters;
    }
    std::sort(ns, ns + reps);
    st.med = reps & 1 ? ns[reps / 2] : 0.5 * (ns[reps / 2 - 1] + ns[reps / 2]);
    st.range = ns[reps - 1] - ns[0];
    return st;
}

static int layout_table() {
    u64 *slots;
    double *out;
    unsigned int *failed;
    hipMalloc(&slots, sizeof(u64) * LSLOTS);
    hipMalloc(&out, LWGS * 8);
    hipMalloc(&failed, 4);
    const int work = 100, reps = 5;  // s_sleep units (64 clocks) of "products" between two exchanges: about 3 us
    const Stat base = run_layout(slots, out, failed, work, 0, 8, 0, 0, 0, reps);
    printf("%d workgroups of %d threads; interval without an exchange (%d sleep units): %.0f ns (range %.0f)\n", LWGS, THREADS,
           work, base.med, base.range);
    printf("us per exchange on top of that: median of %d runs of 4000 exchanges (range max - min)\n", reps);
    const int delays[] = {0, 4, 8, 12, 16, 20, 24, 32};
    printf("%-34s", "W  form        map          delay:");
    for (int d : delays) printf("       %2d      ", d);
    printf("\n");
    int bad = 0;
    for (int W : {8, 4, 2, 1})
        for (int one_store = 0; one_store < 2; ++one_store)
            for (int perm = 0; perm < (W > 1 ? 2 : 1); ++perm) {
                printf("%d  %-10s  %-18s", W, one_store ? "1 x 16 B" : "2 x 8 B", W == 1 ? "-" : perm ? "one XCD per line" : "consecutive ids");
                for (int d : delays) {
                    const Stat s = run_layout(slots, out, failed, work, d, W, one_store, perm, 1, reps);
                    if (!s.ok) ++bad;
                    printf("  %6.3f (%5.3f)%s", (s.med - base.med) * 1e-3, s.range * 1e-3, s.ok ? "" : "!");
                }
                printf("\n");
                fflush(stdout);
            }
    const int fine[] = {12, 13, 14, 15, 16, 17, 18, 19, 20, 22};
    printf("\nfiner scan, consecutive ids; poll: two 8-byte loads per slot or one 16-byte load\n");
    printf("%-34s", "W  form        poll         delay:");
    for (int d : fine) printf("       %2d      ", d);
    printf("\n");
    for (int W : {8, 4})
        for (int one_store = 0; one_store < 2; ++one_store)
            for (int wide = 0; wide < 2; ++wide) {
                printf("%d  %-10s  %-18s", W, one_store ? "1 x 16 B" : "2 x 8 B", wide ? "1 x 16 B" : "2 x 8 B");
                for (int d : fine) {
                    const Stat s = run_layout(slots, out, failed, work, d, W, one_store, 0, 1, reps, wide);
                    if (!s.ok) ++bad;
                    printf("  %6.3f (%5.3f)%s", (s.med - base.med) * 1e-3, s.range * 1e-3, s.ok ? "" : "!");
                }
                printf("\n");
                fflush(stdout);
            }
    if (bad) printf("%d combinations gave up or returned a wrong sum (marked !)\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc < 2 || strcmp(argv[1], "xcd") != 0) return layout_table();
    u64 *flat, *local, *cross;
    float *out;
    int *misplaced, mis = 0;
    hipMalloc(&flat, 2 * WGS * 8);
    hipMalloc(&local, 2 * 8 * 64 * 8);
    hipMalloc(&cross, 2 * 8 * 16 * 8);
    hipMalloc(&out, WGS * 4);
    hipMalloc(&misplaced, 4);
    const int work = 100;  // s_sleep units (64 clocks) of "products" between two exchanges: about 3 us
    const float base = run<3, 0>(flat, local, cross, out, misplaced, work, 0, 0, &mis);
    printf("interval without an exchange (%d sleep units): %.0f ns; workgroups not on XCD blockIdx %% 8: %d of %d\n", work, base, mis, WGS);
    printf("exchange cost = interval - that; delays in sleep units before the first poll of a stage\n");
    for (int d1 : {0, 4, 8, 12, 16, 24})
        printf("flat (512 granules, agent scope), delay %2d:                     %6.0f ns\n", d1,
               run<0, 1>(flat, local, cross, out, misplaced, work, d1, 0, &mis) - base);
    for (int d1 : {0, 4, 8, 12})
        for (int d2 : {0, 4, 8, 12})
            printf("two stages (64 in the XCD's L2, then 8 across), delays %2d, %2d:  %6.0f ns   agent-scope stores in stage 1: %6.0f ns\n",
                   d1, d2, run<1, 1>(flat, local, cross, out, misplaced, work, d1, d2, &mis) - base,
                   run<2, 1>(flat, local, cross, out, misplaced, work, d1, d2, &mis) - base);
    return 0;
}
