// Bootstrap confidence intervals of the benchmark metrics (gfx950): B resamples with replacement of a table of N (measured ddG,
// M predictions) rows, and per resample and prediction column r2, mse, rmse, spearman and pearson (tmpnn_bootstrap_metrics,
// include/tmpnn.h). No resample is sorted: a resample only re-weights the distinct values of a column, so with gid = the dense rank
// of every row's value among the column's distinct values (made once per dataset) the tie-averaged ranks inside a resample follow from
// ONE histogram over the tie groups and ONE prefix sum:
//     cnt[g] = draws of group g,  P = inclusive prefix sum,  X[g] = P[g - 1] + P[g] + 1 = twice the average rank of group g
// and the rank sums Sxy, Sxx, Syy are exact integers (X <= 2 N + 1, a sum <= 4 N^3 < 2^63 up to N = 2^20). Spearman comes from those
// integers, and whether a column is constant inside a resample is decided on them (Sxx == N (N + 1)^2), never on a rounded float sum.
//
// ONE LAUNCH, one workgroup of 1024 threads per resample, a persistent grid that loops when B exceeds it. Per resample:
//   truth pass     every draw i = idx[b, d] is range-checked, then gid[0, i] is range-checked and counted (integer atomics: the result
//                  has no order); the same pass sums the measured values in float64
//   scan           tiles of 4096 bins, a uint4 per thread, wavefront shuffles + one LDS word per wavefront; it leaves X in place of cnt
//                  and returns sum cnt[g] X[g]^2 (= the sum of X^2 over the draws)
//   per column m   the same two steps on the column's own bins (the truth's X is kept for all M columns), then one pass over the draws
//                  for Sxy and the centred float64 sums
// FORMS: the two bin arrays live in LDS (N <= BOOT_LDS_N, dynamic LDS sized by N, above 64 KB with the function attribute) or in the
// caller's workspace (any N, BOOT_WS_GRID slots); one template, so both forms run the same operations in the same order.
// FLOAT ORDER (the contract): thread t takes the draws t, t + 1024, ... in ascending order into its own float64 accumulators; a
// wavefront folds them by shuffles at distances 32, 16, .. 1; thread 0 adds the 16 wavefront sums in ascending order. Contraction is
// off, so each of these is one rounding in both forms. No float atomics.
// SAFETY: an index is compared (unsigned) with N before it addresses anything, in every pass. A resample with a bad idx entry gets
// status -1, one that meets a bad gid entry -2; either writes nothing else: results are held in LDS until every column is through.
#include <stdint.h>

#include "tmpnn_internal.h"

#pragma clang fp contract(off)

#define BOOT_THREADS 1024
#define BOOT_WAVES (BOOT_THREADS / 64)
#define BOOT_LDS_N 16384            // two u32 arrays of it: 128 KB of the 160 KB
#define BOOT_MAX_N (1 << 20)        // 4 N^3 < 2^63
#define BOOT_MAX_B (1 << 20)
#define BOOT_MAX_M 8
#define BOOT_WS_GRID 256            // workgroups (= workspace slots) of the workspace form
#define BOOT_FORCE_WS 1             // flags bit 0
#define BOOT_NSUM 4                 // centred float64 sums per column

struct BootArgs {
    const float *values;            // [C, N]
    const int32_t *gid;             // [C, N]
    const int32_t *idx;             // [B, N]
    int C, N, B, npad;              // npad: N rounded up to 4
    double *metrics;                // [B, M, 5]
    int64_t *ranks;                 // [B, M, 3]
    int32_t *status;                // [B]
    uint32_t *ws;                   // workspace form: [grid, 2, npad]
};

__device__ __forceinline__ double boot_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the count a histogram left: LDS as it is; global through the device-scope path the atomics took
template <bool LDS> __device__ __forceinline__ uint32_t boot_cnt(const uint32_t *p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class T> __device__ __forceinline__ T boot_wave_fold(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// bins [0, npad) of h: counts in, X out; -> this thread's part of sum cnt X^2. Two barriers per tile, uniform trip count.
template <bool LDS> __device__ __forceinline__ uint64_t boot_scan(uint32_t *h, int npad, uint32_t *wsum) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    uint64_t sq = 0;
    for (int base = 0; base < npad; base += 4 * BOOT_THREADS) {
        const int e = base + 4 * tid;
        uint32_t c[4] = {0, 0, 0, 0};
        if (e < npad) {
            if (LDS) {
                const uint4 v = *(const uint4 *)(h + e);
                c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k] = boot_cnt<false>(h + e + k);
            }
        }
        const uint32_t s = c[0] + c[1] + c[2] + c[3];
        uint32_t incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BOOT_WAVES; ++w) {
            const uint32_t v = wsum[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        uint32_t p = carry + before + incl - s;            // P of the bin in front of this thread's four
        if (e < npad) {
            uint32_t x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t q = p + c[k];
                x[k] = p + q + 1u;
                sq += (uint64_t)c[k] * ((uint64_t)x[k] * (uint64_t)x[k]);
                p = q;
            }
            *(uint4 *)(h + e) = make_uint4(x[0], x[1], x[2], x[3]);
        }
        carry += total;
        __syncthreads();
    }
    return sq;
}

struct BootShared {
    uint32_t wsum[BOOT_WAVES];
    int64_t red_i[2][BOOT_WAVES];
    double red_d[BOOT_NSUM][BOOT_WAVES];
    int64_t out_i[2];
    double out_d[BOOT_NSUM];
    int flag;
    int64_t res_i[BOOT_MAX_M][3];
    double res_d[BOOT_MAX_M][5];
};

// fold ni integers and nd doubles over the workgroup in the fixed order; every thread gets the results in sh.out_*
template <int NI, int ND> __device__ __forceinline__ void boot_reduce(BootShared &sh, int64_t *vi, double *vd) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int64_t v = boot_wave_fold<long long>((long long)vi[k]);
        if (lane == 0) sh.red_i[k][wave] = v;
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) {
        const double v = boot_wave_fold<double>(vd[k]);
        if (lane == 0) sh.red_d[k][wave] = v;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            int64_t s = sh.red_i[k][0];
            for (int w = 1; w < BOOT_WAVES; ++w) s += sh.red_i[k][w];
            sh.out_i[k] = s;
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            double s = sh.red_d[k][0];
            for (int w = 1; w < BOOT_WAVES; ++w) s = s + sh.red_d[k][w];
            sh.out_d[k] = s;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NI; ++k) vi[k] = sh.out_i[k];
#pragma unroll
    for (int k = 0; k < ND; ++k) vd[k] = sh.out_d[k];
    __syncthreads();                                       // out_* and red_* are free again
}

// zero the bins, count the draws' groups of one column, sum the column's values over the draws. first: the draws themselves are
// checked here (flag bit 0); a gid outside [0, N) sets flag bit 1. -> the sum, on every thread.
template <bool LDS> __device__ __forceinline__ double boot_count(const BootArgs &a, BootShared &sh, const int32_t *row, const int32_t *gid,
                                                                 const float *val, uint32_t *h, bool first) {
    const int tid = threadIdx.x;
    const uint32_t N = (uint32_t)a.N;
    for (int e = tid; e < a.npad; e += BOOT_THREADS) h[e] = 0u;
    __syncthreads();
    double s = 0.0;
    int bad = 0;
    for (int d = tid; d < a.N; d += BOOT_THREADS) {
        const uint32_t i = (uint32_t)row[d];
        if (i >= N) {
            bad |= 1;
            continue;
        }
        const uint32_t g = (uint32_t)gid[i];
        if (g >= N) {
            bad |= 2;
            continue;
        }
        atomicAdd(h + g, 1u);
        s = s + (double)val[i];
    }
    if (bad) atomicOr(&sh.flag, first ? bad : (bad & 2));
    int64_t none[1];
    double vd[1] = {s};
    boot_reduce<0, 1>(sh, none, vd);                       // (its first barrier also closes the histogram and the flag)
    return vd[0];
}

template <bool LDS> __global__ __launch_bounds__(BOOT_THREADS) void boot_kernel(BootArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t boot_lds[];
    __shared__ BootShared sh;
    const int tid = threadIdx.x, M = a.C - 1;
    const uint32_t N = (uint32_t)a.N;
    uint32_t *const h0 = LDS ? boot_lds : a.ws + (size_t)blockIdx.x * 2 * (size_t)a.npad;
    uint32_t *const hm = h0 + a.npad;
    const double fn = (double)a.N;
    const int64_t base = (int64_t)a.N * ((int64_t)a.N + 1) * ((int64_t)a.N + 1);

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int32_t *row = a.idx + (size_t)b * (size_t)a.N;
        if (tid == 0) sh.flag = 0;
        __syncthreads();
        const double sum_t = boot_count<LDS>(a, sh, row, a.gid, a.values, h0, true);
        int flag = sh.flag;                                // (uniform: read behind boot_reduce's barriers)
        int64_t Syy = 0;
        double mt = 0.0;
        if (!flag) {
            int64_t vi[1] = {(int64_t)boot_scan<LDS>(h0, a.npad, sh.wsum)};
            double none[1];
            boot_reduce<1, 0>(sh, vi, none);
            Syy = vi[0];
            mt = sum_t / fn;
        }
        for (int m = 0; m < M && !flag; ++m) {
            const int32_t *gm = a.gid + (size_t)(m + 1) * (size_t)a.N;
            const float *vm = a.values + (size_t)(m + 1) * (size_t)a.N;
            const double sum_p = boot_count<LDS>(a, sh, row, gm, vm, hm, false);
            flag = sh.flag;
            if (flag) break;
            int64_t vi[2] = {(int64_t)boot_scan<LDS>(hm, a.npad, sh.wsum), 0};
            const double mp = sum_p / fn;
            double vd[BOOT_NSUM] = {0.0, 0.0, 0.0, 0.0};   // sum pc^2, tc^2, pc tc, (p - t)^2
            for (int d = tid; d < a.N; d += BOOT_THREADS) {
                const uint32_t i = (uint32_t)row[d];
                if (i >= N) continue;
                const uint32_t g0 = (uint32_t)a.gid[i], g1 = (uint32_t)gm[i];
                if (g0 >= N || g1 >= N) continue;
                vi[1] += (int64_t)((uint64_t)hm[g1] * (uint64_t)h0[g0]);
                const double t = (double)a.values[i], p = (double)vm[i];
                const double pc = p - mp, tc = t - mt, e = p - t;
                vd[0] = vd[0] + pc * pc;
                vd[1] = vd[1] + tc * tc;
                vd[2] = vd[2] + pc * tc;
                vd[3] = vd[3] + e * e;
            }
            boot_reduce<2, BOOT_NSUM>(sh, vi, vd);
            if (tid == 0) {
                const int64_t Sxx = vi[0], Sxy = vi[1];
                const bool x_const = Sxx == base, y_const = Syy == base;
                const double mse = vd[3] / fn;
                sh.res_i[m][0] = Sxy;
                sh.res_i[m][1] = Sxx;
                sh.res_i[m][2] = Syy;
                sh.res_d[m][0] = y_const ? boot_nan() : 1.0 - vd[3] / vd[1];
                sh.res_d[m][1] = mse;
                sh.res_d[m][2] = sqrt(mse);
                sh.res_d[m][3] = (x_const || y_const) ? boot_nan()
                                                      : (double)(Sxy - base) / (sqrt((double)(Sxx - base)) * sqrt((double)(Syy - base)));
                sh.res_d[m][4] = (x_const || y_const) ? boot_nan() : vd[2] / sqrt(vd[0] * vd[1]);
            }
        }
        __syncthreads();
        if (tid == 0) a.status[b] = (flag & 1) ? -1 : (flag & 2) ? -2 : 0;
        if (!flag && tid < M * 8) {
            const int m = tid >> 3, k = tid & 7;
            if (k < 5) a.metrics[((size_t)b * M + m) * 5 + k] = sh.res_d[m][k];
            else a.ranks[((size_t)b * M + m) * 3 + (k - 5)] = sh.res_i[m][k - 5];
        }
        __syncthreads();                                   // res_* and flag are free again
    }
}

// ---- the C-ABI entries -----------------------------------------------------------------------------------------------------------
static bool boot_sizes_served(int C, int64_t N, int64_t B) {
    return C >= 2 && C <= BOOT_MAX_M + 1 && N >= 0 && B >= 0 && N <= BOOT_MAX_N && B <= BOOT_MAX_B;
}
static bool boot_lds_form(int64_t N, int flags) { return N <= BOOT_LDS_N && !(flags & BOOT_FORCE_WS); }
static int boot_npad(int64_t N) { return (int)((N + 3) & ~(int64_t)3); }
static int boot_ws_grid(int64_t B) { return (int)(B < BOOT_WS_GRID ? B : BOOT_WS_GRID); }
static uint32_t *boot_ws(Carver &c, int64_t N, int64_t B) { return c.take<uint32_t>((size_t)boot_ws_grid(B) * 2 * (size_t)boot_npad(N)); }

extern "C" size_t tmpnn_bootstrap_workspace_bytes(int C, int64_t N, int64_t B, int flags) {
    if (!boot_sizes_served(C, N, B) || (flags & ~BOOT_FORCE_WS) || N == 0 || B == 0 || boot_lds_form(N, flags)) return 0;
    Carver c;
    boot_ws(c, N, B);
    return c.used + 256;
}

extern "C" int tmpnn_bootstrap_metrics(const float *values, const int32_t *gid, int C, int64_t N, const int32_t *idx, int64_t B,
                                       double *metrics, int64_t *ranks, int32_t *status, void *workspace, size_t workspace_bytes,
                                       int flags, tmpnn_stream_t stream) {
    if (N < 0 || B < 0) return tm_set_error(TMPNN_E_INVALID, "bootstrap_metrics: bad sizes (N=%lld, B=%lld)", (long long)N, (long long)B);
    if (C < 2 || C > BOOT_MAX_M + 1)
        return tm_set_error(TMPNN_E_INVALID, "bootstrap_metrics: C=%d columns, the measured one and 1 to %d predictions are served", C, BOOT_MAX_M);
    if (flags & ~BOOT_FORCE_WS) return tm_set_error(TMPNN_E_INVALID, "bootstrap_metrics: unknown flag bits 0x%x", flags);
    if (N > BOOT_MAX_N) return tm_set_error(TMPNN_E_UNSUPPORTED, "bootstrap_metrics: N=%lld exceeds %d (4 N^3 < 2^63)", (long long)N, BOOT_MAX_N);
    if (B > BOOT_MAX_B) return tm_set_error(TMPNN_E_UNSUPPORTED, "bootstrap_metrics: B=%lld exceeds %d resamples per call", (long long)B, BOOT_MAX_B);
    if (N == 0 || B == 0) return TMPNN_OK;
    if (!values || !gid || !idx || !metrics || !ranks || !status) return tm_set_error(TMPNN_E_INVALID, "bootstrap_metrics: null pointer");
    const bool lds = boot_lds_form(N, flags);
    uint32_t *ws = nullptr;
    if (!lds) {
        if (!workspace) return tm_set_error(TMPNN_E_INVALID, "bootstrap_metrics: null pointer (the workspace form needs a workspace)");
        Carver c(workspace, true);
        ws = boot_ws(c, N, B);
        if (c.used > workspace_bytes)
            return tm_set_error(TMPNN_E_WORKSPACE, "bootstrap_metrics: workspace %zu < %zu bytes", workspace_bytes,
                                tmpnn_bootstrap_workspace_bytes(C, N, B, flags));
    }
    const BootArgs a{values, gid, idx, C, (int)N, (int)B, boot_npad(N), metrics, ranks, status, ws};
    hipStream_t st = (hipStream_t)stream;
    if (lds) {
        const size_t bytes = (size_t)2 * a.npad * sizeof(uint32_t);
        // the attribute is per device; set once per device, not per call
        static bool raised[64] = {false};
        int dev = 0;
        if (bytes > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !raised[dev]) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(boot_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      2 * BOOT_LDS_N * (int)sizeof(uint32_t));
            raised[dev] = true;
        }
        // small N: several workgroups share a CU (LDS per workgroup is sized by N; 2048 threads per CU)
        const int64_t cap = (int64_t)tm_num_cus() * 2;
        tm_prof_begin("bootstrap", st);
        hipLaunchKernelGGL(boot_kernel<true>, dim3((unsigned)(B < cap ? B : cap)), dim3(BOOT_THREADS), bytes, st, a);
    } else {
        tm_prof_begin("bootstrap_ws", st);
        hipLaunchKernelGGL(boot_kernel<false>, dim3((unsigned)boot_ws_grid(B)), dim3(BOOT_THREADS), 0, st, a);
    }
    tm_prof_end(st);
    return tm_check_launch("boot_kernel");
}
