// Per-site-pair maps over variant tables (gfx950): for every (state row, position q) the best value base[v] + ddg[v, q, b], the most
// negative and the most positive epistasis e = ddg[v, q, b] - wt[q, b], the sum of |e| and the number of its terms, over the V variant
// tables of one call and over whatever earlier calls left in the caller's state (tmpnn_pair_map, include/tmpnn.h). Double mutants are
// the first user (variant_scan.double_mutant_map): row = the index of the first site p, letter = a, so the state is the [P, L] map of
// every site pair's best double mutant and of its coupling; the [P, 20, L, 20] table never exists.
//
// Float work: ONE fp32 round-to-nearest add for the value, ONE subtract for e, and the adds of |e|; no multiply, so nothing to contract.
// This file is built WITHOUT -fno-honor-nans (build.py FILE_FLAGS), as tmpnn_variant_hits.hip is: inf - inf is a NaN that has to be seen.
// The NaN tests are made on the bits all the same.
//
// KEYS of candidate (variant v, position q, letter b), a = letter[v] (include/tmpnn.h has the contract):
//     best     hits_ord(bits(base[v] + ddg[v, q, b])) << 32 | a << 5 | b        the smallest key = the smallest value, then (a, b)
//     eps_lo   hits_ord(bits(e))                      << 32 | a << 5 | b        the smallest key = the most negative e
//     eps_hi   ~hits_ord(bits(e))                     << 32 | a << 5 | b        the smallest key = the largest e, then the smallest (a, b)
// All ones is "none" (a live key's low word is below 1024).
//
// LAUNCH 1, ceil(V L / 256) workgroups of 256 threads over the V L table rows taken as one flat list (a tile may span two variants):
// the tile's 256 x 20 table entries and the matching rows of wt are staged in LDS with lane-contiguous global reads (a row is 84 bytes at
// ld = 21: one lane per row would touch 42 lines per load instruction), at a row stride of 21 words, which keeps the per-thread row reads
// free of bank conflicts. Thread r then owns row r: its three keys, the sum of |e| in ascending b from +0.0, and the count go to the
// workspace as five arrays (lane-contiguous stores). Without TMPNN_PMAP_CONTINUE the same launch first empties the whole state, in a
// grid-stride loop (launch 2 follows it on the stream).
// LAUNCH 2, one thread per (v, q): the thread of a run's first variant (v = 0 or row[v - 1] != row[v]) folds the run's records in
// ascending v into state entry row[v] L + q: minima of the keys, sum = sum + inner, count += count. Runs of one row are contiguous (the
// caller's promise), so every state entry has one writer. No atomics.
#include <stdint.h>

#include "tmpnn_internal.h"
#include "tmpnn_hits.h"

#define PMAP_THREADS 256
#define PMAP_LDW 21                 // LDS row stride in words: odd, so 64 lanes reading column b of 64 rows hit 64 banks
#define PMAP_MAX_LEN 2048
#define PMAP_RESET_GROUPS 2048      // most workgroups a launch adds for the reset of a state that is larger than the call's tables

struct PMapArgs {
    const float *ddg;               // [V, L, ld]
    int ld;
    const int32_t *S_var;           // [V, L]
    const float *base;              // [V]
    const int32_t *row, *letter, *skip;   // [V]
    const float *wt;                // [L, ld_wt]
    int ld_wt;
    int V, L, R;
    int64_t N, RL;                  // V L table rows, R L state entries (both < 2^31)
    int flags;
    hkey_t *best, *lo, *hi;         // the state, [R L] each
    float *sum;
    int32_t *count;
    hkey_t *w_best, *w_lo, *w_hi;   // the workspace, [V L] each
    float *w_sum;
    int32_t *w_count;
};

__device__ __forceinline__ bool pmap_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

__global__ __launch_bounds__(PMAP_THREADS) void pmap_rows_kernel(PMapArgs a) {
    __shared__ float t_ddg[PMAP_THREADS * PMAP_LDW], t_wt[PMAP_THREADS * PMAP_LDW];
    const int tid = threadIdx.x;
    if (!(a.flags & TMPNN_PMAP_CONTINUE)) {
        for (int64_t i = (int64_t)blockIdx.x * PMAP_THREADS + tid; i < a.RL; i += (int64_t)gridDim.x * PMAP_THREADS) {
            a.best[i] = HITS_NONE;
            a.lo[i] = HITS_NONE;
            a.hi[i] = HITS_NONE;
            a.sum[i] = 0.0f;
            a.count[i] = 0;
        }
    }
    const int64_t row0 = (int64_t)blockIdx.x * PMAP_THREADS;
    if (row0 >= a.N) return;                                                  // (uniform: a workgroup that only resets)
    const int rows = a.N - row0 < PMAP_THREADS ? (int)(a.N - row0) : PMAP_THREADS;
    const int q0 = (int)(row0 % a.L);
    for (int i = tid; i < rows * 20; i += PMAP_THREADS) {
        const int r = i / 20, b = i - r * 20;
        t_ddg[r * PMAP_LDW + b] = a.ddg[(row0 + r) * a.ld + b];
        t_wt[r * PMAP_LDW + b] = a.wt[(int64_t)((q0 + r) % a.L) * a.ld_wt + b];
    }
    __syncthreads();
    if (tid >= rows) return;
    const int64_t g = row0 + tid;
    const int v = (int)(g / a.L), q = (int)(g - (int64_t)v * a.L);
    const int let = a.letter[v], rw = a.row[v], skip = a.skip[v];
    const uint32_t s = (uint32_t)a.S_var[g];
    const float base = a.base[v];
    const bool cys = (a.flags & TMPNN_PMAP_INCLUDE_CYS) != 0;
    const bool live = rw >= 0 && rw < a.R && let >= 0 && let < 20 && s < 20u && ((a.flags & TMPNN_PMAP_UPPER) ? q > skip : q != skip);
    hkey_t k_best = HITS_NONE, k_lo = HITS_NONE, k_hi = HITS_NONE;
    float inner = 0.0f;
    int n = 0;
    if (live) {
        const float *d = t_ddg + tid * PMAP_LDW, *w = t_wt + tid * PMAP_LDW;
#pragma unroll
        for (int b = 0; b < 20; ++b) {                                        // ascending b: the order of the |e| sum is the contract
            if ((uint32_t)b == s || (!cys && b == HITS_CYS)) continue;
            const uint32_t low = (uint32_t)let << 5 | (uint32_t)b;
            const float x = d[b];
            const uint32_t sb = __float_as_uint(__fadd_rn(base, x));
            if (!pmap_is_nan(sb)) {
                const hkey_t k = ((hkey_t)hits_ord(sb) << 32) | low;
                k_best = k < k_best ? k : k_best;
            }
            const float e = __fsub_rn(x, w[b]);
            const uint32_t eb = __float_as_uint(e);
            if (!pmap_is_nan(eb)) {
                const uint32_t o = hits_ord(eb);
                const hkey_t kl = ((hkey_t)o << 32) | low, kh = ((hkey_t)~o << 32) | low;
                k_lo = kl < k_lo ? kl : k_lo;
                k_hi = kh < k_hi ? kh : k_hi;
                inner = __fadd_rn(inner, __uint_as_float(eb & 0x7fffffffu));
                ++n;
            }
        }
    }
    a.w_best[g] = k_best;
    a.w_lo[g] = k_lo;
    a.w_hi[g] = k_hi;
    a.w_sum[g] = inner;
    a.w_count[g] = n;
}

__global__ __launch_bounds__(PMAP_THREADS) void pmap_fold_kernel(PMapArgs a) {
    const int64_t g = (int64_t)blockIdx.x * PMAP_THREADS + threadIdx.x;
    if (g >= a.N) return;
    const int v = (int)(g / a.L), q = (int)(g - (int64_t)v * a.L);
    const int rw = a.row[v];
    if ((v > 0 && a.row[v - 1] == rw) || rw < 0 || rw >= a.R) return;         // not the head of a run, or a run that names no state row
    const int64_t at = (int64_t)rw * a.L + q;
    hkey_t k_best = a.best[at], k_lo = a.lo[at], k_hi = a.hi[at];
    float sum = a.sum[at];
    int n = a.count[at];
    for (int u = v; u < a.V && a.row[u] == rw; ++u) {                         // ascending v: the order of the sum is the contract
        const int64_t i = (int64_t)u * a.L + q;
        const hkey_t x = a.w_best[i], y = a.w_lo[i], z = a.w_hi[i];
        k_best = x < k_best ? x : k_best;
        k_lo = y < k_lo ? y : k_lo;
        k_hi = z < k_hi ? z : k_hi;
        sum = __fadd_rn(sum, a.w_sum[i]);
        n += a.w_count[i];
    }
    a.best[at] = k_best;
    a.lo[at] = k_lo;
    a.hi[at] = k_hi;
    a.sum[at] = sum;
    a.count[at] = n;
}

// ---- the C-ABI entries ---------------------------------------------------------------------------------------------------------
static bool pmap_fits(int64_t n, int64_t L) { return L == 0 || n <= (int64_t)0x7fffffff / L; }
static bool pmap_sizes_served(int64_t V, int64_t L) { return V >= 0 && L >= 0 && L <= PMAP_MAX_LEN && pmap_fits(V, L); }

struct PMapWs {
    hkey_t *best, *lo, *hi;
    float *sum;
    int32_t *count;
};
static PMapWs pmap_ws(Carver &c, int64_t V, int64_t L) {
    const size_t n = (size_t)(V * L);
    PMapWs w;
    w.best = c.take<hkey_t>(n);
    w.lo = c.take<hkey_t>(n);
    w.hi = c.take<hkey_t>(n);
    w.sum = c.take<float>(n);
    w.count = c.take<int32_t>(n);
    return w;
}

extern "C" size_t tmpnn_pair_map_workspace_bytes(int64_t V, int64_t L) {
    if (!pmap_sizes_served(V, L)) return 0;
    Carver c;
    pmap_ws(c, V, L);
    return c.used + 256;
}

extern "C" int tmpnn_pair_map(const float *ddg, int ld, const int32_t *S_var, const float *base, const int32_t *row, const int32_t *letter,
                              const int32_t *skip, const float *wt, int ld_wt, int64_t V, int64_t L, int64_t R, int flags, uint64_t *best,
                              uint64_t *eps_lo, uint64_t *eps_hi, float *eps_abs_sum, int32_t *count, void *workspace,
                              size_t workspace_bytes, tmpnn_stream_t stream) {
    if (V < 0 || L < 0 || R < 0)
        return tm_set_error(TMPNN_E_INVALID, "pair_map: bad sizes (V=%lld, L=%lld, R=%lld)", (long long)V, (long long)L, (long long)R);
    const bool empty = V == 0 || L == 0;                                      // (an empty table has no address: the inputs are not read)
    const bool no_state = R == 0 || L == 0;                                   // (nor has an empty state)
    if ((!empty && (!ddg || !S_var || !base || !row || !letter || !skip || !wt)) ||
        (!no_state && (!best || !eps_lo || !eps_hi || !eps_abs_sum || !count)) || !workspace)
        return tm_set_error(TMPNN_E_INVALID, "pair_map: null pointer");
    if (ld < 20 || ld_wt < 20)
        return tm_set_error(TMPNN_E_INVALID, "pair_map: ld=%d, ld_wt=%d, a ddG table has at least 20 columns", ld, ld_wt);
    if (flags & ~(TMPNN_PMAP_INCLUDE_CYS | TMPNN_PMAP_UPPER | TMPNN_PMAP_CONTINUE))
        return tm_set_error(TMPNN_E_INVALID, "pair_map: unknown flag bits 0x%x", (unsigned)flags);
    if (L > PMAP_MAX_LEN) return tm_set_error(TMPNN_E_UNSUPPORTED, "pair_map: L=%lld exceeds %d", (long long)L, PMAP_MAX_LEN);
    if (!pmap_fits(V, L) || !pmap_fits(R, L))
        return tm_set_error(TMPNN_E_UNSUPPORTED, "pair_map: V L = %lld x %lld table rows or R L = %lld x %lld state entries exceed 2^31 - 1",
                            (long long)V, (long long)L, (long long)R, (long long)L);
    Carver c(workspace, true);
    const PMapWs w = pmap_ws(c, V, L);
    if (c.used > workspace_bytes)
        return tm_set_error(TMPNN_E_WORKSPACE, "pair_map: workspace %zu < %zu bytes", workspace_bytes, tmpnn_pair_map_workspace_bytes(V, L));
    if (no_state) return TMPNN_OK;                                            // nothing to reset, nothing to fold into
    const int64_t N = V * L, RL = R * L;
    const PMapArgs a{ddg, ld, S_var, base, row, letter, skip, wt, ld_wt, (int)V, (int)L, (int)R, N, RL, flags, (hkey_t *)best, (hkey_t *)eps_lo,
                     (hkey_t *)eps_hi, eps_abs_sum, count, w.best, w.lo, w.hi, w.sum, w.count};
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (N + PMAP_THREADS - 1) / PMAP_THREADS;              // (<= 2^23)
    int64_t groups = tiles;
    if (!(flags & TMPNN_PMAP_CONTINUE)) {                                     // the reset rides launch 1; a state beyond the tables adds workgroups
        const int64_t want = (RL + PMAP_THREADS - 1) / PMAP_THREADS;
        const int64_t more = want < PMAP_RESET_GROUPS ? want : PMAP_RESET_GROUPS;
        groups = groups > more ? groups : more;
    }
    if (groups > 0) {
        tm_prof_begin("pmap_rows", st);
        hipLaunchKernelGGL(pmap_rows_kernel, dim3((unsigned)groups), dim3(PMAP_THREADS), 0, st, a);
        tm_prof_end(st);
        if (int rc = tm_check_launch("pmap_rows_kernel")) return rc;
    }
    if (tiles > 0) {
        tm_prof_begin("pmap_fold", st);
        hipLaunchKernelGGL(pmap_fold_kernel, dim3((unsigned)tiles), dim3(PMAP_THREADS), 0, st, a);
        tm_prof_end(st);
        return tm_check_launch("pmap_fold_kernel");
    }
    return TMPNN_OK;
}
