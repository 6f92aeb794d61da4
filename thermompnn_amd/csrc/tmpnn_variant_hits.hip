// Streaming hit lists over variant tables (gfx950): the k smallest values base[v] + ddg[v, q, b] over the V variant tables of one call
// and over whatever earlier calls left in the caller's state (tmpnn_select_variant_hits, include/tmpnn.h). Double mutants are the first
// user (variant_scan.double_mutant_hits): a chunk of single-substitution backgrounds is decoded, reduced to k keys while it is hot, and
// the k keys are carried to the next chunk; the [P, 20, L, 20] table never exists.
//
// The value is ONE fp32 round-to-nearest add, the only float operation here; everything after it is tmpnn_hits.hip's integer sort of
// distinct 64-bit keys. This file is built WITHOUT -fno-honor-nans (build.py FILE_FLAGS): +inf + -inf is a NaN that has to be seen, and
// under that flag the sum would be poison to the compiler. The NaN test is made on the sum's bits all the same.
//
// KEY of candidate (variant v, position q, letter b) with sum bits s:
//     high word  hits_ord(s)                                                                   (-0.0 taken as +0.0)
//     low word   tag[v] << 16 | q << 5 | b                                                     (tag < 65536, q < 2048, b < 32)
// Ascending keys are ascending (value, tag, position, letter); all ones is "none" (hits_ord = 0xffffffff belongs to a NaN). With distinct
// tags over all calls of one selection every key is distinct, so the k smallest are unique whatever the cut into calls.
//
// STAGE 1, W = min(items, 8192 / m - 1) workgroups, m = the power of two >= k, an item = (variant, block of 256 residues): workgroup w
// takes items w, w + W, ... Its LDS image holds its running m leaders in front (all ones at the start), the item's <= 5 120 new keys
// behind them and padding up to a power of two (m + 5 120 <= 5 376 <= 8 192); hits_topk leaves the m smallest in front again. After its
// last item it writes its first k leaders to slot w of the workspace.
// STAGE 2, one workgroup: the W k leaders and, with TMPNN_VHITS_CONTINUE, the state's k keys — at most (8192 / m) k <= 8 192 keys — are
// sorted the same way; the first k go to the state and are decoded (the value from the key: ord is a bijection apart from -0.0).
// No atomics; the result does not depend on W.
#include <stdint.h>
#include <string.h>

#include "tmpnn_internal.h"
#include "tmpnn_hits.h"

#define VHITS_MAX_LEN 2048          // 11 bits of the key's low word
#define VHITS_MAX_TAG 65535
static_assert(HITS_MAX_K + HITS_B * 20 <= HITS_MAX_KEYS, "leaders and one item's keys share the LDS image");

struct VHitsArgs {
    const float *ddg;               // [V, L, ld]
    int ld;
    const int32_t *S_var;           // [V, L]
    const float *base;              // [V]
    const int32_t *tag, *skip;      // [V]
    int V, L, nblk, items;          // nblk = ceil(L / 256), items = V nblk
    int k, W;
    uint32_t cut;                   // ord(cutoff)
    int flags;
    hkey_t *ws;                     // [W][k]
    hkey_t *state;                  // [k]
    uint32_t *hit_ddg;
    int32_t *hit_tag, *hit_pos, *hit_aa, *hit_count;
};

__global__ __launch_bounds__(HITS_THREADS) void vhits_block_kernel(VHitsArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int w = blockIdx.x, tid = threadIdx.x, m = hits_pow2(a.k);
    const bool cys = (a.flags & TMPNN_VHITS_INCLUDE_CYS) != 0, upper = (a.flags & TMPNN_VHITS_UPPER) != 0;
    for (int i = tid; i < m; i += HITS_THREADS) keys[i] = HITS_NONE;
    for (int item = w; item < a.items; item += a.W) {                         // (uniform over the workgroup)
        const int v = item / a.nblk, j = item - v * a.nblk;
        const int r0 = j * HITS_B, rows = a.L - r0 < HITS_B ? a.L - r0 : HITS_B, cand = rows * 20;
        const int tag = a.tag[v], skip = a.skip[v];
        const float base = a.base[v];
        const bool live = tag >= 0 && tag <= VHITS_MAX_TAG;
        const int64_t row0 = (int64_t)v * a.L + r0;
        for (int i = tid; i < cand; i += HITS_THREADS) {
            const int r = i / 20, aa = i - r * 20, q = r0 + r;
            const uint32_t s = (uint32_t)a.S_var[row0 + r];
            const float sum = __fadd_rn(base, a.ddg[(row0 + r) * a.ld + aa]);
            const uint32_t bits = __float_as_uint(sum), o = hits_ord(bits);
            const bool ok = live && s < 20u && (uint32_t)aa != s && (upper ? q > skip : q != skip) && (cys || aa != HITS_CYS) &&
                            (bits & 0x7fffffffu) <= 0x7f800000u && o <= a.cut;
            keys[m + i] = ok ? ((hkey_t)o << 32) | ((uint32_t)tag << 16 | (uint32_t)q << 5 | (uint32_t)aa) : HITS_NONE;
        }
        const int n = hits_pow2(m + cand);                                    // (>= 2 m: cand >= 20 and n is a power of two above m)
        for (int i = m + cand + tid; i < n; i += HITS_THREADS) keys[i] = HITS_NONE;
        __syncthreads();
        hits_topk(keys, n, m);                                                // ends behind a barrier: keys[m ..) may be overwritten
    }
    __syncthreads();
    hkey_t *out = a.ws + (int64_t)w * a.k;
    for (int i = tid; i < a.k; i += HITS_THREADS) out[i] = keys[i];
}

__global__ __launch_bounds__(HITS_THREADS) void vhits_merge_kernel(VHitsArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int tid = threadIdx.x, k = a.k, m = hits_pow2(k);
    const int lead = a.W * k, total = lead + ((a.flags & TMPNN_VHITS_CONTINUE) ? k : 0), n = max(hits_pow2(total), m);
    for (int i = tid; i < n; i += HITS_THREADS) keys[i] = i < lead ? a.ws[i] : i < total ? a.state[i - lead] : HITS_NONE;
    __syncthreads();
    hits_topk(keys, n, m);
    for (int i = tid; i < k; i += HITS_THREADS) {
        const hkey_t x = keys[i];
        a.state[i] = x;
        if (x != HITS_NONE) {
            const uint32_t o = (uint32_t)(x >> 32), lo = (uint32_t)x;
            a.hit_ddg[i] = (o & 0x80000000u) ? o ^ 0x80000000u : ~o;          // hits_ord undone (a -0.0 sum comes back as +0.0)
            a.hit_tag[i] = (int)(lo >> 16);
            a.hit_pos[i] = (int)((lo >> 5) & 2047u);
            a.hit_aa[i] = (int)(lo & 31u);
            if (i + 1 == k || keys[i + 1] == HITS_NONE) a.hit_count[0] = i + 1;   // the last hit: one writer
        } else {
            a.hit_ddg[i] = 0x7fc00000u;
            a.hit_tag[i] = -1;
            a.hit_pos[i] = -1;
            a.hit_aa[i] = -1;
            if (i == 0) a.hit_count[0] = 0;
        }
    }
}

// ---- the C-ABI entries ---------------------------------------------------------------------------------------------------------
static bool vhits_sizes_served(int64_t V, int64_t L, int k) {
    return V >= 0 && L >= 0 && L <= VHITS_MAX_LEN && k >= 1 && k <= HITS_MAX_K && (L == 0 || V <= (int64_t)0x7fffffff / L);
}
static int vhits_pow2_host(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}
static int64_t vhits_items(int64_t V, int64_t L) { return V * ((L + HITS_B - 1) / HITS_B); }
static int vhits_groups(int64_t V, int64_t L, int k) {
    const int64_t items = vhits_items(V, L), most = HITS_MAX_KEYS / vhits_pow2_host(k) - 1;
    return (int)(items < most ? items : most);
}
static hkey_t *vhits_ws(Carver &c, int64_t V, int64_t L, int k) { return c.take<hkey_t>((size_t)vhits_groups(V, L, k) * (size_t)k); }

extern "C" size_t tmpnn_variant_hits_workspace_bytes(int64_t V, int64_t L, int k) {
    if (!vhits_sizes_served(V, L, k)) return 0;
    Carver c;
    vhits_ws(c, V, L, k);
    return c.used + 256;
}

extern "C" int tmpnn_select_variant_hits(const float *ddg, int ld, const int32_t *S_var, const float *base, const int32_t *tag,
                                         const int32_t *skip, int64_t V, int64_t L, int k, float cutoff, int flags, uint64_t *state,
                                         float *hit_ddg, int32_t *hit_tag, int32_t *hit_pos, int32_t *hit_aa, int32_t *hit_count,
                                         void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    if (V < 0 || L < 0) return tm_set_error(TMPNN_E_INVALID, "select_variant_hits: bad sizes (V=%lld, L=%lld)", (long long)V, (long long)L);
    const bool empty = V == 0 || L == 0;                                      // (an empty table has no address: the inputs are not read)
    if ((!empty && (!ddg || !S_var || !base || !tag || !skip)) || !state || !hit_ddg || !hit_tag || !hit_pos || !hit_aa || !hit_count ||
        !workspace)
        return tm_set_error(TMPNN_E_INVALID, "select_variant_hits: null pointer");
    if (k < 1 || k > HITS_MAX_K) return tm_set_error(TMPNN_E_INVALID, "select_variant_hits: k=%d outside [1, %d]", k, HITS_MAX_K);
    if (ld < 20) return tm_set_error(TMPNN_E_INVALID, "select_variant_hits: ld=%d, a ddG table has at least 20 columns", ld);
    if (flags & ~(TMPNN_VHITS_INCLUDE_CYS | TMPNN_VHITS_UPPER | TMPNN_VHITS_CONTINUE))
        return tm_set_error(TMPNN_E_INVALID, "select_variant_hits: unknown flag bits 0x%x", (unsigned)flags);
    uint32_t cb;
    memcpy(&cb, &cutoff, 4);
    if ((cb & 0x7fffffffu) > 0x7f800000u)
        return tm_set_error(TMPNN_E_INVALID, "select_variant_hits: the cutoff is NaN (+inf removes no candidate)");
    if (L > VHITS_MAX_LEN)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "select_variant_hits: L=%lld exceeds %d, the key's 11 position bits", (long long)L, VHITS_MAX_LEN);
    if (!vhits_sizes_served(V, L, k))
        return tm_set_error(TMPNN_E_UNSUPPORTED, "select_variant_hits: V L = %lld x %lld rows exceed 2^31 - 1", (long long)V, (long long)L);
    Carver c(workspace, true);
    hkey_t *ws = vhits_ws(c, V, L, k);
    if (c.used > workspace_bytes)
        return tm_set_error(TMPNN_E_WORKSPACE, "select_variant_hits: workspace %zu < %zu bytes", workspace_bytes,
                            tmpnn_variant_hits_workspace_bytes(V, L, k));
    const int W = vhits_groups(V, L, k);
    const VHitsArgs a{ddg, ld, S_var, base, tag, skip, (int)V, (int)L, (int)((L + HITS_B - 1) / HITS_B), (int)vhits_items(V, L), k, W,
                      hits_ord(cb), flags, ws, (hkey_t *)state, (uint32_t *)hit_ddg, hit_tag, hit_pos, hit_aa, hit_count};
    hipStream_t st = (hipStream_t)stream;
    if (W > 0) {
        tm_prof_begin("vhits_block", st);
        hipLaunchKernelGGL(vhits_block_kernel, dim3((unsigned)W), dim3(HITS_THREADS), 0, st, a);
        tm_prof_end(st);
        if (int rc = tm_check_launch("vhits_block_kernel")) return rc;
    }
    tm_prof_begin("vhits_merge", st);
    hipLaunchKernelGGL(vhits_merge_kernel, dim3(1), dim3(HITS_THREADS), 0, st, a);
    tm_prof_end(st);
    return tm_check_launch("vhits_merge_kernel");
}
