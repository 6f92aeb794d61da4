// Ranked hit lists (gfx950): the k most stabilising substitutions of every protein of a packed ddG table, selected on the device
// (tmpnn_select_hits, include/tmpnn.h). Nothing here is floating-point arithmetic: a value is read as its 32 bits, mapped to an
// unsigned integer of the same order, and the rest is an integer sort of distinct 64-bit keys — so the result is unique, has no
// summation order, and a rerun gives identical bits. The translation unit is built with -fno-honor-nans like every kernel file;
// the NaN test is therefore made on the raw bits too.
//
// KEY of candidate (local position p, letter a) with value bits b:
//     high word  ord(b) = b' ^ (b' >> 31 ? 0xffffffff : 0x80000000),  b' = (b == 0x80000000 ? 0 : b)        (-0.0 taken as +0.0)
//     low word   p * 32 + a                                                                                  (p < 8192: 18 bits)
// ord() is the usual order-preserving map of IEEE-754 singles onto unsigned integers (-inf < ... < -0 = +0 < ... < +inf), so ascending
// keys are ascending (value, position, letter). A non-candidate is all ones: no candidate has that key (ord() = 0xffffffff belongs
// to a NaN, and NaNs are not candidates), so padding sorts behind every candidate.
//
// STAGE 1, work item (protein b, block j of HITS_B = 256 residues): the block's 5 120 keys (20 per residue; with ONE_PER_POSITION the
// minimum key of each residue, 256 keys) go to LDS, their k smallest are found there in ascending order (hits_topk) and written to
// slot (offsets[b] >> 8) + b + j of the workspace. Consecutive blocks of a protein take consecutive slots, and slots of different
// proteins never meet: with o = offsets[b] and L the length, (o >> 8) + b + ceil(L / 256) <= ((o + L) >> 8) + b + 1. The last slot
// used is below (T >> 8) + n_proteins.
// STAGE 2, one workgroup per protein: the protein's ceil(L / 256) <= 32 slots are one contiguous run of at most 32 k <= 8 192
// leaders; their k smallest are found the same way (one block: they are sorted already) and decoded; the value is read back from the
// table, so the output holds the table's own bits (a -0.0 stays -0.0).
//
// hits_topk(keys, n, m), m = the power of two >= k: a bitonic sort network cut off where it stops mattering. (1) The network up to
// merge size m sorts the n / m chunks of m keys, ascending and descending in turn. (2) An ascending chunk A followed by a descending
// chunk B is a bitonic sequence, so min(A[i], B[i]) — the first step of its merge — holds the m smallest of the 2 m keys, as a bitonic
// sequence; log2(m) more steps sort it, again ascending and descending in turn. Each round halves the number of live chunks (they stay
// where they are: live chunks sit 2, 4, 8 ... chunks apart) until chunk 0 holds the m smallest keys of all, ascending. For n = 8 192
// that is 36 full steps + about 9 more at m = 256 and 15 + about 7 at m = 32, where the full sort takes 91.
//
// LDS: 8 192 keys x 8 bytes = 64 KB per workgroup of 512 threads. A compare-exchange at distance d (in keys) reads keys[lo] and
// keys[lo + d] with lo = 2 (i & ~(d - 1)) + (i & (d - 1)) for thread i, as 8-byte accesses (ds_read_b64 / ds_write_b64):
//   d >= 32: the 32 lanes of a read group hold 32 consecutive keys = 256 bytes = each of the 64 banks once: conflict-free; the 16
//            lanes of a write group hold 128 consecutive bytes = each of the 32 write banks once: conflict-free;
//   d <  32: a read group's 32 lower keys spread over 64 consecutive keys (512 bytes, two bank rows): 2-way on reads; a write group's
//            16 keys spread over 32 keys when d < 16: 2-way on writes (d = 16: conflict-free writes).
// The min step of (2) reads two runs of consecutive keys a whole number of chunks apart: conflict-free for m >= 32. At m = 256, 30 of
// the 36 steps of (1) and 5 of the 9 steps of every round of (2) have d < 32. Measured: 38-42 % of the LDS cycles of stage 1.
#include <stdint.h>
#include <string.h>

#include "tmpnn_internal.h"
#include "tmpnn_hits.h"              // hkey_t, hits_ord, hits_cx, hits_topk, hits_pow2: shared with tmpnn_variant_hits.hip

#define HITS_MAX_LEN 8192           // the forward's own bound: 32 blocks, 32 * 256 leaders
static_assert(HITS_B * 20 <= HITS_MAX_KEYS && (HITS_MAX_LEN / HITS_B) * HITS_MAX_K <= HITS_MAX_KEYS, "both stages sort in one LDS image");

struct HitsArgs {
    const uint32_t *ddg;            // the table's bits
    int ld;
    const int32_t *S, *offsets;
    int n_proteins;
    int64_t T;
    int k;
    uint32_t cut;                   // ord(cutoff): a candidate has ord(value) <= cut
    int flags;
    hkey_t *ws;                     // [(T >> 8) + n_proteins][k]
    uint32_t *hit_ddg;
    int32_t *hit_pos, *hit_aa, *hit_count;
};

// the protein's rows [t0, t1), clamped into the table whatever the offsets hold
__device__ __forceinline__ void hits_rows(const HitsArgs &a, int b, int64_t &t0, int64_t &t1) {
    t0 = a.offsets[b];
    t1 = a.offsets[b + 1];
    t0 = t0 < 0 ? 0 : t0 > a.T ? a.T : t0;
    t1 = t1 < t0 ? t0 : t1 > a.T ? a.T : t1;
}

__global__ __launch_bounds__(HITS_THREADS) void hits_block_kernel(HitsArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int b = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
    int64_t t0, t1;
    hits_rows(a, b, t0, t1);
    const int64_t L = t1 - t0;
    if (L > HITS_MAX_LEN || (int64_t)j * HITS_B >= L) return;                 // (uniform over the workgroup)
    const int r0 = j * HITS_B, rows = (int)(L - r0 < HITS_B ? L - r0 : HITS_B), cand = rows * 20;
    const bool cys = (a.flags & TMPNN_HITS_INCLUDE_CYS) != 0;
    for (int i = tid; i < cand; i += HITS_THREADS) {
        const int r = i / 20, aa = i - r * 20;
        const int64_t t = t0 + r0 + r;
        const uint32_t s = (uint32_t)a.S[t], v = a.ddg[t * a.ld + aa], o = hits_ord(v);
        const bool ok = s < 20u && (uint32_t)aa != s && (v & 0x7fffffffu) <= 0x7f800000u && (cys || aa != HITS_CYS) && o <= a.cut;
        keys[i] = ok ? ((hkey_t)o << 32) | (uint32_t)((r0 + r) * 32 + aa) : HITS_NONE;
    }
    __syncthreads();
    const int m = hits_pow2(a.k);
    int n;
    if (a.flags & TMPNN_HITS_ONE_PER_POSITION) {                              // the position's best candidate: first minimum = minimum key
        hkey_t best = HITS_NONE;
        if (tid < rows)
            for (int aa = 0; aa < 20; ++aa) {
                const hkey_t x = keys[tid * 20 + aa];
                best = x < best ? x : best;
            }
        __syncthreads();
        n = max(hits_pow2(rows), m);
        if (tid < n) keys[tid] = best;                                        // (n <= 256 < HITS_THREADS; tid >= rows holds HITS_NONE)
    } else {
        n = max(hits_pow2(cand), m);
        for (int i = cand + tid; i < n; i += HITS_THREADS) keys[i] = HITS_NONE;
    }
    __syncthreads();
    hits_topk(keys, n, m);
    hkey_t *out = a.ws + ((t0 >> 8) + b + j) * (int64_t)a.k;
    for (int i = tid; i < a.k; i += HITS_THREADS) out[i] = i < n ? keys[i] : HITS_NONE;
}

__global__ __launch_bounds__(HITS_THREADS) void hits_merge_kernel(HitsArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int b = blockIdx.x, tid = threadIdx.x, k = a.k;
    int64_t t0, t1;
    hits_rows(a, b, t0, t1);
    const int64_t L = t1 - t0;
    const bool served = L <= HITS_MAX_LEN;
    const int nb = served ? (int)((L + HITS_B - 1) / HITS_B) : 0, total = nb * k, n = hits_pow2(total);
    const hkey_t *in = a.ws + ((t0 >> 8) + b) * (int64_t)k;
    for (int i = tid; i < n; i += HITS_THREADS) keys[i] = i < total ? in[i] : HITS_NONE;
    __syncthreads();
    if (nb > 1) hits_topk(keys, n, hits_pow2(k));                             // (n >= 2 k > the power of two >= k)
    const int64_t o = (int64_t)b * k;
    for (int i = tid; i < k; i += HITS_THREADS) {
        const hkey_t x = i < n ? keys[i] : HITS_NONE;
        if (x != HITS_NONE) {
            const uint32_t lo = (uint32_t)x;
            const int p = (int)(lo >> 5), aa = (int)(lo & 31u);
            a.hit_ddg[o + i] = a.ddg[(t0 + p) * a.ld + aa];
            a.hit_pos[o + i] = p;
            a.hit_aa[o + i] = aa;
            const hkey_t next = i + 1 < k && i + 1 < n ? keys[i + 1] : HITS_NONE;
            if (next == HITS_NONE) a.hit_count[b] = i + 1;                    // the last hit: one writer
        } else {
            a.hit_ddg[o + i] = 0x7fc00000u;
            a.hit_pos[o + i] = -1;
            a.hit_aa[o + i] = -1;
            if (i == 0) a.hit_count[b] = served ? 0 : -1;                     // (-1: a protein longer than HITS_MAX_LEN, not served)
        }
    }
}

// ---- the C-ABI entries ---------------------------------------------------------------------------------------------------------
static bool hits_sizes_served(int64_t T, int n_proteins, int k) {
    return T >= 0 && T <= (int64_t)0x7fffffff && n_proteins >= 1 && k >= 1 && k <= HITS_MAX_K;
}
static hkey_t *hits_ws(Carver &c, int64_t T, int n_proteins, int k) { return c.take<hkey_t>((size_t)((T >> 8) + n_proteins) * (size_t)k); }

extern "C" size_t tmpnn_hits_workspace_bytes(int64_t T, int n_proteins, int k) {
    if (!hits_sizes_served(T, n_proteins, k)) return 0;
    Carver c;
    hits_ws(c, T, n_proteins, k);
    return c.used + 256;
}

extern "C" int tmpnn_select_hits(const float *ddg, int ld, const int32_t *S, const int32_t *offsets, int n_proteins, int64_t T, int k,
                                 float cutoff, int flags, float *hit_ddg, int32_t *hit_pos, int32_t *hit_aa, int32_t *hit_count,
                                 void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    if (!ddg || !S || !offsets || !hit_ddg || !hit_pos || !hit_aa || !hit_count || !workspace)
        return tm_set_error(TMPNN_E_INVALID, "select_hits: null pointer");
    if (k < 1 || k > HITS_MAX_K) return tm_set_error(TMPNN_E_INVALID, "select_hits: k=%d outside [1, %d]", k, HITS_MAX_K);
    if (ld < 20) return tm_set_error(TMPNN_E_INVALID, "select_hits: ld=%d, a ddG table has at least 20 columns", ld);
    if (n_proteins < 0 || T < 0) return tm_set_error(TMPNN_E_INVALID, "select_hits: bad sizes (N=%d, T=%lld)", n_proteins, (long long)T);
    if (flags & ~(TMPNN_HITS_INCLUDE_CYS | TMPNN_HITS_ONE_PER_POSITION))
        return tm_set_error(TMPNN_E_INVALID, "select_hits: unknown flag bits 0x%x", (unsigned)flags);
    uint32_t cb;
    memcpy(&cb, &cutoff, 4);
    if ((cb & 0x7fffffffu) > 0x7f800000u) return tm_set_error(TMPNN_E_INVALID, "select_hits: the cutoff is NaN (+inf removes no candidate)");
    if (n_proteins == 0) return TMPNN_OK;
    if (T > (int64_t)0x7fffffff)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "select_hits: T=%lld rows exceed the int32 offsets", (long long)T);
    Carver c(workspace, true);
    hkey_t *ws = hits_ws(c, T, n_proteins, k);
    if (c.used > workspace_bytes)
        return tm_set_error(TMPNN_E_WORKSPACE, "select_hits: workspace %zu < %zu bytes", workspace_bytes, tmpnn_hits_workspace_bytes(T, n_proteins, k));
    const HitsArgs a{(const uint32_t *)ddg, ld, S, offsets, n_proteins, T, k, hits_ord(cb), flags, ws,
                     (uint32_t *)hit_ddg, hit_pos, hit_aa, hit_count};
    hipStream_t st = (hipStream_t)stream;
    tm_prof_begin("hits_block", st);
    hipLaunchKernelGGL(hits_block_kernel, dim3((unsigned)n_proteins, HITS_MAX_LEN / HITS_B), dim3(HITS_THREADS), 0, st, a);
    tm_prof_end(st);
    if (int rc = tm_check_launch("hits_block_kernel")) return rc;
    tm_prof_begin("hits_merge", st);
    hipLaunchKernelGGL(hits_merge_kernel, dim3((unsigned)n_proteins), dim3(HITS_THREADS), 0, st, a);
    tm_prof_end(st);
    return tm_check_launch("hits_merge_kernel");
}
