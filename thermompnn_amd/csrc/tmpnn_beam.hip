// One step of a beam search over n-point mutants (gfx950): from the V members of a beam and their freshly decoded variant tables, the k
// best DISTINCT children with their sequence rows, all on the device (tmpnn_beam_step, include/tmpnn.h). A search of order n is n
// decodes plus n steps over one encoded backbone (variant_scan.multi_mutant_search); no table goes to the host, no sequence comes back.
//
// The value of candidate (member v, position q, letter b) is ONE fp32 round-to-nearest add, score[v] + ddg[v, q, b], the only float
// operation here; everything after it is tmpnn_hits.h's integer sort of distinct 64-bit keys. This file is built WITHOUT
// -fno-honor-nans (build.py FILE_FLAGS), as tmpnn_variant_hits.hip is and for the same reason: +inf + -inf is a NaN that has to be seen.
//
// KEY:  hits_ord(sum bits) << 32 | v << 16 | q << 5 | b                                  (v < 65536, q < 2048, b < 32; all ones: none)
// CHILD SET of a candidate: muts[v] (d - 1 words q << 5 | b, ascending, distinct positions) with q << 5 | b inserted in place. Two
// candidates are duplicates when their sets are equal; the result keeps, walking the keys in ascending order, every candidate whose set
// no earlier candidate has, until k are kept.
// THE d-PARENTS LEMMA: the caller promises that live members are distinct sets. A child set of size d has d subsets of size d - 1, so
// at most d members are its parents, and each reaches it by exactly one candidate (the one element it lacks). Among the k d smallest
// keys every set therefore occurs at most d times, so they hold at least k distinct sets or every candidate there is — and a set's
// smallest key lies among them whenever the set is one of the first k. The step never looks beyond the kd = k d <= 256 smallest keys.
//
// STAGE 1 (vhits_block_kernel's shape), W = min(items, 8192 / m - 1) workgroups, m = the power of two >= kd, an item = (member, block
// of 256 residues): a workgroup loops over items w, w + W, ..., keeps its m running leaders in front of its LDS image through
// hits_topk, and leaves kd keys in slot w of the workspace.
// STAGE 2, one workgroup: sorts the W kd leaders, builds the first kd keys' child sets in LDS (behind the keys, 256 x 8 words), marks
// entry i a duplicate when some j < i holds an equal set (equality is an equivalence: no sequential walk), ranks the survivors by a
// prefix count, writes the first k (out_muts, out_score, out_parent, the new substitution into the workspace) and the padding.
// STAGE 3, (kept row, block of 256 residues): out_S[r] = S_var[parent] with q <- b; 20 in padding rows.
// No atomics; the result does not depend on W.
//
// MANY PROTEINS IN ONE STEP (tmpnn_beam_step_each, behind the single-protein entry below): P proteins of a packed axis of T rows, row v
// of the [V, T] inputs holding beam slot v of every protein, so that one decode per round serves the whole pack. The same three stages
// with a protein index in front: stage 1 works on slots (p, w), W = min(V ceil(max_len / 256), 8192 / m - 1) per protein, workgroup
// (p, w) looping over p's OWN items; stage 2 is one workgroup per protein; stage 3 works on (p, kept row, block of 256 rows). The
// grids are capped and every workgroup loops over its slots, so no size of P needs a fourth launch. The offsets live on the device:
// every workgroup of a protein evaluates beam_each_range, the same predicate in 64-bit arithmetic, before it reads a row of p.
#include <stdint.h>
#include <string.h>

#include "tmpnn_internal.h"
#include "tmpnn_hits.h"

#define BEAM_MAX_LEN 2048           // 11 bits of the key's low word
#define BEAM_MAX_V 65536            // 16 bits
#define BEAM_MAX_DEPTH 8
#define BEAM_ROW_THREADS 256
static_assert(HITS_MAX_K + HITS_B * 20 <= HITS_MAX_KEYS, "leaders and one item's keys share the LDS image");
static_assert(HITS_MAX_K * sizeof(hkey_t) + HITS_MAX_K * (BEAM_MAX_DEPTH + 1) * sizeof(int32_t) <= HITS_MAX_KEYS * sizeof(hkey_t),
              "the sorted leaders, their child sets and the survivor flags share the LDS image");

struct BeamArgs {
    const float *ddg;               // [V, L, ld]
    int ld;
    const int32_t *S_var;           // [V, L]
    const float *score;             // [V]
    const int32_t *muts;            // [V, depth - 1]
    const int32_t *allowed;         // [L] or null
    int depth;
    int V, L, nblk, items;          // nblk = ceil(L / 256), items = V nblk
    int k, kd, W;                   // kd = k depth
    uint32_t cut;                   // ord(cutoff)
    int flags;
    hkey_t *ws;                     // [W][kd]
    int32_t *fresh;                 // [k]: the substitution q << 5 | b that row r adds to its parent (-1: padding)
    int32_t *out_muts;              // [k, depth]
    uint32_t *out_score;            // [k]
    int32_t *out_parent, *out_S, *out_count;
};

__global__ __launch_bounds__(HITS_THREADS) void beam_block_kernel(BeamArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int w = blockIdx.x, tid = threadIdx.x, m = hits_pow2(a.kd), nm = a.depth - 1;
    const bool cys = (a.flags & TMPNN_BEAM_INCLUDE_CYS) != 0;
    for (int i = tid; i < m; i += HITS_THREADS) keys[i] = HITS_NONE;
    for (int item = w; item < a.items; item += a.W) {                         // (uniform over the workgroup)
        const int v = item / a.nblk, j = item - v * a.nblk;
        const int r0 = j * HITS_B, rows = a.L - r0 < HITS_B ? a.L - r0 : HITS_B, cand = rows * 20;
        int taken[BEAM_MAX_DEPTH - 1];                                        // the member's positions; a negative word: a dead member
        bool live = true;
#pragma unroll
        for (int c = 0; c < BEAM_MAX_DEPTH - 1; ++c) {
            const int e = c < nm ? a.muts[(int64_t)v * nm + c] : 0;
            live = live && e >= 0;
            taken[c] = c < nm ? e >> 5 : -1;
        }
        const float base = a.score[v];
        const int64_t row0 = (int64_t)v * a.L + r0;
        for (int i = tid; i < cand; i += HITS_THREADS) {
            const int r = i / 20, aa = i - r * 20, q = r0 + r;
            const uint32_t s = (uint32_t)a.S_var[row0 + r];
            const float sum = __fadd_rn(base, a.ddg[(row0 + r) * a.ld + aa]);
            const uint32_t bits = __float_as_uint(sum), o = hits_ord(bits);
            bool ok = live && s < 20u && (uint32_t)aa != s && (cys || aa != HITS_CYS) && (bits & 0x7fffffffu) <= 0x7f800000u && o <= a.cut &&
                      (!a.allowed || a.allowed[q] != 0);
#pragma unroll
            for (int c = 0; c < BEAM_MAX_DEPTH - 1; ++c) ok = ok && q != taken[c];
            keys[m + i] = ok ? ((hkey_t)o << 32) | ((uint32_t)v << 16 | (uint32_t)q << 5 | (uint32_t)aa) : HITS_NONE;
        }
        const int n = hits_pow2(m + cand);                                    // (>= 2 m: cand >= 20 and n is a power of two above m)
        for (int i = m + cand + tid; i < n; i += HITS_THREADS) keys[i] = HITS_NONE;
        __syncthreads();
        hits_topk(keys, n, m);                                                // ends behind a barrier: keys[m ..) may be overwritten
    }
    __syncthreads();
    hkey_t *out = a.ws + (int64_t)w * a.kd;
    for (int i = tid; i < a.kd; i += HITS_THREADS) out[i] = keys[i];
}

__global__ __launch_bounds__(HITS_THREADS) void beam_merge_kernel(BeamArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int tid = threadIdx.x, k = a.k, kd = a.kd, d = a.depth, m = hits_pow2(kd);
    const int total = a.W * kd, n = max(hits_pow2(total), m);
    for (int i = tid; i < n; i += HITS_THREADS) keys[i] = i < total ? a.ws[i] : HITS_NONE;
    __syncthreads();
    hits_topk(keys, n, m);                                                    // keys[0 .. kd): the leaders; behind them the image is free
    int32_t *sets = (int32_t *)(keys + HITS_MAX_K);                           // [HITS_MAX_K][BEAM_MAX_DEPTH]
    int32_t *keep = sets + HITS_MAX_K * BEAM_MAX_DEPTH;                       // [HITS_MAX_K]
    const hkey_t x = tid < kd ? keys[tid] : HITS_NONE;                        // (NONE sorts last: a valid entry has only valid ones before it)
    const uint32_t lo = (uint32_t)x;
    const int parent = (int)(lo >> 16), add = (int)(lo & 0xffffu);
    if (x != HITS_NONE) {
        const int32_t *mv = a.muts + (int64_t)parent * (d - 1);               // (not read when d = 1)
        int32_t *set = sets + tid * BEAM_MAX_DEPTH;
        int o = 0;
        bool placed = false;
        for (int c = 0; c < d - 1; ++c) {
            const int e = mv[c];
            if (!placed && add < e) {
                set[o++] = add;
                placed = true;
            }
            set[o++] = e;
        }
        if (!placed) set[o++] = add;
    }
    __syncthreads();
    bool mine = x != HITS_NONE;
    if (mine) {
        const int32_t *set = sets + tid * BEAM_MAX_DEPTH;
        for (int j = 0; j < tid && mine; ++j) {
            const int32_t *other = sets + j * BEAM_MAX_DEPTH;
            bool same = true;
            for (int c = 0; c < d; ++c) same = same && set[c] == other[c];
            mine = !same;
        }
    }
    if (tid < HITS_MAX_K) keep[tid] = mine ? 1 : 0;
    __syncthreads();
    if (tid >= HITS_MAX_K) return;                                            // (k <= kd <= 256: the rest has nothing to write)
    int rank = 0, kept = 0;
    for (int j = 0; j < kd; ++j) {
        const int f = keep[j];
        rank += j < tid ? f : 0;
        kept += f;
    }
    const int count = kept < k ? kept : k;
    if (mine && rank < k) {
        const uint32_t o = (uint32_t)(x >> 32);
        a.out_score[rank] = (o & 0x80000000u) ? o ^ 0x80000000u : ~o;         // hits_ord undone (a -0.0 sum comes back as +0.0)
        a.out_parent[rank] = parent;
        a.fresh[rank] = add;
        for (int c = 0; c < d; ++c) a.out_muts[(int64_t)rank * d + c] = sets[tid * BEAM_MAX_DEPTH + c];
    }
    if (tid >= count && tid < k) {                                            // padding rows: one writer each, disjoint from the kept rows
        a.out_score[tid] = 0x7fc00000u;
        a.out_parent[tid] = -1;
        a.fresh[tid] = -1;
        for (int c = 0; c < d; ++c) a.out_muts[(int64_t)tid * d + c] = -1;
    }
    if (tid == 0) a.out_count[0] = count;
}

__global__ __launch_bounds__(BEAM_ROW_THREADS) void beam_rows_kernel(BeamArgs a) {
    const int r = blockIdx.x, q = blockIdx.y * BEAM_ROW_THREADS + threadIdx.x;
    if (q >= a.L) return;
    const int parent = a.out_parent[r];
    int s = 20;                                                               // a legal decoder letter that makes no candidates
    if (parent >= 0) {
        const int add = a.fresh[r];
        s = (add >> 5) == q ? (add & 31) : a.S_var[(int64_t)parent * a.L + q];
    }
    a.out_S[(int64_t)r * a.L + q] = s;
}

// ---- many proteins ---------------------------------------------------------------------------------------------------------------
#define BEAM_EACH_MAX_GRID (1 << 13)                                          // workgroups per launch; the slots beyond are looped over

struct BeamEachArgs {
    const float *ddg;               // [V, T, ld]
    int ld;
    const int32_t *S_var;           // [V, T]
    const float *score;             // [P, V]
    const int32_t *muts;            // [P, V, depth - 1]; a position is local to its protein
    const int32_t *allowed;         // [T] or null
    const int32_t *offsets;         // [P + 1] or null (V == 0 or T == 0: every protein empty)
    int depth;
    int P, V;
    int64_t T;
    int max_len, nblk;              // nblk = ceil(max_len / 256)
    int k, kd, W;                   // W = min(V nblk, 8192 / m - 1) slots per protein
    uint32_t cut;
    int flags;
    hkey_t *ws;                     // [P][W][kd]
    int32_t *fresh;                 // [P][k]
    int32_t *out_muts;              // [P, k, depth]
    uint32_t *out_score;            // [P, k]
    int32_t *out_parent, *out_S, *out_count;   // [P, k], [k, T], [P]
};

// protein p's rows [o, o + L): false (and L = 0, nothing of p may be read) unless 0 <= offsets[p] <= offsets[p + 1] <= T and L <= max_len
__device__ __forceinline__ bool beam_each_range(const BeamEachArgs &a, int p, int64_t &o, int &L) {
    o = 0;
    L = 0;
    if (!a.offsets) return true;
    const int64_t lo = a.offsets[p], hi = a.offsets[p + 1];
    if (lo < 0 || hi < lo || hi > a.T || hi - lo > (int64_t)a.max_len) return false;
    o = lo;
    L = (int)(hi - lo);
    return true;
}

__global__ __launch_bounds__(HITS_THREADS) void beam_each_block_kernel(BeamEachArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int tid = threadIdx.x, m = hits_pow2(a.kd), nm = a.depth - 1;
    const bool cys = (a.flags & TMPNN_BEAM_INCLUDE_CYS) != 0;
    const int64_t slots = (int64_t)a.P * a.W;
    for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {        // (uniform over the workgroup, as everything derived from it)
        const int p = (int)(slot / a.W), w = (int)(slot - (int64_t)p * a.W);
        int64_t o;
        int L;
        beam_each_range(a, p, o, L);                                          // a refused protein has L = 0: no item, kd times NONE
        const int nblk = (L + HITS_B - 1) / HITS_B, items = a.V * nblk;       // (V nblk <= 65536 x 8)
        for (int i = tid; i < m; i += HITS_THREADS) keys[i] = HITS_NONE;
        for (int item = w; item < items; item += a.W) {
            const int v = item / nblk, j = item - v * nblk;
            const int r0 = j * HITS_B, rows = L - r0 < HITS_B ? L - r0 : HITS_B, cand = rows * 20;
            const int64_t member = (int64_t)p * a.V + v;
            int taken[BEAM_MAX_DEPTH - 1];
            bool live = true;
#pragma unroll
            for (int c = 0; c < BEAM_MAX_DEPTH - 1; ++c) {
                const int e = c < nm ? a.muts[member * nm + c] : 0;
                live = live && e >= 0;
                taken[c] = c < nm ? e >> 5 : -1;
            }
            const float base = a.score[member];
            const int64_t row0 = (int64_t)v * a.T + o + r0;                   // (< V T <= 2^31 - 1)
            for (int i = tid; i < cand; i += HITS_THREADS) {
                const int r = i / 20, aa = i - r * 20, q = r0 + r;
                const uint32_t s = (uint32_t)a.S_var[row0 + r];
                const float sum = __fadd_rn(base, a.ddg[(row0 + r) * a.ld + aa]);
                const uint32_t bits = __float_as_uint(sum), od = hits_ord(bits);
                bool ok = live && s < 20u && (uint32_t)aa != s && (cys || aa != HITS_CYS) && (bits & 0x7fffffffu) <= 0x7f800000u &&
                          od <= a.cut && (!a.allowed || a.allowed[o + q] != 0);
#pragma unroll
                for (int c = 0; c < BEAM_MAX_DEPTH - 1; ++c) ok = ok && q != taken[c];
                keys[m + i] = ok ? ((hkey_t)od << 32) | ((uint32_t)v << 16 | (uint32_t)q << 5 | (uint32_t)aa) : HITS_NONE;
            }
            const int n = hits_pow2(m + cand);
            for (int i = m + cand + tid; i < n; i += HITS_THREADS) keys[i] = HITS_NONE;
            __syncthreads();
            hits_topk(keys, n, m);
        }
        __syncthreads();
        hkey_t *out = a.ws + slot * a.kd;
        for (int i = tid; i < a.kd; i += HITS_THREADS) out[i] = keys[i];
        __syncthreads();                                                      // the next slot starts by overwriting the leaders
    }
}

__global__ __launch_bounds__(HITS_THREADS) void beam_each_merge_kernel(BeamEachArgs a) {
    __shared__ hkey_t keys[HITS_MAX_KEYS];
    const int tid = threadIdx.x, k = a.k, kd = a.kd, d = a.depth, m = hits_pow2(kd);
    const int total = a.W * kd, n = max(hits_pow2(total), m);
    int32_t *sets = (int32_t *)(keys + HITS_MAX_K);                           // [HITS_MAX_K][BEAM_MAX_DEPTH]
    int32_t *keep = sets + HITS_MAX_K * BEAM_MAX_DEPTH;                       // [HITS_MAX_K]
    for (int p = blockIdx.x; p < a.P; p += gridDim.x) {
        int64_t o;
        int L;
        const bool good = beam_each_range(a, p, o, L);
        const hkey_t *ws = a.ws + (int64_t)p * total;
        for (int i = tid; i < n; i += HITS_THREADS) keys[i] = good && i < total ? ws[i] : HITS_NONE;
        __syncthreads();
        hits_topk(keys, n, m);
        const hkey_t x = tid < kd ? keys[tid] : HITS_NONE;                    // (the sets lie behind the kd <= 256 leaders)
        const uint32_t lo = (uint32_t)x;
        const int parent = (int)(lo >> 16), add = (int)(lo & 0xffffu);
        if (x != HITS_NONE) {
            const int32_t *mv = a.muts + ((int64_t)p * a.V + parent) * (d - 1);   // (not read when d = 1)
            int32_t *set = sets + tid * BEAM_MAX_DEPTH;
            int c2 = 0;
            bool placed = false;
            for (int c = 0; c < d - 1; ++c) {
                const int e = mv[c];
                if (!placed && add < e) {
                    set[c2++] = add;
                    placed = true;
                }
                set[c2++] = e;
            }
            if (!placed) set[c2++] = add;
        }
        __syncthreads();
        bool mine = x != HITS_NONE;
        if (mine) {
            const int32_t *set = sets + tid * BEAM_MAX_DEPTH;
            for (int j = 0; j < tid && mine; ++j) {
                const int32_t *other = sets + j * BEAM_MAX_DEPTH;
                bool same = true;
                for (int c = 0; c < d; ++c) same = same && set[c] == other[c];
                mine = !same;
            }
        }
        if (tid < HITS_MAX_K) keep[tid] = mine ? 1 : 0;
        __syncthreads();
        if (tid < HITS_MAX_K) {                                               // (k <= kd <= 256: the rest has nothing to write)
            int rank = 0, kept = 0;
            for (int j = 0; j < kd; ++j) {
                const int f = keep[j];
                rank += j < tid ? f : 0;
                kept += f;
            }
            const int count = kept < k ? kept : k;
            const int64_t row = (int64_t)p * k;
            if (mine && rank < k) {
                const uint32_t od = (uint32_t)(x >> 32);
                a.out_score[row + rank] = (od & 0x80000000u) ? od ^ 0x80000000u : ~od;
                a.out_parent[row + rank] = parent;
                a.fresh[row + rank] = add;
                for (int c = 0; c < d; ++c) a.out_muts[(row + rank) * d + c] = sets[tid * BEAM_MAX_DEPTH + c];
            }
            if (tid >= count && tid < k) {
                a.out_score[row + tid] = 0x7fc00000u;
                a.out_parent[row + tid] = -1;
                a.fresh[row + tid] = -1;
                for (int c = 0; c < d; ++c) a.out_muts[(row + tid) * d + c] = -1;
            }
            if (tid == 0) a.out_count[p] = good ? count : -1;
        }
        __syncthreads();                                                      // the next protein's keys overwrite the sets and the flags
    }
}

__global__ __launch_bounds__(BEAM_ROW_THREADS) void beam_each_rows_kernel(BeamEachArgs a) {
    const int64_t per = (int64_t)a.k * a.nblk, slots = (int64_t)a.P * per;
    for (int64_t slot = blockIdx.x; slot < slots; slot += gridDim.x) {
        const int p = (int)(slot / per);
        const int rem = (int)(slot - (int64_t)p * per), r = rem / a.nblk, q = (rem - r * a.nblk) * BEAM_ROW_THREADS + threadIdx.x;
        int64_t o;
        int L;
        beam_each_range(a, p, o, L);                                          // (refused: L = 0, no column is written)
        if (q >= L) continue;
        const int parent = a.out_parent[(int64_t)p * a.k + r];
        int s = 20;
        if (parent >= 0) {
            const int add = a.fresh[(int64_t)p * a.k + r];
            s = (add >> 5) == q ? (add & 31) : a.S_var[(int64_t)parent * a.T + o + q];
        }
        a.out_S[(int64_t)r * a.T + o + q] = s;
    }
}

// ---- the C-ABI entries ---------------------------------------------------------------------------------------------------------
static bool beam_sizes_served(int64_t V, int64_t L, int k, int depth) {
    return V >= 0 && V <= BEAM_MAX_V && L >= 0 && L <= BEAM_MAX_LEN && k >= 1 && depth >= 1 && depth <= BEAM_MAX_DEPTH &&
           (int64_t)k * depth <= HITS_MAX_K && (L == 0 || V <= (int64_t)0x7fffffff / L);
}
static int beam_pow2_host(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}
static int64_t beam_items(int64_t V, int64_t L) { return V * ((L + HITS_B - 1) / HITS_B); }
static int beam_groups(int64_t V, int64_t L, int kd) {
    const int64_t items = beam_items(V, L), most = HITS_MAX_KEYS / beam_pow2_host(kd) - 1;
    return (int)(items < most ? items : most);
}
struct BeamWs {
    hkey_t *keys;
    int32_t *fresh;
};
static BeamWs beam_ws(Carver &c, int64_t V, int64_t L, int k, int depth) {
    BeamWs w;
    w.keys = c.take<hkey_t>((size_t)beam_groups(V, L, k * depth) * (size_t)(k * depth));
    w.fresh = c.take<int32_t>((size_t)k);
    return w;
}

extern "C" size_t tmpnn_beam_step_workspace_bytes(int64_t V, int64_t L, int k, int depth) {
    if (!beam_sizes_served(V, L, k, depth)) return 0;
    Carver c;
    beam_ws(c, V, L, k, depth);
    return c.used + 256;
}

extern "C" int tmpnn_beam_step(const float *ddg, int ld, const int32_t *S_var, const float *score, const int32_t *muts, int depth,
                               const int32_t *allowed_opt, int64_t V, int64_t L, int k, float cutoff, int flags, int32_t *out_muts,
                               float *out_score, int32_t *out_parent, int32_t *out_S, int32_t *out_count, void *workspace,
                               size_t workspace_bytes, tmpnn_stream_t stream) {
    if (V < 0 || L < 0) return tm_set_error(TMPNN_E_INVALID, "beam_step: bad sizes (V=%lld, L=%lld)", (long long)V, (long long)L);
    if (depth < 1 || depth > BEAM_MAX_DEPTH)
        return tm_set_error(TMPNN_E_INVALID, "beam_step: depth=%d outside [1, %d]", depth, BEAM_MAX_DEPTH);
    if (k < 1) return tm_set_error(TMPNN_E_INVALID, "beam_step: k=%d, at least one child is kept", k);
    const bool empty = V == 0 || L == 0;                                      // (an empty beam has no address: the inputs are not read)
    if ((!empty && (!ddg || !S_var || !score || (depth > 1 && !muts))) || !out_muts || !out_score || !out_parent || !out_count ||
        (L > 0 && !out_S) || !workspace)
        return tm_set_error(TMPNN_E_INVALID, "beam_step: null pointer");
    if (ld < 20) return tm_set_error(TMPNN_E_INVALID, "beam_step: ld=%d, a ddG table has at least 20 columns", ld);
    if (flags & ~TMPNN_BEAM_INCLUDE_CYS) return tm_set_error(TMPNN_E_INVALID, "beam_step: unknown flag bits 0x%x", (unsigned)flags);
    uint32_t cb;
    memcpy(&cb, &cutoff, 4);
    if ((cb & 0x7fffffffu) > 0x7f800000u)
        return tm_set_error(TMPNN_E_INVALID, "beam_step: the cutoff is NaN (+inf removes no candidate)");
    if ((int64_t)k * depth > HITS_MAX_K)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step: k depth = %d x %d exceeds %d, the leaders one workgroup dedupes", k, depth,
                            HITS_MAX_K);
    if (L > BEAM_MAX_LEN)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step: L=%lld exceeds %d, the key's 11 position bits", (long long)L, BEAM_MAX_LEN);
    if (V > BEAM_MAX_V)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step: V=%lld exceeds %d, the key's 16 member bits", (long long)V, BEAM_MAX_V);
    if (!beam_sizes_served(V, L, k, depth))
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step: V L = %lld x %lld rows exceed 2^31 - 1", (long long)V, (long long)L);
    Carver c(workspace, true);
    const BeamWs w = beam_ws(c, V, L, k, depth);
    if (c.used > workspace_bytes)
        return tm_set_error(TMPNN_E_WORKSPACE, "beam_step: workspace %zu < %zu bytes", workspace_bytes,
                            tmpnn_beam_step_workspace_bytes(V, L, k, depth));
    const int kd = k * depth, W = beam_groups(V, L, kd), nblk = (int)((L + HITS_B - 1) / HITS_B);
    const BeamArgs a{ddg, ld, S_var, score, muts, allowed_opt, depth, (int)V, (int)L, nblk, (int)beam_items(V, L), k, kd, W, hits_ord(cb),
                     flags, w.keys, w.fresh, out_muts, (uint32_t *)out_score, out_parent, out_S, out_count};
    hipStream_t st = (hipStream_t)stream;
    if (W > 0) {
        tm_prof_begin("beam_block", st);
        hipLaunchKernelGGL(beam_block_kernel, dim3((unsigned)W), dim3(HITS_THREADS), 0, st, a);
        tm_prof_end(st);
        if (int rc = tm_check_launch("beam_block_kernel")) return rc;
    }
    tm_prof_begin("beam_merge", st);
    hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(HITS_THREADS), 0, st, a);
    tm_prof_end(st);
    if (int rc = tm_check_launch("beam_merge_kernel")) return rc;
    if (nblk == 0) return TMPNN_OK;
    tm_prof_begin("beam_rows", st);
    hipLaunchKernelGGL(beam_rows_kernel, dim3((unsigned)k, (unsigned)nblk), dim3(BEAM_ROW_THREADS), 0, st, a);
    tm_prof_end(st);
    return tm_check_launch("beam_rows_kernel");
}

// ---- ... for many proteins ---------------------------------------------------------------------------------------------------
static bool beam_each_sizes_served(int P, int64_t V, int max_len, int k, int depth) {
    return P >= 0 && beam_sizes_served(V, max_len, k, depth);
}
struct BeamEachWs {
    hkey_t *keys;
    int32_t *fresh;
};
static BeamEachWs beam_each_ws(Carver &c, int P, int64_t V, int max_len, int k, int depth) {
    BeamEachWs w;
    w.keys = c.take<hkey_t>((size_t)P * (size_t)beam_groups(V, max_len, k * depth) * (size_t)(k * depth));
    w.fresh = c.take<int32_t>((size_t)P * (size_t)k);
    return w;
}

extern "C" size_t tmpnn_beam_step_each_workspace_bytes(int P, int64_t V, int max_len, int k, int depth) {
    if (!beam_each_sizes_served(P, V, max_len, k, depth)) return 0;
    Carver c;
    beam_each_ws(c, P, V, max_len, k, depth);
    return c.used + 256;
}

extern "C" int tmpnn_beam_step_each(const float *ddg, int ld, const int32_t *S_var, const float *score, const int32_t *muts, int depth,
                                    const int32_t *allowed_opt, const int32_t *offsets, int P, int64_t T, int64_t V, int max_len, int k,
                                    float cutoff, int flags, int32_t *out_muts, float *out_score, int32_t *out_parent, int32_t *out_S,
                                    int32_t *out_count, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    if (P < 0 || V < 0 || T < 0 || max_len < 0)
        return tm_set_error(TMPNN_E_INVALID, "beam_step_each: bad sizes (P=%d, V=%lld, T=%lld, max_len=%d)", P, (long long)V, (long long)T,
                            max_len);
    if (depth < 1 || depth > BEAM_MAX_DEPTH)
        return tm_set_error(TMPNN_E_INVALID, "beam_step_each: depth=%d outside [1, %d]", depth, BEAM_MAX_DEPTH);
    if (k < 1) return tm_set_error(TMPNN_E_INVALID, "beam_step_each: k=%d, at least one child is kept", k);
    const bool empty = P == 0 || V == 0 || T == 0;                            // (nothing to read: the inputs may have no address)
    if ((!empty && (!ddg || !S_var || !score || !offsets || (depth > 1 && !muts))) ||
        (P > 0 && (!out_muts || !out_score || !out_parent || !out_count || (T > 0 && !out_S) || !workspace)))
        return tm_set_error(TMPNN_E_INVALID, "beam_step_each: null pointer");
    if (ld < 20) return tm_set_error(TMPNN_E_INVALID, "beam_step_each: ld=%d, a ddG table has at least 20 columns", ld);
    if (flags & ~TMPNN_BEAM_INCLUDE_CYS) return tm_set_error(TMPNN_E_INVALID, "beam_step_each: unknown flag bits 0x%x", (unsigned)flags);
    uint32_t cb;
    memcpy(&cb, &cutoff, 4);
    if ((cb & 0x7fffffffu) > 0x7f800000u)
        return tm_set_error(TMPNN_E_INVALID, "beam_step_each: the cutoff is NaN (+inf removes no candidate)");
    if ((int64_t)k * depth > HITS_MAX_K)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step_each: k depth = %d x %d exceeds %d, the leaders one workgroup dedupes", k, depth,
                            HITS_MAX_K);
    if (max_len > BEAM_MAX_LEN)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step_each: max_len=%d exceeds %d, the key's 11 position bits", max_len, BEAM_MAX_LEN);
    if (V > BEAM_MAX_V)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step_each: V=%lld exceeds %d, the key's 16 member bits", (long long)V, BEAM_MAX_V);
    if (T > 0 && V > (int64_t)0x7fffffff / T)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "beam_step_each: V T = %lld x %lld rows exceed 2^31 - 1", (long long)V, (long long)T);
    if (P == 0) return TMPNN_OK;
    Carver c(workspace, true);
    const BeamEachWs w = beam_each_ws(c, P, V, max_len, k, depth);
    if (c.used > workspace_bytes)
        return tm_set_error(TMPNN_E_WORKSPACE, "beam_step_each: workspace %zu < %zu bytes", workspace_bytes,
                            tmpnn_beam_step_each_workspace_bytes(P, V, max_len, k, depth));
    const int kd = k * depth, nblk = (max_len + HITS_B - 1) / HITS_B;
    const int W = T == 0 ? 0 : beam_groups(V, max_len, kd);                   // (no row: no item; the workspace is sized for T > 0)
    const BeamEachArgs a{ddg, ld, S_var, score, muts, allowed_opt, empty ? nullptr : offsets, depth, P, (int)V, T, max_len, nblk, k, kd, W,
                         hits_ord(cb), flags, w.keys, w.fresh, out_muts, (uint32_t *)out_score, out_parent, out_S, out_count};
    hipStream_t st = (hipStream_t)stream;
    const auto grid = [](int64_t slots) { return dim3((unsigned)(slots < BEAM_EACH_MAX_GRID ? slots : BEAM_EACH_MAX_GRID)); };
    if (W > 0) {
        tm_prof_begin("beam_each_block", st);
        hipLaunchKernelGGL(beam_each_block_kernel, grid((int64_t)P * W), dim3(HITS_THREADS), 0, st, a);
        tm_prof_end(st);
        if (int rc = tm_check_launch("beam_each_block_kernel")) return rc;
    }
    tm_prof_begin("beam_each_merge", st);
    hipLaunchKernelGGL(beam_each_merge_kernel, grid(P), dim3(HITS_THREADS), 0, st, a);
    tm_prof_end(st);
    if (int rc = tm_check_launch("beam_each_merge_kernel")) return rc;
    if (nblk == 0 || T == 0 || empty) return TMPNN_OK;
    tm_prof_begin("beam_each_rows", st);
    hipLaunchKernelGGL(beam_each_rows_kernel, grid((int64_t)P * k * nblk), dim3(BEAM_ROW_THREADS), 0, st, a);
    tm_prof_end(st);
    return tm_check_launch("beam_each_rows_kernel");
}
