// Autoregressive sampling over one encoded backbone (tmpnn_sample, tmpnn_sample_tied; protein_mpnn_utils.py:1279-1494) and over
// every protein of a packed batch on its own steps (tmpnn_sample_each, tmpnn_sample_tied_each): sample_chain_kernel<SP, TIED, EACH>.
//
// A CHAIN is one sequence being sampled over the packed residue axis (T rows); N chains per call, each with its own decoding order,
// fixed positions and uniform draws. One workgroup (512 threads, 8 wavefronts) owns a group of up to 16 chains and loops over the T
// steps INSIDE the kernel; the grid is ceil(N / 16) workgroups. No workgroup ever reads what another writes: there is no grid
// barrier, no spin-wait, no flag, and the only atomic is the OR into the status word.
//
// Step s of chain c, t = order[c][s] — the arithmetic tmpnn_decode_ordered performs for row t of a variant whose ranks are the inverse
// of `order`. For layer l = 0..2: the own term Wa_l h_in + ba_l (layer 0: the ctx's P0 row; above: the projection of the layer below's
// output, made in this step), the message pass over t's 48 neighbour slots exactly as var_msg8_kernel<SP, true> runs it (W1e_l hE[t]
// from a ZERO accumulator; a neighbour j the chain has already decoded gives the chain's own row Wc_l h^l[c][j] + seq_table[l][S[c][j]],
// every other neighbour the encoder-state row Penc_l[j]; GELU, GEMM 2, GELU, masked sum), and the node update of the group's 16 rows
// (W3 with the count, LayerNorm, feed-forward, LayerNorm, times mask[t]). Then logits, probs = softmax(logits / temperature + bias[t])
// (times allowed[t], renormalised), the inverse-CDF draw, and the chain's three neighbour-projection rows of t go to the table
// [N, 3, T, 128] with the sequence term of the letter just chosen.
//
// Precisions. The message GEMMs are templated on SP as var_msg8_kernel is (f16x2 reads the K-permuted fragment images of W1e / W2,
// bf16x3 splits the fp32 weights as it loads them). The 16-row node update, the projections and the logits are ONE form for both:
// the exact-fp32 matrix-core arithmetic of node_update_kernel<1> (v_mfma_f32_16x16x4_f32, weights from the raw tensors), so nothing
// here needs an image and no new weights exist. An fp32 handle is refused by the launcher with TMPNN_E_UNSUPPORTED (its message names
// "bf16x3", the precision to use instead).
//
// Tied form (sample_chain_kernel<SP, true>, tmpnn_sample_tied; protein_mpnn_utils.py:1385-1494). A chain's steps fall into GROUPS
// (maximal runs of steps ending at close == 1) that share one draw. Per chain the LDS holds the open group's first step, whether a
// masked member ended it (and which), and the 21 weighted logits so far. A member whose group is dead runs with row mask
// mask[t] * alive = 0, so its state is exactly zero; a non-closing step stores its three table rows WITHOUT the sequence term (a later
// member of the group sees this state and no letter), the closing step computes the group's distribution and letter, stores its own
// rows with the term as the untied form does, and adds the term to the earlier members' rows (row = row + seq_tab[l][letter]: the
// same single fp32 add, so an untied chain's bits are the untied form's). The untied form (<SP, false>) is the kernel as it was,
// instruction for instruction, and the only one tmpnn_sample launches.
//
// Ordering. Between a step's table writes and the next step's gathers stand a workgroup-scope release, one __syncthreads() and a
// workgroup-scope acquire. Untied, a row is stored once and never LOADED before that (a neighbour that is not yet decoded is read
// from Penc_l, never from the table). Tied, a row can be loaded by a later member of its group, then rewritten at the close, then
// loaded again — and that is ordered too: a chain's rows are written and read by the wavefronts of ONE workgroup only, all of which
// run on one CU and go through that CU's one vector L1 (write-through; a store updates or drops the line it hits), so after the
// release -> barrier -> acquire every later load of the address, by any of them, returns the rewritten row. The rewrite itself is a
// load and a store of the same address by the lanes that stored the row before (the chain's half-wavefront), in program order. Rows
// are whole 128-byte lines (512 bytes, 256-byte-aligned base), so no line holds part of a row already written and part of one still
// to be written. The rank array (residue -> step, the host fills it with a large value, the prologue scatters `order` into it) is
// complete before its first load. All of this holds for the per-protein form as it stands: a work item there is one workgroup too,
// the rows of the table and of the rank array it touches are those of ITS chains at ITS protein's residues (a step or a neighbour
// outside [t0, t1) is skipped before anything is indexed with it), so no two workgroups share a row, and the same release ->
// barrier -> acquire stands between a step's writes and the next step's gathers.
//
// Per-protein form (sample_chain_kernel<SP, TIED, true>; tmpnn_sample_each, tmpnn_sample_tied_each). The ctx is a packed batch of P
// proteins and a WORK ITEM is (protein b, block of 16 chains): workgroup i of the (p1 - p0) * ceil(N / 16) takes the protein
// sched[i / nblk] (or p0 + i / nblk) and the chain block i % nblk, reads t0 = offsets[b], t1 = offsets[b + 1] and runs the prologue
// and the step loop for s in [t0, t1) only; chain n's schedule for the protein is order[n, t0:t1], a permutation of t0..t1-1.
// Every [N,T] / [T,21] array is indexed by the packed residue as before; the scratch (table, rank array, the encoder state's
// projections) holds the rows [row0, row0 + rows) of the launch's protein range and is indexed with t - row0, [t0, t1) is clipped to
// that window, and a step whose residue falls outside it is skipped as an out-of-range entry is. Visibility is rank < s with the
// packed s, which compares as the local step does; the arithmetic of a step is untouched and E_idx never leaves the protein, so a
// (protein, chain) pair has the bits of tmpnn_sample on that protein encoded alone. Tied: the first group opens at s = t0 and
// the segment's last step closes regardless of `close` (the host refuses a batch where it would not). The EACH = false forms take
// t0 = 0, t1 = T, row0 = 0, rows = T as constants: they are the kernels as they were.
//
// Safe indices. An `order` entry outside [0, T) skips the step for that chain (nothing is dereferenced with it); letters are clamped to
// [0, 21) before they reach a table; non-finite logits or probabilities OR TMPNN_STATUS_RANGE and the step takes S_fixed.
// Independence. Every number of a chain comes from its own rows alone (each output element of the 16-row GEMMs is its own fma chain,
// LayerNorm reduces inside a row): results do not depend on N, on the chain's slot in its group or on its companions.
#include <stdio.h>
#include <stdlib.h>

#include "tmpnn_split.h"
#include "tmpnn_internal.h"

#define TM_SAMPLE_CHAINS 16

struct SampleLayer {
    const float *W1e; int ld1;
    const float *W2, *b2;
    const char *imgp1, *imgp2;                       // f16x2: K-permuted fragment images of W1e / W2
    const float *W3, *b3, *n1w, *n1b, *Win, *bin, *Wout, *bout, *n2w, *n2b;
    const float *Wa; int lda; const float *ba; const float *Wc; int ldc;     // projection of THIS layer's output for layer l + 1 (l < 2)
    const float *seq_tab;                            // [21,128] sequence term of this layer's neighbour rows
    const float *Penc;                               // [T,256]: the encoder state's projection (neighbour half used)
};

struct SampleArgs {
    SampleLayer L[3];
    const float *Wlog, *blog;                        // W_out [21,128], b [21]
    const float *hE; const int32_t *E_idx; const float *hV, *P0, *mask;
    const int32_t *order, *S_fixed;
    const float *free_, *u;
    float inv_temp;
    const float *bias, *allowed;                     // [T,21] or null
    int32_t *S_out; float *probs; int32_t *status;
    float *tab;                                      // [N,3,T,128]
    int32_t *rank;                                   // [N,T], pre-filled with a large value
    int T, N;
    // tied form only (sample_chain_kernel<SP, true>)
    const int32_t *close;                            // [N,T] 1 = the step ends its group
    const float *weight;                             // [N,T] by residue, or null (1)
    const float *pssm_mix, *pssm_bias, *pssm_keep;   // [T], [T,21], [T,21] or null
    // per-protein form only (sample_chain_kernel<SP, TIED, true>): tab / rank / Penc hold the rows [row0, row0 + rows) of the batch
    const int32_t *offsets, *sched;                  // [P+1]; [np] launch order as protein indices, or null (index order)
    int p0, np, row0, rows;
};

// 16-row fp32 GEMM unit: columns [n0 + 16 wv, +16) of W (rows of the weight matrix) against the swizzled [16,128] tile
__device__ __forceinline__ f4 sample_gemm16(const float *tile, const float *W, int ld, int n0, int k0, int n_rows, f4 init, int lane) {
    float wf[1][32];
    load_wfrag<8>(W, ld, n0, k0, n_rows, wf[0], lane);
    f4 acc[1][1];
    acc[0][0] = init;
    mma_tile<8, 1, 128, 1>(tile, wf, acc, lane);
    return acc[0][0];
}

// The tied form's step epilogue for one chain (one thread): a live member adds weight[t] * logits to the group's accumulator; the
// closing step turns the accumulator into the group's distribution and letter (tmpnn.h, tmpnn_sample_tied). Every per-residue table
// is read at the CLOSING member t (the reference's leaked loop variable, :1468-1488). Leaves the letter in S and the probs row that
// every member receives (zeros for a dead group) in `logit`.
__device__ __forceinline__ void tied_epilogue(const SampleArgs &a, int c, int t, float mk, bool closing, bool dead, int t_dead,
                                              int &bad_acc, float *acc, float *logit, int &S_out) {
    const int T = a.T;
    const bool live = t >= 0 && !dead;
    if (live) {
        const unsigned *ul = reinterpret_cast<const unsigned *>(logit);
        const float w = a.weight ? a.weight[(size_t)c * T + t] : 1.0f;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < TMPNN_VOCAB; ++k) {
            bad = bad || tm_nonfinite_bits(ul[k]);
            acc[k] = __builtin_fmaf(w, logit[k], acc[k]);
        }
        if (bad) bad_acc = 1;
    }
    if (!closing) return;
    int S = 0;
    float p[TMPNN_VOCAB];
#pragma unroll
    for (int k = 0; k < TMPNN_VOCAB; ++k) p[k] = 0.f;
    if (live) {
        const size_t ct = (size_t)c * T + t;
        bool bad = bad_acc != 0;
        float z[TMPNN_VOCAB];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < TMPNN_VOCAB; ++k) {
            z[k] = acc[k] * a.inv_temp + (a.bias ? a.bias[(size_t)t * TMPNN_VOCAB + k] : 0.f);
            mx = fmaxf(mx, z[k]);
        }
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < TMPNN_VOCAB; ++k) {
            p[k] = expf(z[k] - mx);
            den += p[k];
        }
#pragma unroll
        for (int k = 0; k < TMPNN_VOCAB; ++k) p[k] = p[k] / den;
        if (a.pssm_mix) {                                           // :1472-1476
            const float mix = a.pssm_mix[t];
#pragma unroll
            for (int k = 0; k < TMPNN_VOCAB; ++k) p[k] = (1.0f - mix) * p[k] + mix * a.pssm_bias[(size_t)t * TMPNN_VOCAB + k];
        }
        if (a.pssm_keep) {                                          // :1477-1481
            float d1 = 0.f;
#pragma unroll
            for (int k = 0; k < TMPNN_VOCAB; ++k) {
                p[k] = p[k] * a.pssm_keep[(size_t)t * TMPNN_VOCAB + k] + p[k] * 0.001f;
                d1 += p[k];
            }
#pragma unroll
            for (int k = 0; k < TMPNN_VOCAB; ++k) p[k] = p[k] / d1;
        }
        if (a.allowed) {
            float d2 = 0.f;
#pragma unroll
            for (int k = 0; k < TMPNN_VOCAB; ++k) {
                p[k] = p[k] * a.allowed[(size_t)t * TMPNN_VOCAB + k];
                d2 += p[k];
            }
#pragma unroll
            for (int k = 0; k < TMPNN_VOCAB; ++k) p[k] = p[k] / d2;
        }
        float cum[TMPNN_VOCAB];
        float run = 0.f;
#pragma unroll
        for (int k = 0; k < TMPNN_VOCAB; ++k) {
            run += p[k];
            cum[k] = run;
        }
        {   // raw-bit test of the computed total (see tm_f16_range_computed): NaN / inf / not positive
            float tot = run;
            asm volatile("" : "+v"(tot));
            const unsigned b = __float_as_uint(tot);
            bad = bad || tm_nonfinite_bits(b) || (b >> 31) != 0u || (b & 0x7fffffffu) == 0u;
        }
        const float thr = a.u[ct] * run;
        int pick = -1, lastpos = 0;
#pragma unroll
        for (int k = TMPNN_VOCAB - 1; k >= 0; --k)
            if (cum[k] > thr) pick = k;                             // ends at the smallest such k
#pragma unroll
        for (int k = 0; k < TMPNN_VOCAB; ++k)
            if (p[k] > 0.f) lastpos = k;
        if (pick < 0) pick = lastpos;
        int sf = a.S_fixed[ct];
        sf = sf < 0 ? 0 : sf >= TMPNN_VOCAB ? TMPNN_VOCAB - 1 : sf;
        const bool is_free = a.free_[ct] * mk == 1.0f;
        if (bad) {
            if (a.status) atomicOr(a.status, TMPNN_STATUS_RANGE);
            pick = sf;
        }
        pick = pick < 0 ? 0 : pick >= TMPNN_VOCAB ? TMPNN_VOCAB - 1 : pick;
        S = is_free ? pick : sf;
    } else if (dead) {                                              // :1445-1448: the letter of the member that ended the group
        const int sf = a.S_fixed[(size_t)c * T + t_dead];
        S = sf < 0 ? 0 : sf >= TMPNN_VOCAB ? TMPNN_VOCAB - 1 : sf;
        if (bad_acc && a.status) atomicOr(a.status, TMPNN_STATUS_RANGE);
    }
    S_out = S;
#pragma unroll
    for (int k = 0; k < TMPNN_VOCAB; ++k) logit[k] = p[k];
}

template <typename SP, bool TIED, bool EACH>
__global__ __launch_bounds__(512) void sample_chain_kernel(SampleArgs a) {
    constexpr int TILEB = SP::NP * SPLIT_PLANE_BYTES, NC = TM_SAMPLE_CHAINS;
    constexpr bool PERM = SP::NP == 2;
    __shared__ __attribute__((aligned(16))) char tA[2][TILEB];      // [1]: e planes, [0]: activation planes
    __shared__ __attribute__((aligned(16))) float tS[NC * TM_H];    // summed messages of the 16 rows (swizzled tile)
    __shared__ __attribute__((aligned(16))) float tH[NC * TM_H];    // node state of the 16 rows: layer input, then output
    __shared__ __attribute__((aligned(16))) float tB[NC * TM_H];
    __shared__ __attribute__((aligned(16))) float tC[NC * TM_H];
    __shared__ __attribute__((aligned(16))) float s_own[NC * TM_H]; // own term of the current layer, row-major
    __shared__ __attribute__((aligned(16))) float s_nb[2][NC * TM_H];   // neighbour halves of layers 1, 2 (without the sequence term)
    __shared__ float s_logit[NC][32];
    __shared__ int s_j[NC][TM_KS];
    __shared__ int s_vis[NC][TM_KS];
    __shared__ float s_cnt[NC], s_mk[NC];
    __shared__ int s_t[NC], s_S[NC];
    // tied form: the chain's open group — its first step, whether a masked member ended it (and which), the weighted logits so far
    __shared__ int s_gs[TIED ? NC : 1], s_close[TIED ? NC : 1], s_dead[TIED ? NC : 1], s_tdead[TIED ? NC : 1], s_bad[TIED ? NC : 1];
    __shared__ float s_acc[TIED ? NC : 1][TMPNN_VOCAB];
    const int tid = tm_tid(), lane = tid & 63, wv = tid >> 6, m = lane & 15, q = lane >> 4;
    const int ncol = 16 * wv + 4 * q, c4 = 4 * wv + q;
    const int c4s = PERM ? perm_c4(c4) : c4;
    const int c32 = lane & 31, hw = tid >> 5;                       // row phases: half-wavefront hw owns row hw
    const int T = a.T;
    const f4 z4 = f4{0.f, 0.f, 0.f, 0.f};
    // steps [t0, t1) over residues [t0, t1); scratch rows are t - r0 of TR (the whole axis unless EACH)
    int cg0 = tm_bid() * NC, t0 = 0, t1 = T, r0 = 0, TR = T;
    if constexpr (EACH) {                                           // work item (protein b, block of 16 chains); all of it workgroup-uniform
        const int nblk = (a.N + NC - 1) / NC, pi = tm_bid() / nblk;
        cg0 = (tm_bid() - pi * nblk) * NC;
        const int b = a.sched ? a.sched[pi] : a.p0 + pi;
        if (b < a.p0 || b >= a.p0 + a.np) return;
        r0 = a.row0;
        TR = a.rows;
        const int lo = r0 > 0 ? r0 : 0, hi = r0 + TR < T ? r0 + TR : T;     // a step outside the scratch's rows is skipped
        t0 = a.offsets[b];
        t1 = a.offsets[b + 1];
        t0 = t0 > lo ? t0 : lo;
        t1 = t1 < hi ? t1 : hi;
        if (t1 <= t0) return;
    }

    // ---- prologue: rank[c][order[c][s]] = s
    for (int r = 0; r < NC; ++r) {
        const int c = cg0 + r;
        if (c >= a.N) break;
        for (int s = t0 + tid; s < t1; s += 512) {
            const int t = a.order[(size_t)c * T + s];
            if (t >= t0 && t < t1) a.rank[(size_t)c * TR + (t - r0)] = s;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    for (int s = t0; s < t1; ++s) {
        // ---- the step's residues
        if (tid < NC) {
            const int c = cg0 + tid, cc = c < a.N ? c : a.N - 1;
            const int t = a.order[(size_t)cc * T + s];
            const bool ok = c < a.N && t >= t0 && t < t1;
            s_t[tid] = ok ? t : -1;
            if constexpr (TIED) {
                if (s == t0 || s_close[tid]) {                       // the step before closed a group: a new one opens here
                    s_gs[tid] = s;
                    s_dead[tid] = 0;
                    s_bad[tid] = 0;
#pragma unroll
                    for (int k = 0; k < TMPNN_VOCAB; ++k) s_acc[tid][k] = 0.f;
                }
                s_close[tid] = c < a.N ? (a.close[(size_t)cc * T + s] != 0 ? 1 : 0) : 1;
                if constexpr (EACH) {
                    if (s == t1 - 1) s_close[tid] = 1;              // a segment's last step closes regardless
                }
                const float mk = ok ? a.mask[t] : 0.f;
                if (ok && !s_dead[tid] && mk == 0.f) {              // the reference's break (:1444-1450): the group is dead from t on
                    s_dead[tid] = 1;
                    s_tdead[tid] = t;
                }
                s_mk[tid] = s_dead[tid] ? 0.f : mk;                 // mask[t] * alive: a skipped member's state is zero
            } else {
                s_mk[tid] = ok ? a.mask[t] : 0.f;
            }
        }
        __syncthreads();
        {   // neighbour lists, visibility, counts: wavefront wv looks after rows 2 wv, 2 wv + 1
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int r = 2 * wv + k, t = s_t[r], tt = t < 0 ? 0 : t;
                const int c = cg0 + r, cc = c < a.N ? c : a.N - 1;
                int j = -1;
                if (lane < TM_KS) j = a.E_idx[(size_t)tt * TM_KS + lane];
                if (j >= t1) j = -1;                                // (never on a ctx of tmpnn_encode)
                if constexpr (EACH) {
                    if (j < t0) j = -1;                             // (nor this: E_idx never leaves the protein)
                }
                const unsigned long long have = __ballot(j >= 0);
                int vis = 0;
                if (j >= 0) vis = a.rank[(size_t)cc * TR + (j - r0)] < s ? 1 : 0;
                if (lane < TM_KS) {
                    s_j[r][lane] = j;
                    s_vis[r][lane] = vis;
                }
                if (lane == 0) s_cnt[r] = (float)__popcll(have);
            }
            // rows of the encoder state and layer 0's own term
            const int t = s_t[hw], tt = t < 0 ? 0 : t;
            st4(tH + chunk_off(hw, c32), ld4(a.hV + (size_t)tt * TM_H + 4 * c32));
            st4(s_own + hw * TM_H + 4 * c32, ld4(a.P0 + (size_t)tt * 256 + 4 * c32));
            st4(tS + chunk_off(hw, c32), z4);
        }
        __syncthreads();

#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            const SampleLayer &L = a.L[l];
            {   // ---- message pass, chain after chain (var_msg8_kernel<SP, true> with one variant per tile)
                WFragS<SP> w1[1][4], w2[1][4];
                load_wfrag_auto<SP, PERM>(PERM ? L.imgp1 : nullptr, L.W1e, L.ld1, wv, lane, w1[0]);
                load_wfrag_auto<SP, PERM>(PERM ? L.imgp2 : nullptr, L.W2, TM_H, wv, lane, w2[0]);
                const f4 bias2 = ld4(L.b2 + ncol);
                const int prow = 6 * wv + (lane >> 5), pc = lane & 31;
                const int pcs = PERM ? perm_c4(pc) : pc;
                f4 e[3];
                auto fetch_e = [&](int r) {                         // the e tile of row r's residue, row layout
                    const int t = s_t[r < NC ? r : NC - 1], tt = t < 0 ? 0 : t;
                    const float *src = a.hE + (size_t)tt * (TM_KS * TM_H);
#pragma unroll
                    for (int it = 0; it < 3; ++it) e[it] = ld4(src + ((prow + 2 * it) * TM_H + 4 * pc));
                };
                fetch_e(0);
#pragma unroll 1
                for (int r = 0; r < NC; ++r) {
                    const int t = __builtin_amdgcn_readfirstlane(s_t[r]);
                    if (t < 0) {                                    // (workgroup-uniform)
                        fetch_e(r + 1);
                        continue;
                    }
                    const int c = cg0 + r;
#pragma unroll
                    for (int it = 0; it < 3; ++it) store_split<SP>(tA[1], prow + 2 * it, pcs, e[it]);
                    __syncthreads();                                // e planes complete; tA[0] free (every wavefront is past GEMM 2 of the row before)
                    const float *tabc = a.tab + ((size_t)c * 3 + l) * (size_t)TR * TM_H;
                    f4 gj[3];
                    float ma[3];
#pragma unroll
                    for (int rb = 0; rb < 3; ++rb) {
                        const int j0 = s_j[r][16 * rb + m];
                        const int jj = j0 < 0 ? t : j0;
                        ma[rb] = j0 < 0 ? 0.f : 1.f;
                        const float *p = s_vis[r][16 * rb + m] ? tabc + (size_t)(jj - r0) * TM_H + ncol : L.Penc + (size_t)(jj - r0) * 256 + 128 + ncol;
                        gj[rb] = ld4(p);
                    }
                    const f4 g0 = ld4(s_own + r * TM_H + ncol);
                    const float mi = s_mk[r];
                    f4 e1[3][1];
#pragma unroll
                    for (int rb = 0; rb < 3; ++rb) e1[rb][0] = z4;
                    mma_tile_split<SP, 4, 1, 3, TM_TILE, 256, 4, 0, true, TM_MSG_PF>(tA[1], w1, e1, lane);
#pragma unroll
                    for (int rb = 0; rb < 3; ++rb) store_split<SP>(tA[0], 16 * rb + m, c4s, gelu4(g0 + mi * (e1[rb][0] + gj[rb])));
                    __syncthreads();                                // activation planes complete; tA[1] free
                    fetch_e(r + 1);                                 // the next row's tile travels behind GEMM 2
                    f4 acc[3][1];
#pragma unroll
                    for (int rb = 0; rb < 3; ++rb) acc[rb][0] = bias2;
                    mma_tile_split<SP, 4, 1, 3, TM_TILE, 256, 4, 0, true, TM_MSG_PF>(tA[0], w2, acc, lane);
                    f4 tot = z4;
#pragma unroll
                    for (int rb = 0; rb < 3; ++rb) {
                        const f4 g = gelu4(acc[rb][0]);
                        tot = f4{__builtin_fmaf(g.x, ma[rb], tot.x), __builtin_fmaf(g.y, ma[rb], tot.y), __builtin_fmaf(g.z, ma[rb], tot.z),
                                 __builtin_fmaf(g.w, ma[rb], tot.w)};
                    }
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {                // inclusive DPP row_shr scan over the 16 rows of the lane group
                        float x = tot[cc];
                        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xf, 0xf, true));
                        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xf, 0xf, true));
                        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x114, 0xf, 0xf, true));
                        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x118, 0xf, 0xf, true));
                        tot[cc] = x;
                    }
                    if (m == 15) st4(tS + chunk_off(r, c4), tot);
                }
            }
            __syncthreads();

            // ---- node update of the 16 rows (node_update_kernel<1>'s arithmetic, 16 columns per wavefront)
            {
                const f4 acc = sample_gemm16(tS, L.W3, TM_H, 16 * wv, 0, TM_H, z4, lane);
                const float cn = s_cnt[m];
                const int off = chunk_off(m, c4);
                const f4 dh = (acc + cn * ld4(L.b3 + ncol)) / 30.0f;
                st4(tB + off, ld4(tH + off) + dh);
            }
            __syncthreads();
            {
                float *p = tB + chunk_off(hw, c32);
                st4(p, layer_norm_row(ld4(p), ld4(L.n1w + 4 * c32), ld4(L.n1b + 4 * c32)));
            }
            __syncthreads();
            f4 out = ld4(L.bout + ncol);
#pragma unroll 1
            for (int ch = 0; ch < 4; ++ch) {                        // FFN hidden 512 in four 128-wide chunks
                const f4 hid = sample_gemm16(tB, L.Win, TM_H, 128 * ch + 16 * wv, 0, 512, ld4(L.bin + 128 * ch + ncol), lane);
                st4(tC + chunk_off(m, c4), gelu4(hid));
                __syncthreads();
                out = sample_gemm16(tC, L.Wout, 512, 16 * wv, 128 * ch, TM_H, out, lane);
                __syncthreads();
            }
            {
                const int off = chunk_off(m, c4);
                st4(tC + off, ld4(tB + off) + out);
            }
            __syncthreads();
            {
                f4 y = layer_norm_row(ld4(tC + chunk_off(hw, c32)), ld4(L.n2w + 4 * c32), ld4(L.n2b + 4 * c32));
                y = y * s_mk[hw];
                st4(tH + chunk_off(hw, c32), y);
                st4(tS + chunk_off(hw, c32), z4);                   // (skipped rows of the next layer's message pass read as zero)
            }
            __syncthreads();
            if (l < 2) {                                            // the next layer's own term and this state's neighbour half
                const f4 pa = sample_gemm16(tH, L.Wa, L.lda, 16 * wv, 0, TM_H, ld4(L.ba + ncol), lane);
                const f4 pcn = sample_gemm16(tH, L.Wc, L.ldc, 16 * wv, 0, TM_H, z4, lane);
                st4(s_own + m * TM_H + ncol, pa);
                st4(s_nb[l] + m * TM_H + ncol, pcn);
                __syncthreads();
            }
        }

        // ---- logits: thread (row, letter), the k order of log_probs_kernel
        if (tid < NC * TMPNN_VOCAB) {
            const int r = tid / TMPNN_VOCAB, aa = tid - r * TMPNN_VOCAB;
            const float *wr = a.Wlog + aa * TM_H;
            float sum = 0.f;
#pragma unroll 8
            for (int k = 0; k < TM_H; ++k) sum += wr[k] * tH[chunk_off(r, k >> 2) + (k & 3)];
            s_logit[r][aa] = sum + a.blog[aa];
        }
        __syncthreads();
        // ---- softmax, tables, the draw: one thread per chain
        if constexpr (TIED) {
            if (tid < NC) tied_epilogue(a, cg0 + tid, s_t[tid], s_mk[tid], s_close[tid] != 0, s_dead[tid] != 0, s_tdead[tid],
                                        s_bad[tid], s_acc[tid], s_logit[tid], s_S[tid]);
        } else if (tid < NC) {
            const int t = s_t[tid], c = cg0 + tid;
            if (t >= 0) {
                const size_t ct = (size_t)c * T + t;
                const unsigned *ul = reinterpret_cast<const unsigned *>(&s_logit[tid][0]);
                bool bad = false;
                float z[TMPNN_VOCAB], p[TMPNN_VOCAB];
                float mx = -INFINITY;
#pragma unroll
                for (int k = 0; k < TMPNN_VOCAB; ++k) {
                    bad = bad || tm_nonfinite_bits(ul[k]);
                    z[k] = s_logit[tid][k] * a.inv_temp + (a.bias ? a.bias[(size_t)t * TMPNN_VOCAB + k] : 0.f);
                    mx = fmaxf(mx, z[k]);
                }
                float den = 0.f;
#pragma unroll
                for (int k = 0; k < TMPNN_VOCAB; ++k) {
                    p[k] = expf(z[k] - mx);
                    den += p[k];
                }
#pragma unroll
                for (int k = 0; k < TMPNN_VOCAB; ++k) p[k] = p[k] / den;
                if (a.allowed) {
                    float d2 = 0.f;
#pragma unroll
                    for (int k = 0; k < TMPNN_VOCAB; ++k) {
                        p[k] = p[k] * a.allowed[(size_t)t * TMPNN_VOCAB + k];
                        d2 += p[k];
                    }
#pragma unroll
                    for (int k = 0; k < TMPNN_VOCAB; ++k) p[k] = p[k] / d2;
                }
                float cum[TMPNN_VOCAB];
                float run = 0.f;
#pragma unroll
                for (int k = 0; k < TMPNN_VOCAB; ++k) {
                    run += p[k];
                    cum[k] = run;
                }
                {   // raw-bit test of the computed total (see tm_f16_range_computed): NaN / inf / not positive
                    float tot = run;
                    asm volatile("" : "+v"(tot));
                    const unsigned b = __float_as_uint(tot);
                    bad = bad || tm_nonfinite_bits(b) || (b >> 31) != 0u || (b & 0x7fffffffu) == 0u;
                }
                const float thr = a.u[ct] * run;
                int pick = -1, lastpos = 0;
#pragma unroll
                for (int k = TMPNN_VOCAB - 1; k >= 0; --k)
                    if (cum[k] > thr) pick = k;                     // ends at the smallest such k
#pragma unroll
                for (int k = 0; k < TMPNN_VOCAB; ++k)
                    if (p[k] > 0.f) lastpos = k;
                if (pick < 0) pick = lastpos;
                int sf = a.S_fixed[ct];
                sf = sf < 0 ? 0 : sf >= TMPNN_VOCAB ? TMPNN_VOCAB - 1 : sf;
                const bool is_free = a.free_[ct] * s_mk[tid] == 1.0f;
                if (bad) {
                    if (a.status) atomicOr(a.status, TMPNN_STATUS_RANGE);
                    pick = sf;
                }
                pick = pick < 0 ? 0 : pick >= TMPNN_VOCAB ? TMPNN_VOCAB - 1 : pick;
                const int S = is_free ? pick : sf;
                s_S[tid] = S;
                a.S_out[ct] = S;
                if (a.probs) {
#pragma unroll
                    for (int k = 0; k < TMPNN_VOCAB; ++k) a.probs[ct * TMPNN_VOCAB + k] = is_free ? p[k] : 0.f;
                }
            } else {
                s_S[tid] = 0;
            }
        }
        __syncthreads();
        if constexpr (TIED) {
            // ---- the three neighbour rows of t: WITHOUT a sequence term while the group is open (a later member sees this state and no
            // letter, :1454-1461), with it at the close — and then every earlier member's rows gain it (row = row + seq, the same
            // single fp32 add), written by the half-wavefront that stored them; S_out and the probs row go to every member
            const int t = s_t[hw], c = cg0 + hw;
            if (c < a.N) {
                const bool closing = s_close[hw] != 0;
                const int S = s_S[hw];
                float *tabc = a.tab + (size_t)c * 3 * (size_t)TR * TM_H + 4 * c32;
                const float *sq0 = a.L[0].seq_tab + S * TM_H + 4 * c32, *sq1 = a.L[1].seq_tab + S * TM_H + 4 * c32,
                            *sq2 = a.L[2].seq_tab + S * TM_H + 4 * c32;
                if (t >= 0) {
                    float *row = tabc + (size_t)(t - r0) * TM_H;
                    const f4 n0 = ld4(a.P0 + (size_t)t * 256 + 128 + 4 * c32);
                    const f4 n1 = ld4(s_nb[0] + hw * TM_H + 4 * c32), n2 = ld4(s_nb[1] + hw * TM_H + 4 * c32);
                    if (closing) {
                        st4(row, ld4(sq0) + n0);
                        st4(row + (size_t)TR * TM_H, ld4(sq1) + n1);
                        st4(row + 2 * (size_t)TR * TM_H, ld4(sq2) + n2);
                    } else {
                        st4(row, n0);
                        st4(row + (size_t)TR * TM_H, n1);
                        st4(row + 2 * (size_t)TR * TM_H, n2);
                    }
                }
                if (closing) {
                    for (int sp = s_gs[hw]; sp <= s; ++sp) {
                        const int tp = a.order[(size_t)c * T + sp];
                        if (tp < t0 || tp >= t1) continue;
                        if (sp < s) {
                            float *row = tabc + (size_t)(tp - r0) * TM_H;
                            st4(row, ld4(row) + ld4(sq0));
                            st4(row + (size_t)TR * TM_H, ld4(row + (size_t)TR * TM_H) + ld4(sq1));
                            st4(row + 2 * (size_t)TR * TM_H, ld4(row + 2 * (size_t)TR * TM_H) + ld4(sq2));
                        }
                        const size_t cp = (size_t)c * T + tp;
                        if (c32 == 0) a.S_out[cp] = S;
                        if (a.probs && c32 < TMPNN_VOCAB) a.probs[cp * TMPNN_VOCAB + c32] = s_logit[hw][c32];
                    }
                }
            }
        } else {   // ---- the chain's three neighbour rows of t, with the sequence term of the letter just chosen
            const int t = s_t[hw];
            if (t >= 0) {
                const int S = s_S[hw];
                float *row = a.tab + (size_t)(cg0 + hw) * 3 * (size_t)TR * TM_H + (size_t)(t - r0) * TM_H + 4 * c32;
                const f4 n0 = ld4(a.P0 + (size_t)t * 256 + 128 + 4 * c32);
                st4(row, ld4(a.L[0].seq_tab + S * TM_H + 4 * c32) + n0);
                st4(row + (size_t)TR * TM_H, ld4(a.L[1].seq_tab + S * TM_H + 4 * c32) + ld4(s_nb[0] + hw * TM_H + 4 * c32));
                st4(row + 2 * (size_t)TR * TM_H, ld4(a.L[2].seq_tab + S * TM_H + 4 * c32) + ld4(s_nb[1] + hw * TM_H + 4 * c32));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// Precision by the handle's mode (f16x2 | bf16x3; the caller refuses fp32). Penc[l]: [T,256] projections of the encoder state
// (layer 0: the ctx's P0). rank [N,T] and tab [N,3,T,128] are scratch. `tied` (or null) selects the tied form and carries its
// arrays. `each` (or null) selects the per-protein form: the grid is (p1 - p0) * ceil(N / 16) workgroups, and Penc[l], rank and tab
// then hold the rows [row0, row0 + rows) only ([rows,256], [N,rows], [N,3,rows,128]; Penc[0] = P0 + 256 row0).
// Reads no environment, allocates nothing, never synchronises.
template <bool TIED, bool EACH>
static void sample_chains_go(bool h2, int grid, const SampleArgs &a, hipStream_t st) {
    if (h2) sample_chain_kernel<SplitH2, TIED, EACH><<<grid, 512, 0, st>>>(a);
    else sample_chain_kernel<SplitBF3, TIED, EACH><<<grid, 512, 0, st>>>(a);
}

int launch_sample_chains(const tmpnn_weights *w, const float *hE, const int32_t *E_idx, const float *hV, const float *P0,
                         const float *const *Penc, const float *mask, int64_t T, int64_t N, const int32_t *order, const int32_t *S_fixed,
                         const float *free_, const float *u, float inv_temp, const float *bias, const float *allowed, int32_t *S_out,
                         float *probs, int32_t *status, float *tab, int32_t *rank, const SampleTied *tied, const SampleEach *each,
                         hipStream_t st) {
    SampleArgs a{};
    const bool h2 = w->mode == TM_MM_F16X2;
    for (int l = 0; l < 3; ++l) {
        const DecW &d = w->dec[l];
        SampleLayer &L = a.L[l];
        L.W1e = d.msg.W1e; L.ld1 = d.msg.ld1; L.W2 = d.msg.W2; L.b2 = d.msg.b2;
        L.imgp1 = d.msg.img.p1; L.imgp2 = d.msg.img.p2;
        if (h2 && !(L.imgp1 && L.imgp2))
            return tm_set_error(TMPNN_E_INVALID, "sample: f16x2 handle without the K-permuted fragment images of W1e / W2");
        L.W3 = d.node.W3; L.b3 = d.node.b3; L.n1w = d.node.n1w; L.n1b = d.node.n1b; L.Win = d.node.Win; L.bin = d.node.bin;
        L.Wout = d.node.Wout; L.bout = d.node.bout; L.n2w = d.node.n2w; L.n2b = d.node.n2b;
        const ProjSpec &ps = w->dec[l < 2 ? l + 1 : 2].msg_proj.spec;
        L.Wa = ps.Wa; L.lda = ps.lda; L.ba = ps.ba; L.Wc = ps.Wc; L.ldc = ps.ldc;
        L.seq_tab = w->seq_table[l];
        L.Penc = Penc[l];
    }
    a.Wlog = w->Wout_w; a.blog = w->Wout_b;
    a.hE = hE; a.E_idx = E_idx; a.hV = hV; a.P0 = P0; a.mask = mask;
    a.order = order; a.S_fixed = S_fixed; a.free_ = free_; a.u = u; a.inv_temp = inv_temp; a.bias = bias; a.allowed = allowed;
    a.S_out = S_out; a.probs = probs; a.status = status; a.tab = tab; a.rank = rank;
    a.T = (int)T; a.N = (int)N;
    int grid = (int)((N + TM_SAMPLE_CHAINS - 1) / TM_SAMPLE_CHAINS);
    if (each) {
        a.offsets = each->offsets; a.sched = each->sched;
        a.p0 = (int)each->p0; a.np = (int)(each->p1 - each->p0); a.row0 = (int)each->row0; a.rows = (int)each->rows;
        grid *= a.np;
    }
    if (tied) {
        a.close = tied->close; a.weight = tied->weight; a.pssm_mix = tied->pssm_mix; a.pssm_bias = tied->pssm_bias; a.pssm_keep = tied->pssm_keep;
    }
    const char *name = tied ? (each ? "sample_chains_tied_each" : "sample_chains_tied") : each ? "sample_chains_each" : "sample_chains";
    tm_prof_begin(name, st);
    if (tied && each) sample_chains_go<true, true>(h2, grid, a, st);
    else if (tied) sample_chains_go<true, false>(h2, grid, a, st);
    else if (each) sample_chains_go<false, true>(h2, grid, a, st);
    else sample_chains_go<false, false>(h2, grid, a, st);
    tm_prof_end(st);
    return tm_check_launch(name);
}
