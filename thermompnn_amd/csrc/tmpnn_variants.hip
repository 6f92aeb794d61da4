// Decoder message pass of MANY sequence variants over ONE encoded backbone (tmpnn_decode_variants, tmpnn_decode_ordered),
// split-precision forms (f16x2 and bf16x3): var_msg8_kernel<SP, ORD>. Plus the row-wise
// helpers of those entries (variant_expand_kernel, variant_hidden_kernel, variant_vis_kernel, variant_penc0_kernel, variant_remap_kernel).
#include <stdio.h>
#include <stdlib.h>

#include "tmpnn_split.h"
#include "tmpnn_internal.h"

// ------------------------------------------------------------------------------------------------
// Through the decoder h_E and E_idx are constants of the backbone; the node projections P, and with them the gathers and the sums,
// belong to a variant (row v T + t of the [V T, ...] arrays). The message of edge (i, k) of variant v is
//     gelu(W2 gelu(g0_v[i] + m_i (W1e e_ik + g_v[j_ik])) + b2),
// and W1e e_ik does not know v. A workgroup (8 wavefronts, the column split of msg8_rp_kernel, tmpnn_msg.hip) owns one residue and a
// chunk of VC variants: it fetches and splits the 48 x 128 e tile once, runs GEMM 1 once from a ZERO accumulator and keeps the result —
// 3 row blocks x 4 values per thread — in registers over the variant loop. Per variant: three gathered 16-byte pieces of the
// neighbours' projection rows and one of the residue's own, the GELU, GEMM 2, the GELU and the masked sum over the 48 rows (DPP
// scan, one store per column group). msg8_rp_kernel starts its accumulator AT g_j, so the two kernels sum in a different order: a
// variant's numbers are not the fused forward's bit for bit. They do not depend on V, on the variant's slot or on VC: nothing of
// one variant's arithmetic sees another's.
// The activation planes are double-buffered — the second buffer IS the e planes, dead after GEMM 1 — so a variant costs one
// workgroup barrier: the planes a wavefront writes for variant v + 1 were last read in GEMM 2 of variant v - 1 (or in GEMM 1), which
// every wavefront left before it reached the barrier of variant v. The next variant's gathers ride behind the first MFMA steps of
// GEMM 2 (their rows differ per variant; the addresses do not, up to the uniform base).
// f16x2 reads the K-permuted fragment images of W1e / W2 and writes its planes in that K order (perm_c4), as every message kernel.
//
// Order-masked form (ORD, tmpnn_decode_ordered; protein_mpnn_utils.py:1247-1272 without the overwrite of :1259, as conditional_probs
// :1496-1587 decodes): neighbour j of residue i is VISIBLE to variant v when rank[v][j] < rank[v][i]. A visible neighbour gives
// the variant's own projection row (decoder state of this layer + sequence term), an invisible one the row of the ENCODER state's
// projection Penc_l[j] = W1c_l h_V_enc[j], which knows neither the variant nor the sequence. P is then a [V + 1, T, 256] table
// whose slot V is Penc_l, and the only change to the loop is where a gather points: one 64-bit visibility word per (variant,
// residue) — bit k = slot k visible, made by variant_vis_kernel — is read wave-uniformly with the next variant's prefetch, and
// each lane picks between the two slot bases with its bits 16 rb + m. All offsets stay 32-bit: the launcher bounds (V + 1) T.
// ------------------------------------------------------------------------------------------------
struct VarMsgArgs {
    const float *W1e; int ld1;
    const float *W2, *b2, *P;               // P [V T, 256]
    const float *hE;
    const int32_t *E_idx;
    const float *mask;
    float *Ssum, *cnt;                      // [V T, 128], [V T]
    int T, V, VC, n_chunks;                 // workgroup b: residue b / n_chunks, variants [VC (b % n_chunks), + VC)
    const char *imgp1, *imgp2;              // f16x2: K-permuted fragment images of W1e / W2
    const uint2 *vis;                       // ORD: [V T] visibility words, bit k of (x | y << 32) = slot k of the residue is visible
    unsigned enc_off;                       // ORD: V T 256, the float offset of slot V (Penc_l) inside P
};

// ORD: a lane's gather of row block rb goes to the variant's slot (float offset var_off) or to slot V (enc_off), by bit
// 16 rb + m of the residue's visibility word
__device__ __forceinline__ unsigned var_ord_off(unsigned goff, int rb, int m, uint2 wd, unsigned var_off, unsigned enc_off) {
    const unsigned bit = ((rb < 2 ? wd.x : wd.y) >> (16 * (rb & 1) + m)) & 1u;
    return goff + (bit ? var_off : enc_off);
}

template <typename SP, bool ORD = false>
__global__ __launch_bounds__(512, 2) void var_msg8_kernel(VarMsgArgs a) {
    constexpr int TILEB = SP::NP * SPLIT_PLANE_BYTES;
    __shared__ __attribute__((aligned(16))) char tA[2][TILEB];     // activation planes; [1] holds the e planes until GEMM 1 is through
    __shared__ int s_idx[TM_TILE];
    __shared__ float s_cnt;
    const int tid = tm_tid(), lane = tid & 63, wv = tid >> 6, m = lane & 15, q = lane >> 4;
    const int i = tm_bid() / a.n_chunks, ch = tm_bid() - i * a.n_chunks;
    const int v0 = ch * a.VC, v1 = min(a.V, v0 + a.VC);

    constexpr bool PERM = SP::NP == 2;
    const int ncol = 16 * wv + 4 * q, c4 = 4 * wv + q;
    const int c4s = PERM ? perm_c4(c4) : c4;
    const unsigned ucol = (unsigned)ncol;
    {   // the residue's e tile, row layout (one half-wavefront per 512-byte row), split into planes once
        const int prow = 6 * wv + (lane >> 5), pc = lane & 31;
        const int pcs = PERM ? perm_c4(pc) : pc;
        const float *src = a.hE + (size_t)i * (TM_KS * TM_H);
        f4 e[3];
#pragma unroll
        for (int it = 0; it < 3; ++it) e[it] = ld4(src + ((prow + 2 * it) * TM_H + 4 * pc));
        if (tid < TM_TILE) {                                    // lanes 0..47 of wavefront 0
            const int j = a.E_idx[(size_t)i * TM_KS + tid];
            s_idx[tid] = j;
            const unsigned long long have = __ballot(j >= 0);
            if (tid == 0) s_cnt = (float)__popcll(have);        // the decoder's attention mask is 1 on every listed neighbour
        }
#pragma unroll
        for (int it = 0; it < 3; ++it) store_split<SP>(tA[1], prow + 2 * it, pcs, e[it]);
    }
    WFragS<SP> w2[1][4];
    f4 e1[3][1];
    {
        WFragS<SP> w1[1][4];
        load_wfrag_auto<SP, PERM>(PERM ? a.imgp1 : nullptr, a.W1e, a.ld1, wv, lane, w1[0]);
        load_wfrag_auto<SP, PERM>(PERM ? a.imgp2 : nullptr, a.W2, TM_H, wv, lane, w2[0]);
        __syncthreads();                                        // e planes + neighbour list complete
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) e1[rb][0] = f4{0.f, 0.f, 0.f, 0.f};
        mma_tile_split<SP, 4, 1, 3, TM_TILE, 256, 4, 0, true, TM_MSG_PF>(tA[1], w1, e1, lane);      // W1e e: kept over the variants
    }
    const f4 bias2 = ld4(a.b2 + ncol);
    const float mi = a.mask[i], cntv = s_cnt;
    unsigned goff[3];                                           // this lane's three neighbour rows inside a variant's projection table
    float ma[3];
#pragma unroll
    for (int rb = 0; rb < 3; ++rb) {
        const int j0 = s_idx[16 * rb + m];
        goff[rb] = (unsigned)(j0 < 0 ? i : j0) * 256u + (128u + ucol);      // T <= T_MAX: below 2^32 floats
        ma[rb] = j0 < 0 ? 0.f : 1.f;
    }
    const unsigned soff = (unsigned)i * 256u + ucol;
    const size_t vstride = (size_t)a.T * 256;
    auto vis_word = [&](int v) {                                // wave-uniform: one word per (variant, residue)
        const uint2 wd = a.vis[(size_t)v * a.T + i];
        return uint2{(unsigned)__builtin_amdgcn_readfirstlane((int)wd.x), (unsigned)__builtin_amdgcn_readfirstlane((int)wd.y)};
    };
    f4 g0, gj[3];
    {
        const float *Pv = a.P + (size_t)v0 * vstride;           // wave-uniform base + 32-bit lane offsets
        g0 = ld4(Pv + soff);
        if constexpr (ORD) {
            const uint2 wd = vis_word(v0);
#pragma unroll
            for (int rb = 0; rb < 3; ++rb) gj[rb] = ld4(a.P + var_ord_off(goff[rb], rb, m, wd, (unsigned)v0 * (unsigned)vstride, a.enc_off));
        } else {
#pragma unroll
            for (int rb = 0; rb < 3; ++rb) gj[rb] = ld4(Pv + goff[rb]);
        }
    }
    int buf = 0;
    for (int v = v0; v < v1; ++v) {
        uint2 wn = uint2{0u, 0u};
        if constexpr (ORD) wn = vis_word(v + 1 < v1 ? v + 1 : v);      // the next variant's word, on its way through the GELU below
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) store_split<SP>(tA[buf], 16 * rb + m, c4s, gelu4(g0 + mi * (e1[rb][0] + gj[rb])));
        __syncthreads();                                        // the one barrier of a variant: tA[buf] complete
        const float *Pn = a.P + (size_t)(v + 1 < v1 ? v + 1 : v) * vstride;      // (the last variant asks for its own rows again)
        f4 acc[3][1];
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) acc[rb][0] = bias2;
        mma_tile_split_ride<SP, 4, 3, TM_MSG_PF>(tA[buf], w2, acc, lane, [&](auto S) {
            constexpr int s = decltype(S)::value;
            if constexpr (s == 0) g0 = ld4(Pn + soff);
            if constexpr (s >= 1 && s <= 3) {
                if constexpr (ORD)        // (V + 1) T 256 < 2^32 (launcher)
                    gj[s - 1] = ld4(a.P + var_ord_off(goff[s - 1], s - 1, m, wn, (unsigned)(v + 1 < v1 ? v + 1 : v) * (unsigned)vstride, a.enc_off));
                else gj[s - 1] = ld4(Pn + goff[s - 1]);
            }
        });
        f4 tot = f4{0.f, 0.f, 0.f, 0.f};                        // masked sum over the 48 neighbours, as msg8_rp_kernel forms it
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) {
            const f4 g = gelu4(acc[rb][0]);
            tot = f4{__builtin_fmaf(g.x, ma[rb], tot.x), __builtin_fmaf(g.y, ma[rb], tot.y), __builtin_fmaf(g.z, ma[rb], tot.z),
                     __builtin_fmaf(g.w, ma[rb], tot.w)};
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {                            // inclusive DPP row_shr scan over the 16 rows of the lane group
            float x = tot[c];
            x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xf, 0xf, true));
            x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xf, 0xf, true));
            x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x114, 0xf, 0xf, true));
            x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x118, 0xf, 0xf, true));
            tot[c] = x;
        }
        touch(g0);                                               // the gathers' vmcnt wait in front of the stores
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) touch(gj[rb]);
        const size_t row = (size_t)v * a.T + i;
        if (m == 15) st4(a.Ssum + row * TM_H + ucol, tot);
        if (tid == 0) a.cnt[row] = cntv;
        buf ^= 1;
    }
}

// Rows of an ordered decode: one wavefront per row r = v T + i makes the row's visibility word — bit k is set when slot k of
// residue i holds a neighbour j with rank[v][j] < rank[v][i] (equal ranks: not visible; empty slots: 0).
__global__ __launch_bounds__(TM_THREADS) void variant_vis_kernel(const int32_t *__restrict__ rank, const int32_t *__restrict__ E_idx,
                                                                 int T, int64_t R, uint2 *__restrict__ vis) {
    const int lane = tm_tid() & 63;
    const int64_t wpb = TM_THREADS / 64, nw = (int64_t)tm_nblk() * wpb;
    for (int64_t r = (int64_t)tm_bid() * wpb + (tm_tid() >> 6); r < R; r += nw) {
        const int64_t v = r / T;
        const int i = (int)(r - v * T);
        const int32_t *rk = rank + v * T;
        bool see = false;
        if (lane < TM_KS) {
            const int j = E_idx[(size_t)i * TM_KS + lane];
            see = j >= 0 && rk[j] < rk[i];
        }
        const unsigned long long word = __ballot(see);
        if (lane == 0) vis[r] = uint2{(unsigned)word, (unsigned)(word >> 32)};
    }
}

// Slot V of an ordered decode's [V + 1, T, 256] table for decoder layer 0: the sequence-free projection the encode context holds
// (its neighbour half is W1c_0 h_V_enc). The later layers' slot V is a node_proj of the encoder state.
__global__ __launch_bounds__(TM_THREADS) void variant_penc0_kernel(const float *__restrict__ P0, int64_t T, float *__restrict__ Penc) {
    const int64_t n = T * 64;
    for (int64_t k = (int64_t)tm_bid() * TM_THREADS + tm_tid(); k < n; k += (int64_t)tm_nblk() * TM_THREADS) st4(Penc + 4 * k, ld4(P0 + 4 * k));
}

// fp32 form: variant v's neighbour list for the fused forward's message kernel run on the rows [v T, (V + 1) T) of the table — a
// visible neighbour keeps its row j of the variant's slot, an invisible one becomes row j + delta (delta = (V - v) T: slot V).
__global__ __launch_bounds__(TM_THREADS) void variant_remap_kernel(const uint2 *__restrict__ vis, const int32_t *__restrict__ E_idx,
                                                                   int T, int delta, int32_t *__restrict__ out) {
    const int64_t n = (int64_t)T * TM_KS;
    for (int64_t k = (int64_t)tm_bid() * TM_THREADS + tm_tid(); k < n; k += (int64_t)tm_nblk() * TM_THREADS) {
        const int64_t i = k / TM_KS;
        const int s = (int)(k - i * TM_KS), j = E_idx[k];
        const uint2 wd = vis[i];
        const unsigned bit = ((s < 32 ? wd.x : wd.y) >> (s & 31)) & 1u;
        out[k] = j < 0 || bit ? j : j + delta;
    }
}

// Rows of a decode: row r = v T + t gets the backbone's encoder state, mask and decoder-layer-0 projection, the latter with the
// variant's sequence term tab[S_var[r]] added to the neighbour half — the one fp32 add node_update's fused projection makes
// (NodeProj::add_tab), so the rows carry the bits the fused forward's projection has for that sequence. Zeroes the status word.
__global__ __launch_bounds__(TM_THREADS) void variant_expand_kernel(const float *__restrict__ hV, const float *__restrict__ P0,
                                                                    const float *__restrict__ mask, const float *__restrict__ tab,
                                                                    const int32_t *__restrict__ S_var, int T, int64_t R,
                                                                    float *__restrict__ hV_rep, float *__restrict__ P,
                                                                    float *__restrict__ mask_rep, int32_t *__restrict__ status) {
    if (status && tm_bid() == 0 && tm_tid() == 0) *status = 0;
    const int64_t n = R * 96;                                   // 32 + 64 float4 per row
    for (int64_t k = (int64_t)tm_bid() * TM_THREADS + tm_tid(); k < n; k += (int64_t)tm_nblk() * TM_THREADS) {
        const int64_t r = k / 96;
        const int c = (int)(k - r * 96), t = (int)(r % T);
        if (c < 32) {
            st4(hV_rep + r * TM_H + 4 * c, ld4(hV + (size_t)t * TM_H + 4 * c));
            if (c == 0) mask_rep[r] = mask[t];
        } else {
            const int p = 4 * (c - 32);
            f4 x = ld4(P0 + (size_t)t * 256 + p);
            if (p >= 128) x = ld4(tab + S_var[r] * TM_H + (p - 128)) + x;
            st4(P + r * 256 + p, x);
        }
    }
}

// decoder states [3][V T, 128] (the workspace's layout: what the row-wise kernels write) -> hidden [V, 3, T, 128]
__global__ __launch_bounds__(TM_THREADS) void variant_hidden_kernel(const float *__restrict__ h1, const float *__restrict__ h2,
                                                                    const float *__restrict__ h3, int T, int64_t R,
                                                                    float *__restrict__ out) {
    const int64_t n = R * 96;
    for (int64_t k = (int64_t)tm_bid() * TM_THREADS + tm_tid(); k < n; k += (int64_t)tm_nblk() * TM_THREADS) {
        const int64_t r = k / 96, v = r / T;
        const int c = (int)(k - r * 96), l = c >> 5, t = (int)(r - v * T);
        const float *src = l == 0 ? h1 : l == 1 ? h2 : h3;
        st4(out + ((v * 3 + l) * T + t) * TM_H + 4 * (c & 31), ld4(src + r * TM_H + 4 * (c & 31)));
    }
}

static int rowwise_grid(int64_t n) {
    const int64_t blocks = (n + TM_THREADS - 1) / TM_THREADS, cap = (int64_t)tm_num_cus() * 8;
    return (int)(blocks < cap ? blocks : cap);
}

int launch_variant_expand(const float *hV, const float *P0, const float *mask, const float *tab, const int32_t *S_var, int64_t T,
                          int64_t V, float *hV_rep, float *P, float *mask_rep, int32_t *status, hipStream_t st) {
    const int64_t R = V * T;
    tm_prof_begin("variant_expand", st);
    variant_expand_kernel<<<rowwise_grid(R * 96), TM_THREADS, 0, st>>>(hV, P0, mask, tab, S_var, (int)T, R, hV_rep, P, mask_rep, status);
    tm_prof_end(st);
    return tm_check_launch("variant_expand");
}

int launch_variant_hidden(const float *const *h, int64_t T, int64_t V, float *out, hipStream_t st) {
    const int64_t R = V * T;
    variant_hidden_kernel<<<rowwise_grid(R * 96), TM_THREADS, 0, st>>>(h[0], h[1], h[2], (int)T, R, out);
    return tm_check_launch("variant_hidden");
}

int launch_variant_vis(const int32_t *rank, const int32_t *E_idx, int64_t T, int64_t V, void *vis, hipStream_t st) {
    const int64_t R = V * T;
    tm_prof_begin("variant_vis", st);
    variant_vis_kernel<<<rowwise_grid(R * 64), TM_THREADS, 0, st>>>(rank, E_idx, (int)T, R, (uint2 *)vis);
    tm_prof_end(st);
    return tm_check_launch("variant_vis");
}

int launch_variant_penc0(const float *P0, int64_t T, float *Penc, hipStream_t st) {
    tm_prof_begin("variant_penc0", st);
    variant_penc0_kernel<<<rowwise_grid(T * 64), TM_THREADS, 0, st>>>(P0, T, Penc);
    tm_prof_end(st);
    return tm_check_launch("variant_penc0");
}

// vis == nullptr: every neighbour visible, P [V T, 256] (tmpnn_decode_variants). Otherwise P [(V + 1) T, 256] with Penc_l in slot V,
// (V + 1) T 256 < 2^32 (checked by the caller); remap [T,48]: scratch of the fp32 form.
int launch_variant_msg(int mode, const MsgW &m, const float *P, const float *hE, const int32_t *E_idx, const float *mask, int64_t T,
                       int64_t V, float *Ssum, float *cnt, hipStream_t st, const void *vis, int32_t *remap) {
    if (mode == TM_MM_FP32) {       // the fused forward's own kernel, variant after variant: its arithmetic exactly
        for (int64_t v = 0; v < V; ++v) {
            const int32_t *list = E_idx;
            if (vis) {              // (stream order keeps the one remapped list safe between the variants)
                tm_prof_begin("variant_remap", st);
                variant_remap_kernel<<<rowwise_grid(T * TM_KS), TM_THREADS, 0, st>>>((const uint2 *)vis + (size_t)v * T, E_idx, (int)T,
                                                                                   (int)((V - v) * T), remap);
                tm_prof_end(st);
                const int rc = tm_check_launch("variant_remap");
                if (rc != TMPNN_OK) return rc;
                list = remap;
            }
            const int rc = launch_msg(mode, m, P + (size_t)v * T * 256, hE, list, mask, T, Ssum + (size_t)v * T * TM_H, cnt + (size_t)v * T, st);
            if (rc != TMPNN_OK) return rc;
        }
        return TMPNN_OK;
    }
    const bool h2 = mode == TM_MM_F16X2;
    VarMsgArgs a{m.W1e, m.ld1, m.W2, m.b2, P, hE, E_idx, mask, Ssum, cnt, (int)T, (int)V, 0, 0, m.img.p1, m.img.p2, (const uint2 *)vis,
                 (unsigned)((uint64_t)V * (uint64_t)T * 256u)};
    if (h2 && !(a.imgp1 && a.imgp2))
        return tm_set_error(TMPNN_E_INVALID, "variant_msg: f16x2 handle without the K-permuted fragment images of W1e / W2");
    // Variants per workgroup: all of them once the residues alone fill the chip four times over; below that the variant axis is cut
    // so that they do, but not under 8 variants per workgroup (the tile, GEMM 1 and the weight fragments are paid once per workgroup).
    const int64_t want = (4 * (int64_t)tm_num_cus() + T - 1) / T;
    int64_t vc = (V + want - 1) / want;
    if (vc < 8) vc = V < 8 ? V : 8;
    a.VC = (int)vc;
    a.n_chunks = (int)((V + vc - 1) / vc);
    const int grid = (int)(T * a.n_chunks);
    if (vis) {
        tm_prof_begin("dec_msg_ordered", st);
        if (h2) var_msg8_kernel<SplitH2, true><<<grid, 512, 0, st>>>(a);
        else var_msg8_kernel<SplitBF3, true><<<grid, 512, 0, st>>>(a);
        tm_prof_end(st);
        return tm_check_launch("dec_msg_ordered");
    }
    tm_prof_begin("dec_msg_variants", st);
    if (h2) var_msg8_kernel<SplitH2><<<grid, 512, 0, st>>>(a);
    else var_msg8_kernel<SplitBF3><<<grid, 512, 0, st>>>(a);
    tm_prof_end(st);
    return tm_check_launch("dec_msg_variants");
}
