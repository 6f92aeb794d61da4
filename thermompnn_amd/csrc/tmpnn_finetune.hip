// Fine-tuning of ProteinMPNN together with the ddG head (gfx950): the training forward of one protein that keeps what the backward
// needs, the backward through the head, the 3 decoder layers, W_s, the 3 encoder layers, W_e, norm_edges, edge_embedding and the
// positional embeddings.linear, and gradients into ONE flat fp32 slab.
//
// Reference semantics (/root/reference): transfer_model.py:31-35 (freeze_weights: false leaves ProteinMPNN in train mode),
// train_thermompnn.py:88-113 (AdamW groups), protein_mpnn_utils.py:816-880 (EncLayer / DecLayer, nn.Dropout(0.1) x 15), :1127-1180
// (features), :1222-1277 (ProteinMPNN.forward with order_mask_backward = ones: decoder input [h_V_i | h_E_ij | h_S_j | h_V_j] times
// mask_i, no neighbour mask). One protein of length L per call, K = min(48, L) neighbours, E = L K edge rows (i, k) in row-major order.
//
// Precision: exact fp32 everywhere; every matrix product runs on v_mfma_f32_16x16x4_f32; GELU is the exact-erf form (erff).
//
// Saved activations (workspace, per call): the k-NN graph (E_idx, compacted to [L, K]), the positional class (0..65) of every edge, the
// 416 raw edge features [E_pos(16) | 400 RBF], edge_embedding's output and norm_edges' mean / rstd, h_E before every encoder layer and
// after the last one; per message / edge-update / FFN the two GELU pre-activations; per LayerNorm its input (residual sum) and
// mean / rstd; the node state after every layer; W_s[S]; the head rows [h_dec(last) | ... | W_s[S]] of the labelled mutants.
// Dropout keep-masks are never stored: the backward recomputes them from the generator (or reads the injected masks again).
//
// Determinism: no floating-point atomics. Weight gradients over [L K] or [L] rows: each wavefront sums a fixed block of rows into a
// partial (k-ordered inside the MFMA), a second kernel adds up to FT_MAX_PARTS partials in block order. LayerNorm gamma / beta, column
// sums and class-indexed sums (W_s over S, embeddings.linear over the positional class) use the same two-level fixed order. The sum
// over K runs k = 0..K-1. The transposes of the gathers h_V_j / h_S_j are scatter-adds run as gathers through an inverse-neighbour CSR
// built on the device per protein: a counting sort whose per-node lists are then sorted by edge id (stable (i, k) order; the integer
// atomics of the count only decide where a list is filled, never the order of a float sum). Mutants that share a residue are summed
// through the same kind of CSR, in mutant order.
//
// Dropout generator (p = 0.1, the 15 sites of EncLayer / DecLayer): the stated 64-bit mix tr_mix of tmpnn_train.hip (splitmix64's
// finaliser), k1 = mix(seed ^ 0x9E3779B97F4A7C15), k2 = mix(k1 + step), ks = mix(k2 ^ (0xD6E8FEB86659FD93 * (site + 1))),
// h = mix(ks ^ (row << 32 | col)); the element is KEPT when (h >> 40) >= thr, thr = round(p 2^24), and kept values are scaled by
// 1 / (1 - thr / 2^24). row = residue i for node sites, i K + k for edge sites; col = channel 0..127. Sites:
//   encoder layer l (0..2): 3 l + 0 dropout1 (dh [L,128]), 3 l + 1 dropout2 (FFN output [L,128]), 3 l + 2 dropout3 (edge message [E,128]);
//   decoder layer l (0..2): 9 + 2 l + 0 dropout1 (dh [L,128]), 9 + 2 l + 1 dropout2 (FFN output [L,128]).
// Injected / exported masks (keep_in, keep_out: 0 / 1 values) are one flat buffer, the sites in this order, each [rows, 128].
// tests/test_gpu_finetune.py restates the generator in numpy bit for bit.
//
// The sequence loss (tmpnn_seqloss_forward / _backward, at the end of the file): ProteinMPNN's own objective, log p(S | X) under a decoding
// order (/root/reference/model_utils.py:396-470), on the same kernels. Its decoder operand carries a per-edge-row order predicate
// (FtSeg::vis, ft_row), the inverse-neighbour gathers of the backward take it too (FtCollect::vis), the output layer W_out with its
// log-softmax closes the forward and seeds the backward from any dL / dlog_probs, and the slab is the whole state dict (sq_layout).
// Every operand of the ddG path has vis = 0 and keeps its arithmetic.
//
// Segments: ft_forward / ft_backward run over L rows in n_prot segments (FtCtx, tmpnn_ft.h). Every entry of this file has one segment
// [0, L]; the packed sequence loss (tmpnn_seqbatch.hip, tmpnn_seqloss_batch_*) runs the same two functions over a batch's T rows.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "tmpnn_ft.h"

__device__ __forceinline__ uint64_t ft_mix(uint64_t x) {   // = tr_mix (tmpnn_train.hip)
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ float ft_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float ft_gelu_d(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// ---- dropout (FtDrop: tmpnn_ft.h) -------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ft_keep(const FtDrop &d, int site, int row, int col) {
    if (d.mode == 0) return 1.f;
    const int64_t idx = d.off[site] + (int64_t)row * FT_H + col;
    if (d.mode == 1) return d.keep_in[idx] * d.scale;
    const uint64_t ks = ft_mix(d.k2 ^ (0xD6E8FEB86659FD93ull * (uint64_t)(site + 1)));
    const uint64_t h = ft_mix(ks ^ (((uint64_t)(uint32_t)row << 32) | (uint32_t)col));
    const float keep = (uint32_t)(h >> 40) >= d.thr ? 1.f : 0.f;
    if (d.keep_out) d.keep_out[idx] = keep;
    return keep * d.scale;
}

// ---- gathered operand: the row of A for GEMM row m is up to 4 segments side by side ----------------------------------------------
// mode 0: row m of p; 1: node row m / K (h_V_i); 2: node row E_idx[m] (h_V_j, h_S_j). masked: the segment is scaled by mask[m / K]
// (the decoder's mask_bw). act 2: GELU on every element (the input of W2 / W3 / W_out is GELU of the saved pre-activation).
// Order predicate (the sequence loss; ranks set): edge row m = (i, k) with j = eidx[m] is VISIBLE iff ranks[j] < ranks[i] (equal ranks
// are not, the self edge included). vis 1: the segment is scaled by 0 on an invisible row (h_S_j); vis 2: an invisible row reads
// p2 instead of p (h_V_j of the current layer / of the encoder). vis 0 (every fine-tune operand): the arithmetic is unchanged.
struct FtSeg { const float *p; int ld, width, mode, masked, rows, vis; const float *p2; };
struct FtA { FtSeg s[4]; int n_seg, K, act; const int32_t *eidx; const float *mask; const int32_t *ranks; };

__device__ __forceinline__ bool ft_visible(const int32_t *ranks, const int32_t *eidx, int e, int K, int L) {
    return ranks[min(max(eidx[e], 0), L - 1)] < ranks[e / K];
}

__device__ __forceinline__ const float *ft_row(const FtA &a, const FtSeg &s, int m, float *scale) {
    int r = s.mode == 0 ? m : s.mode == 1 ? m / a.K : a.eidx[m];
    r = min(max(r, 0), s.rows - 1);
    *scale = s.masked ? a.mask[m / a.K] : 1.f;
    const float *base = s.p;
    if (s.vis && !ft_visible(a.ranks, a.eidx, m, a.K, s.rows)) {
        if (s.vis == 1) *scale = 0.f;
        else base = s.p2;
    }
    return base + (size_t)r * s.ld;
}

__device__ __forceinline__ float ft_act(float v, int act) { return act == 2 ? ft_gelu(v) : v; }

// ---- dense layer: Y[m, n] (+)= epi(b[n] + sum_k A(m, k) W[n ldw + k wks]); epi: * gelu'(G[m, n]) when G is set ---------------------
// Same tiling as tr_dense_kernel: one 16-row tile x one 16-column block per wavefront, lane (m, q) holds Y[tile + m, n0 + 4q + r].
struct FtDense { FtA a; const float *W; int ldw, wks; const float *b; float *Y; int ldy; const float *G; int accum, M, N; };

__global__ __launch_bounds__(TM_THREADS) void ft_dense_kernel(FtDense d) {
    const int lane = tm_tid() & 63, wv = tm_wave(tm_tid()), m = lane & 15, q = lane >> 4;
    const int n_tiles = (d.M + 15) / 16, n_cb = (d.N + 15) / 16;
    for (int item = tm_bid() * 4 + wv; item < n_tiles * n_cb; item += tm_nblk() * 4) {
        const int tile = item / n_cb, n0 = (item - tile * n_cb) * 16;
        const int row = tile * 16 + m;
        const bool row_ok = row < d.M;
        const int wrow = n0 + m;
        const bool w_ok = wrow < d.N;
        const float *w = d.W + (size_t)(w_ok ? wrow : 0) * d.ldw;
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        int kbase = 0;
        for (int s = 0; s < d.a.n_seg; ++s) {
            const FtSeg sg = d.a.s[s];
            float sc;
            const float *x = ft_row(d.a, sg, row_ok ? row : 0, &sc);
            for (int k = 0; k < sg.width; k += 4) {
                const int kk = k + q;
                const bool k_ok = kk < sg.width;
                const float xv = row_ok && k_ok ? ft_act(x[kk], d.a.act) * sc : 0.f;
                const float wvv = w_ok && k_ok ? w[(size_t)(kbase + kk) * d.wks] : 0.f;
                acc = mfma16(wvv, xv, acc);
            }
            kbase += sg.width;
        }
        if (!row_ok) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = n0 + 4 * q + r;
            if (col >= d.N) continue;
            const size_t e = (size_t)row * d.ldy + col;
            float y = d.b ? acc[r] + d.b[col] : acc[r];
            if (d.G) y *= ft_gelu_d(d.G[e]);
            if (d.accum) y += d.Y[e];
            d.Y[e] = y;
        }
    }
}

// ---- weight gradient partials: P[part][n][k] = sum over the part's rows m of dY[m, n] A(m, k); column k = Ktot is 1 (the bias) ------
struct FtWgrad { const float *dY; int ldd; FtA a; float *P; int M, N, Ktot, rows_per_part, n_parts; };

__global__ __launch_bounds__(TM_THREADS) void ft_wgrad_kernel(FtWgrad w) {
    const int lane = tm_tid() & 63, wv = tm_wave(tm_tid()), i = lane & 15, q = lane >> 4;
    const int K1 = w.Ktot + 1, n_nb = (w.N + 15) / 16, n_kb = (K1 + 15) / 16;
    for (int item = tm_bid() * 4 + wv; item < n_nb * n_kb * w.n_parts; item += tm_nblk() * 4) {
        const int part = item / (n_nb * n_kb), rest = item - part * (n_nb * n_kb), nb = rest / n_kb, kb = rest - nb * n_kb;
        const int n0 = nb * 16, k0 = kb * 16, m_beg = part * w.rows_per_part, m_end = min(w.M, m_beg + w.rows_per_part);
        const int n = n0 + i, k = k0 + i;
        int seg = 0, kin = k;                                   // the segment that holds column k of A
        while (seg + 1 < w.a.n_seg && kin >= w.a.s[seg].width) { kin -= w.a.s[seg].width; ++seg; }
        const FtSeg sg = w.a.s[seg];
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        for (int m0 = m_beg; m0 < m_end; m0 += 4) {
            const int mm = m0 + q;
            const bool m_ok = mm < m_end;
            const float dy = m_ok && n < w.N ? w.dY[(size_t)mm * w.ldd + n] : 0.f;
            float av = 0.f;
            if (m_ok && k < w.Ktot) {
                float sc;
                const float *x = ft_row(w.a, sg, mm, &sc);
                av = ft_act(x[kin], w.a.act) * sc;
            } else if (m_ok && k == w.Ktot) {
                av = 1.f;
            }
            acc = mfma16(dy, av, acc);
        }
        float *P = w.P + (size_t)part * w.N * K1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int nn = n0 + 4 * q + r;
            if (nn < w.N && k < K1) P[(size_t)nn * K1 + k] = acc[r];
        }
    }
}

// G[n Ktot + k] = sum_p P[p][n][k] (k < Ktot), Gb[n] = sum_p P[p][n][Ktot] (when Gb): partials added in part order.
__global__ __launch_bounds__(TM_THREADS) void ft_wsum_kernel(const float *__restrict__ P, int n_parts, int N, int K, float *__restrict__ G,
                                                             float *__restrict__ Gb) {
    const int K1 = K + 1;
    const int64_t total = (int64_t)N * K1, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t e = (int64_t)tm_bid() * TM_THREADS + tm_tid(); e < total; e += stride) {
        float s = P[e];
        for (int p = 1; p < n_parts; ++p) s += P[(size_t)p * total + e];
        const int n = (int)(e / K1), k = (int)(e - (int64_t)n * K1);
        if (k < K) G[(size_t)n * K + k] = s;
        else if (Gb) Gb[n] = s;
    }
}

// ---- LayerNorm (eps 1e-5, biased variance), one wavefront per 128-wide row ---------------------------------------------------------
__device__ __forceinline__ float ft_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// x = base + keep(site) * delta (delta may be null); y = LN(x) * (omask ? omask[row] : 1). Saves x, mean, rstd.
struct FtLnF { const float *base, *delta; int site; const float *g, *b, *omask; float *xs, *y, *mu, *rs; int R; FtDrop d; };

__global__ __launch_bounds__(TM_THREADS) void ft_ln_fwd_kernel(FtLnF a) {
    const int lane = tm_tid() & 63, wv = tm_wave(tm_tid());
    for (int r = tm_bid() * 4 + wv; r < a.R; r += tm_nblk() * 4) {
        float x[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = 2 * lane + j;
            const size_t e = (size_t)r * FT_H + c;
            x[j] = a.base[e];
            if (a.delta) x[j] += ft_keep(a.d, a.site, r, c) * a.delta[e];
        }
        const float mean = ft_wave_sum(x[0] + x[1]) * (1.f / FT_H);
        const float d0 = x[0] - mean, d1 = x[1] - mean;
        const float var = ft_wave_sum(d0 * d0 + d1 * d1) * (1.f / FT_H);
        const float rstd = 1.f / sqrtf(var + 1e-5f);
        const float om = a.omask ? a.omask[r] : 1.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = 2 * lane + j;
            const size_t e = (size_t)r * FT_H + c;
            a.xs[e] = x[j];
            a.y[e] = ((x[j] - mean) * rstd * a.g[c] + a.b[c]) * om;
        }
        if (lane == 0) { a.mu[r] = mean; a.rs[r] = rstd; }
    }
}

// dy' = dy * omask; dx (+)= rstd (g dy' - mean(g dy') - xh mean(g dy' xh)); ddelta = dx * keep(site) (when set);
// gx = dy' xh and gb = dy' per row (for the fixed-order gamma / beta column sums).
struct FtLnB { const float *dy, *omask, *xs, *mu, *rs, *g; float *dx; int accum; float *ddelta; int site; float *gx, *gb; int R; FtDrop d; };

__global__ __launch_bounds__(TM_THREADS) void ft_ln_bwd_kernel(FtLnB a) {
    const int lane = tm_tid() & 63, wv = tm_wave(tm_tid());
    for (int r = tm_bid() * 4 + wv; r < a.R; r += tm_nblk() * 4) {
        const float om = a.omask ? a.omask[r] : 1.f, mean = a.mu[r], rstd = a.rs[r];
        float dy[2], xh[2], gg[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = 2 * lane + j;
            const size_t e = (size_t)r * FT_H + c;
            dy[j] = a.dy[e] * om;
            xh[j] = (a.xs[e] - mean) * rstd;
            gg[j] = dy[j] * a.g[c];
        }
        const float mg = ft_wave_sum(gg[0] + gg[1]) * (1.f / FT_H);
        const float mgx = ft_wave_sum(gg[0] * xh[0] + gg[1] * xh[1]) * (1.f / FT_H);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = 2 * lane + j;
            const size_t e = (size_t)r * FT_H + c;
            float dx = rstd * (gg[j] - mg - xh[j] * mgx);
            if (a.accum) dx += a.dx[e];
            a.dx[e] = dx;
            if (a.ddelta) a.ddelta[e] = rstd * (gg[j] - mg - xh[j] * mgx) * ft_keep(a.d, a.site, r, c);
            a.gx[e] = dy[j] * xh[j];
            a.gb[e] = dy[j];
        }
    }
}

// ---- graph, features, embeddings ---------------------------------------------------------------------------------------------------
// (the pair order c_ft_pa / c_ft_pb and ft_atom: tmpnn_ft.h)
// per edge e = (i, k): compact E_idx, positional class, Ein[e] = [W_pos[:, cls] + b_pos | 400 RBF]. L rows in N segments (offs [N + 1],
// already made safe: ft_offsets_kernel / sq_segments_kernel); a neighbour is clamped into its residue's own segment.
struct FtGraph { const float *X; const int32_t *ridx, *cenc, *E48; const float *D48, *pos_w, *pos_b; int32_t *eidx, *cls; float *Ein; int L, K;
                 const int32_t *offs; int N; };

__global__ __launch_bounds__(TM_THREADS) void ft_graph_kernel(FtGraph a) {
    const int64_t E = (int64_t)a.L * a.K, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t e = (int64_t)tm_bid() * TM_THREADS + tm_tid(); e < E; e += stride) {
        const int i = (int)(e / a.K), k = (int)(e - (int64_t)i * a.K);
        int lo = 0, hi = a.N;                                 // segment p with offs[p] <= i < offs[p + 1] (as the k-NN kernel finds it)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.offs[mid] <= i) lo = mid; else hi = mid;
        }
        const int s0 = min(max(a.offs[lo], 0), a.L - 1), s1 = min(max(a.offs[lo + 1], s0 + 1), a.L);
        int j = a.E48[(size_t)i * TM_KS + k];
        j = min(max(j, s0), s1 - 1);
        a.eidx[e] = j;
        const int cl = a.cenc[i] == a.cenc[j] ? min(max(a.ridx[i] - a.ridx[j] + 32, 0), 64) : 65;
        a.cls[e] = cl;
        float *out = a.Ein + (size_t)e * 416;
        for (int d = 0; d < 16; ++d) out[d] = a.pos_w[d * 66 + cl] + a.pos_b[d];
        const float *xi = a.X + (size_t)i * 12, *xj = a.X + (size_t)j * 12;
        for (int p = 0; p < 25; ++p) {
            float D;
            if (p == 0) {
                D = a.D48[(size_t)i * TM_KS + k];                 // masked Ca-Ca distance of _dist (:1142)
            } else {
                float A[3], B[3];
                ft_atom(xi, c_ft_pa[p], A);
                ft_atom(xj, c_ft_pb[p], B);
                const float dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
                D = sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
            }
            for (int r = 0; r < 16; ++r) {
                const float mu = r < 8 ? (float)(2.0 + (20.0 / 15.0) * r) : (float)(22.0 - (20.0 / 15.0) * (15 - r));
                const float t = (D - mu) * 0.8f;
                out[16 + 16 * p + r] = expf(-(t * t));
            }
        }
    }
}

__global__ __launch_bounds__(TM_THREADS) void ft_offsets_kernel(int32_t *offs, int L) {
    if (tm_bid() == 0 && tm_tid() == 0) { offs[0] = 0; offs[1] = L; }
}

// hS[i] = W_s[S_i]
__global__ __launch_bounds__(TM_THREADS) void ft_embed_kernel(const float *Ws, const int32_t *S, int L, float *hS) {
    const int64_t n = (int64_t)L * FT_H, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int i = (int)(t / FT_H), c = (int)(t - (int64_t)i * FT_H);
        const int s = min(max(S[i], 0), TMPNN_VOCAB - 1);
        hS[t] = Ws[s * FT_H + c];
    }
}

// headX[m] = [hD[2][pos] | hD[1][pos] | ... (n_final parts) | hS[pos]], rows_id[m] = m
struct FtHeadRows { const float *hD[3]; const float *hS; const int32_t *pos; float *X; int32_t *rows_id; int M, L, nf; };

__global__ __launch_bounds__(TM_THREADS) void ft_head_rows_kernel(FtHeadRows a) {
    const int D0 = FT_H * (a.nf + 1);
    const int64_t n = (int64_t)a.M * D0, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int m = (int)(t / D0), col = (int)(t - (int64_t)m * D0), part = col / FT_H, c = col - part * FT_H;
        const int p = min(max(a.pos[m], 0), a.L - 1);
        const float *src = part < a.nf ? a.hD[2 - part] : a.hS;
        a.X[t] = src[(size_t)p * FT_H + c];
        if (col == 0) a.rows_id[m] = m;
    }
}

// d rows -> per residue: out[part][i, c] = sum over the mutants at i (mutant order) of dX[m, part 128 + c];
// part < nf -> dH[2 - part], part nf -> dS
struct FtHeadScatter { const float *dX; const int32_t *off, *list; float *dH[3]; float *dS; int L, nf; };

__global__ __launch_bounds__(TM_THREADS) void ft_head_scatter_kernel(FtHeadScatter a) {
    const int D0 = FT_H * (a.nf + 1);
    const int64_t n = (int64_t)a.L * D0, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int i = (int)(t / D0), col = (int)(t - (int64_t)i * D0), part = col / FT_H, c = col - part * FT_H;
        float s = 0.f;
        for (int u = a.off[i]; u < a.off[i + 1]; ++u) s += a.dX[(size_t)a.list[u] * D0 + col];
        float *dst = part < a.nf ? a.dH[2 - part] : a.dS;
        dst[(size_t)i * FT_H + c] = s;
    }
}

// ---- message aggregation and its transpose ---------------------------------------------------------------------------------------
// dh[i, c] = (sum_k ma(i, k) msg[i K + k, c]) / 30, ma = mask_i mask_j (encoder, mask_attend) or 1 (decoder)
__global__ __launch_bounds__(TM_THREADS) void ft_msg_sum_kernel(const float *msg, const float *mask, const int32_t *eidx, int attend, int L,
                                                                int K, float *dh) {
    const int64_t n = (int64_t)L * FT_H, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int i = (int)(t / FT_H), c = (int)(t - (int64_t)i * FT_H);
        float s = 0.f;
        for (int k = 0; k < K; ++k) {
            const size_t e = (size_t)i * K + k;
            const float ma = attend ? mask[i] * mask[eidx[e]] : 1.f;
            s += ma * msg[e * FT_H + c];
        }
        dh[t] = s / 30.f;
    }
}

// dmsg[e, c] = ma(e) ddh[i, c] / 30
__global__ __launch_bounds__(TM_THREADS) void ft_msg_expand_kernel(const float *ddh, const float *mask, const int32_t *eidx, int attend, int L,
                                                                   int K, float *dmsg) {
    const int64_t n = (int64_t)L * K * FT_H, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int64_t e = t / FT_H;
        const int c = (int)(t - e * FT_H), i = (int)(e / K);
        const float ma = attend ? mask[i] * mask[eidx[e]] : 1.f;
        dmsg[t] = ma * ddh[(size_t)i * FT_H + c] / 30.f;
    }
}

// out[i, c] = (base ? base[i, c] : 0) + sum_k f(e) src[e, self + c] + sum_{e in inv(i)} f(e) src[e, nb + c]; f(e) = mask[e / K] when
// masked, else 1; self / nb < 0: that term is absent. inv(i): the edges whose neighbour is i, in ascending edge order (the CSR).
// vis 1 / 2 (ranks set): the neighbour term takes only the visible / only the invisible edges, in the same order.
struct FtCollect { float *out; const float *base, *src; int lds, self, nb, masked; const float *mask; const int32_t *off, *list; int L, K;
                   int vis; const int32_t *ranks; };

__global__ __launch_bounds__(TM_THREADS) void ft_collect_kernel(FtCollect a) {
    const int64_t n = (int64_t)a.L * FT_H, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int i = (int)(t / FT_H), c = (int)(t - (int64_t)i * FT_H);
        float s = a.base ? a.base[t] : 0.f;
        if (a.self >= 0) {
            const float f = a.masked ? a.mask[i] : 1.f;
            for (int k = 0; k < a.K; ++k) s += f * a.src[((size_t)i * a.K + k) * a.lds + a.self + c];
        }
        if (a.nb >= 0)
            for (int u = a.off[i]; u < a.off[i + 1]; ++u) {
                const int e = a.list[u];
                if (a.vis && (a.ranks[i] < a.ranks[e / a.K]) != (a.vis == 1)) continue;
                const float f = a.masked ? a.mask[e / a.K] : 1.f;
                s += f * a.src[(size_t)e * a.lds + a.nb + c];
            }
        a.out[t] = s;
    }
}

// dst[e, c] = (a ? a[e, c] : dst[e, c]) + f(e) b[e, off + c] (f = mask[e / K] when masked)
__global__ __launch_bounds__(TM_THREADS) void ft_edge_add_kernel(float *dst, const float *a, const float *b, int ldb, int off, const float *mask,
                                                                 int masked, int64_t E, int K) {
    const int64_t n = E * FT_H, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int64_t e = t / FT_H;
        const int c = (int)(t - e * FT_H);
        const float f = masked ? mask[e / K] : 1.f;
        dst[t] = (a ? a[t] : dst[t]) + f * b[e * ldb + off + c];
    }
}

// ---- fixed-order class-indexed sums: dst[cl ldc + c ldd] = sum over rows r with cls[r] == cl (all rows when cls is null) of src[r, off + c]
__global__ __launch_bounds__(TM_THREADS) void ft_class_part_kernel(const int32_t *cls, const float *src, int lds, int off, int R, int C, int ncls,
                                                                   int P, int rpp, float *part) {
    const int64_t n = (int64_t)P * ncls * C, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t t = (int64_t)tm_bid() * TM_THREADS + tm_tid(); t < n; t += stride) {
        const int p = (int)(t / ((int64_t)ncls * C)), rest = (int)(t - (int64_t)p * ncls * C), cl = rest / C, c = rest - cl * C;
        const int r1 = min(R, (p + 1) * rpp);
        float s = 0.f;
        for (int r = p * rpp; r < r1; ++r)
            if (!cls || cls[r] == cl) s += src[(size_t)r * lds + off + c];
        part[t] = s;
    }
}

__global__ __launch_bounds__(TM_THREADS) void ft_class_fin_kernel(const float *part, int P, int ncls, int C, float *dst, int ldc, int ldd) {
    const int n = ncls * C;
    for (int t = tm_bid() * TM_THREADS + tm_tid(); t < n; t += tm_nblk() * TM_THREADS) {
        float s = 0.f;
        for (int p = 0; p < P; ++p) s += part[(size_t)p * n + t];
        const int cl = t / C, c = t - cl * C;
        dst[(size_t)cl * ldc + (size_t)c * ldd] = s;
    }
}

// ---- CSR of keys[0..n) over [0, nbins): off [nbins + 1], list = the indices grouped by key, ascending inside each group ------------
__global__ __launch_bounds__(TM_THREADS) void ft_csr_count_kernel(const int32_t *keys, int n, int nbins, int32_t *cnt) {
    for (int t = tm_bid() * TM_THREADS + tm_tid(); t < n; t += tm_nblk() * TM_THREADS)
        atomicAdd(&cnt[min(max(keys[t], 0), nbins - 1)], 1);
}

__global__ __launch_bounds__(TM_THREADS) void ft_csr_scan_kernel(const int32_t *cnt, int nbins, int32_t *off, int32_t *cur) {
    __shared__ int s_tot[TM_THREADS];
    const int tid = tm_tid(), per = (nbins + TM_THREADS - 1) / TM_THREADS, b0 = min(nbins, tid * per), b1 = min(nbins, b0 + per);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += cnt[b];
    s_tot[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < TM_THREADS; ++t) { const int v = s_tot[t]; s_tot[t] = run; run += v; }
        off[nbins] = run;
    }
    __syncthreads();
    int run = s_tot[tid];
    for (int b = b0; b < b1; ++b) { off[b] = run; cur[b] = run; run += cnt[b]; }
}

__global__ __launch_bounds__(TM_THREADS) void ft_csr_fill_kernel(const int32_t *keys, int n, int nbins, int32_t *cur, int32_t *list) {
    for (int t = tm_bid() * TM_THREADS + tm_tid(); t < n; t += tm_nblk() * TM_THREADS)
        list[atomicAdd(&cur[min(max(keys[t], 0), nbins - 1)], 1)] = t;
}

__global__ __launch_bounds__(TM_THREADS) void ft_csr_sort_kernel(const int32_t *off, int nbins, int32_t *list) {
    for (int b = tm_bid() * TM_THREADS + tm_tid(); b < nbins; b += tm_nblk() * TM_THREADS) {
        const int lo = off[b], hi = off[b + 1];
        for (int u = lo + 1; u < hi; ++u) {
            const int v = list[u];
            int w = u - 1;
            while (w >= lo && list[w] > v) { list[w + 1] = list[w]; --w; }
            list[w + 1] = v;
        }
    }
}

// ---- the sequence loss's output layer: one thread per residue, sums over the 21 letters in index order -----------------------------
__global__ __launch_bounds__(TM_THREADS) void sq_logsoftmax_kernel(float *lg, int L) {      // logits -> log_probs, in place
    for (int i = tm_bid() * TM_THREADS + tm_tid(); i < L; i += tm_nblk() * TM_THREADS) {
        float *x = lg + (size_t)i * TMPNN_VOCAB, mx = x[0], s = 0.f;
        for (int a = 1; a < TMPNN_VOCAB; ++a) mx = fmaxf(mx, x[a]);
        for (int a = 0; a < TMPNN_VOCAB; ++a) s += expf(x[a] - mx);
        const float lse = mx + logf(s);
        for (int a = 0; a < TMPNN_VOCAB; ++a) x[a] -= lse;
    }
}

__global__ __launch_bounds__(TM_THREADS) void sq_dlogits_kernel(const float *dlp, const float *lp, int L, float *dlg) {
    for (int i = tm_bid() * TM_THREADS + tm_tid(); i < L; i += tm_nblk() * TM_THREADS) {
        const size_t o = (size_t)i * TMPNN_VOCAB;
        float s = 0.f;
        for (int a = 0; a < TMPNN_VOCAB; ++a) s += dlp[o + a];
        for (int a = 0; a < TMPNN_VOCAB; ++a) dlg[o + a] = dlp[o + a] - expf(lp[o + a]) * s;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
static int ft_dims_ok(int n_final, int n_layers, const int32_t *dims) {
    if (n_final < 0 || n_final > 3 || n_layers < 1 || n_layers > FT_MAX_LAYERS || !dims) return 0;
    if (dims[0] != FT_H * n_final + FT_H || dims[n_layers] != TMPNN_VOCAB) return 0;
    for (int l = 1; l < n_layers; ++l)
        if (dims[l] < 1 || dims[l] > 4096) return 0;
    return 1;
}

// Slab offsets (FtLayout: tmpnn_ft.h)
static FtLayout ft_layout(int n_final) {
    FtLayout S{};
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o += n; return r; };
    const int64_t H = FT_H;
    if (n_final == 0) {
        S.Ws = take(TMPNN_VOCAB * H);
        S.head = o;
        return S;
    }
    S.posw = take(16 * 66); S.posb = take(16); S.edgew = take(H * 416); S.new_ = take(H); S.neb = take(H);
    S.Wew = take(H * H); S.Web = take(H); S.Ws = take(TMPNN_VOCAB * H);
    for (int l = 0; l < 3; ++l) {
        FtEncP &e = S.enc[l];
        e.n1w = take(H); e.n1b = take(H); e.n2w = take(H); e.n2b = take(H); e.n3w = take(H); e.n3b = take(H);
        e.W1 = take(H * 3 * H); e.b1 = take(H); e.W2 = take(H * H); e.b2 = take(H); e.W3 = take(H * H); e.b3 = take(H);
        e.W11 = take(H * 3 * H); e.b11 = take(H); e.W12 = take(H * H); e.b12 = take(H); e.W13 = take(H * H); e.b13 = take(H);
        e.Win = take(4 * H * H); e.bin = take(4 * H); e.Wout = take(H * 4 * H); e.bout = take(H);
    }
    for (int l = 0; l < 3; ++l) {
        FtDecP &d = S.dec[l];
        d.n1w = take(H); d.n1b = take(H); d.n2w = take(H); d.n2b = take(H);
        d.W1 = take(H * 4 * H); d.b1 = take(H); d.W2 = take(H * H); d.b2 = take(H); d.W3 = take(H * H); d.b3 = take(H);
        d.Win = take(4 * H * H); d.bin = take(4 * H); d.Wout = take(H * 4 * H); d.bout = take(H);
    }
    S.head = o;
    return S;
}

// The sequence loss's slab, a layout of its own: ProteinMPNN's tensors in state-dict order with W_out.weight [21,128] and W_out.bias
// [21] at the end, and no head.
FtLayout sq_layout() {
    FtLayout S = ft_layout(3);
    S.Wo = S.head;
    S.bo = S.Wo + TMPNN_VOCAB * FT_H;
    S.total = S.bo + TMPNN_VOCAB;
    return S;
}

static int ft_parts(int64_t M) {
    const int64_t p = (M + 63) / 64;
    return (int)(p < 1 ? 1 : p > FT_MAX_PARTS ? FT_MAX_PARTS : p);
}
static int ft_cparts(int64_t R) {
    const int64_t p = (R + 255) / 256;
    return (int)(p < 1 ? 1 : p > FT_CLS_PARTS ? FT_CLS_PARTS : p);
}

// The workspace in two parts (FtWs, tmpnn_ft.h), carved in a fixed order.
// seq: the sequence loss's buffers (tmpnn_seqloss_*): no mutants and no head (M = 0, dims unused), log_probs and two gradients more.
FtWs ft_carve2(void *saved, void *scratch, bool split, int64_t L, int64_t M, int lightattn, int n_layers, const int32_t *dims, bool seq,
               int64_t Kc, int64_t n_prot) {
    FtWs w{};
    Carver sv(saved, false), sc(scratch, false);       // (a null base measures; the entries compare with the byte counts first)
    auto f = [&](int64_t n) { return sv.take<float>((size_t)n); };
    auto i32 = [&](int64_t n) { return sv.take<int32_t>((size_t)n); };
    auto fc = [&](int64_t n) { return sc.take<float>((size_t)n); };
    auto ic = [&](int64_t n) { return sc.take<int32_t>((size_t)n); };
    const int64_t K = Kc > 0 ? Kc : L < TM_KS ? L : TM_KS, E = L * K, H = FT_H, D0 = seq ? 0 : dims[0];
    // saved
    w.offs = i32(n_prot + 1); w.E48 = i32(L * TM_KS); w.eidx = i32(E); w.cls = i32(E); w.rows_id = i32(M); w.status = i32(1);
    w.D48 = f(L * TM_KS); w.Ein = f(E * 416); w.E0 = f(E * H); w.nemu = f(E); w.ners = f(E); w.En = f(E * H);
    for (int l = 0; l < 4; ++l) w.hE[l] = f(E * H);
    w.hV0 = f(L * H); w.hS = f(L * H); w.headX = f(M * D0);
    for (int l = 0; l < 3; ++l) {
        FtEncS &s = w.enc[l];
        s.a1 = f(E * H); s.a2 = f(E * H); s.b1 = f(E * H); s.b2 = f(E * H); s.x3 = f(E * H); s.mu3 = f(E); s.rs3 = f(E);
        s.x1 = f(L * H); s.mu1 = f(L); s.rs1 = f(L); s.hV1 = f(L * H); s.fa = f(L * 4 * H); s.x2 = f(L * H); s.mu2 = f(L); s.rs2 = f(L);
        s.out = f(L * H);
    }
    for (int l = 0; l < 3; ++l) {
        FtDecS &s = w.dec[l];
        s.a1 = f(E * H); s.a2 = f(E * H);
        s.x1 = f(L * H); s.mu1 = f(L); s.rs1 = f(L); s.hV1 = f(L * H); s.fa = f(L * 4 * H); s.x2 = f(L * H); s.mu2 = f(L); s.rs2 = f(L);
        s.out = f(L * H);
    }
    w.head_bytes = seq ? 0 : tmpnn_head_train_workspace_bytes(M, n_layers >= 1 ? (int)(D0 / H - 1) : 0, lightattn, n_layers, dims);
    w.head_ws = sv.take<char>(w.head_bytes);
    if (seq) w.lp = f(L * TMPNN_VOCAB);
    if (split) { w.ftm = f(E * H); w.fdh = f(L * H); w.fdF = f(L * H); }
    // scratch
    w.cnt = ic(L + 1); w.cur = ic(L + 1); w.coff = ic(L + 1); w.clist = ic(E);
    w.mcnt = ic(L + 1); w.mcur = ic(L + 1); w.moff = ic(L + 1); w.mlist = ic(M); w.dheadX = fc(M * D0);
    w.tm = fc(E * H); w.t1 = fc(E * H); w.t2 = fc(E * H); w.dA = fc(E * 4 * H); w.dE = fc(E * H); w.dE2 = fc(E * H); w.dEd = fc(E * H);
    w.gx = fc(E * H); w.gb = fc(E * H); w.dEp = fc(E * 16);
    w.dV = fc(L * H); w.dV2 = fc(L * H); w.dh1 = fc(L * H); w.dF = fc(L * H); w.dhS = fc(L * H);
    for (int l = 0; l < 3; ++l) w.dH[l] = fc(L * H);
    w.dG = fc(L * 4 * H);
    const int64_t pe = std::max(ft_parts(E), ft_parts(L));
    w.P = fc(pe * std::max<int64_t>(H * (4 * H + 1), 4 * H * (H + 1)));
    w.CP = fc((int64_t)FT_CLS_PARTS * std::max<int64_t>(66 * 16, TMPNN_VOCAB * H));
    if (seq) { w.dlg = fc(L * TMPNN_VOCAB); w.dVe = fc(L * H); }
    if (split) {
        w.head_ws_b = sc.take<char>(w.head_bytes);
    } else {
        w.ftm = w.tm; w.fdh = w.dh1; w.fdF = w.dF;
        w.head_ws_b = w.head_ws;
    }
    w.saved_bytes = sv.used + (split ? 256 : 0);
    w.scratch_bytes = sc.used + 256;
    w.bytes = sv.used + sc.used + 256;
    return w;
}

// the fused entries' one workspace: the saved part, then the scratch part
static FtWs ft_carve(void *base, int64_t L, int64_t M, int lightattn, int n_layers, const int32_t *dims) {
    const FtWs sz = ft_carve2(nullptr, nullptr, false, L, M, lightattn, n_layers, dims);
    return ft_carve2(base, base ? (void *)((char *)base + sz.saved_bytes) : nullptr, false, L, M, lightattn, n_layers, dims);
}

static int ft_grid_items(int64_t wave_items) {
    const int64_t b = (wave_items + 3) / 4, cap = (int64_t)tm_num_cus() * 8;
    return (int)(b < 1 ? 1 : b < cap ? b : cap);
}
static int ft_grid_threads(int64_t n) {
    const int64_t b = (n + TM_THREADS - 1) / TM_THREADS, cap = (int64_t)tm_num_cus() * 8;
    return (int)(b < 1 ? 1 : b < cap ? b : cap);
}

// (One call's context, FtCtx: tmpnn_ft.h)
static FtSeg ft_seg(const float *p, int ld, int width, int mode, int masked, int rows) { return FtSeg{p, ld, width, mode, masked, rows, 0, nullptr}; }
static FtA ft_plain(const float *p, int ld, int width, int rows, int act = 0) {
    FtA a{};
    a.s[0] = ft_seg(p, ld, width, 0, 0, rows);
    a.n_seg = 1;
    a.K = 1;
    a.act = act;
    return a;
}

// Y [M, N] (ldy) (+)= A W^T + b, W [N, Ktot] row-major; G: gelu' gate
static void ft_linear(const FtCtx &c, const FtA &a, const float *W, const float *b, float *Y, int ldy, int M, int N, const float *G = nullptr,
                      int accum = 0) {
    int Kt = 0;
    for (int s = 0; s < a.n_seg; ++s) Kt += a.s[s].width;
    FtDense d{a, W, Kt, 1, b, Y, ldy, G, accum, M, N};
    ft_dense_kernel<<<ft_grid_items((int64_t)((M + 15) / 16) * ((N + 15) / 16)), TM_THREADS, 0, c.st>>>(d);
}
// dX [M, Kin] (+)= dY [M, N] W, W [N, Kin] (ld ldw) read transposed; G: gelu' gate of the result
static void ft_linear_t(const FtCtx &c, const float *dY, int ldd, const float *W, int ldw, float *dX, int ldx, int M, int N, int Kin,
                        const float *G = nullptr, int accum = 0) {
    FtDense d{ft_plain(dY, ldd, N, M), W, 1, ldw, nullptr, dX, ldx, G, accum, M, Kin};
    ft_dense_kernel<<<ft_grid_items((int64_t)((M + 15) / 16) * ((Kin + 15) / 16)), TM_THREADS, 0, c.st>>>(d);
}
// G [N, Ktot] = sum_m dY[m]^T A(m), Gb [N] = sum_m dY[m] (when Gb)
static void ft_wgrad(const FtCtx &c, const float *dY, int ldd, const FtA &a, int M, int N, float *G, float *Gb) {
    int Kt = 0;
    for (int s = 0; s < a.n_seg; ++s) Kt += a.s[s].width;
    const int parts = ft_parts(M), rpp = (((M + parts - 1) / parts) + 3) & ~3;
    FtWgrad w{dY, ldd, a, c.w.P, M, N, Kt, rpp, parts};
    ft_wgrad_kernel<<<ft_grid_items((int64_t)((N + 15) / 16) * ((Kt + 1 + 15) / 16) * parts), TM_THREADS, 0, c.st>>>(w);
    ft_wsum_kernel<<<ft_grid_threads((int64_t)N * (Kt + 1)), TM_THREADS, 0, c.st>>>(c.w.P, parts, N, Kt, G, Gb);
}
static void ft_class_sum(const FtCtx &c, const int32_t *cls, const float *src, int lds, int off, int R, int C, int ncls, float *dst, int ldc,
                         int ldd) {
    const int P = ft_cparts(R), rpp = (R + P - 1) / P;
    ft_class_part_kernel<<<ft_grid_threads((int64_t)P * ncls * C), TM_THREADS, 0, c.st>>>(cls, src, lds, off, R, C, ncls, P, rpp, c.w.CP);
    ft_class_fin_kernel<<<ft_grid_threads((int64_t)ncls * C), TM_THREADS, 0, c.st>>>(c.w.CP, P, ncls, C, dst, ldc, ldd);
}
static void ft_ln_fwd(const FtCtx &c, const float *base, const float *delta, int site, const float *g, const float *b, const float *omask,
                      float *xs, float *y, float *mu, float *rs, int64_t R) {
    FtLnF a{base, delta, site, g, b, omask, xs, y, mu, rs, (int)R, c.drop};
    a.d.keep_out = c.drop.keep_out;
    ft_ln_fwd_kernel<<<ft_grid_items(R), TM_THREADS, 0, c.st>>>(a);
}
// LayerNorm backward; the gamma / beta gradients go straight into the slab
static void ft_ln_bwd(const FtCtx &c, const float *dy, const float *omask, const float *xs, const float *mu, const float *rs, int64_t gofs,
                      int64_t bofs, float *dx, int accum, float *ddelta, int site, int64_t R) {
    FtLnB a{dy, omask, xs, mu, rs, c.params + gofs, dx, accum, ddelta, site, c.w.gx, c.w.gb, (int)R, c.drop};
    a.d.keep_out = nullptr;                      // masks are exported by the forward only
    ft_ln_bwd_kernel<<<ft_grid_items(R), TM_THREADS, 0, c.st>>>(a);
    ft_class_sum(c, nullptr, c.w.gx, FT_H, 0, (int)R, FT_H, 1, c.grads + gofs, 0, 1);
    ft_class_sum(c, nullptr, c.w.gb, FT_H, 0, (int)R, FT_H, 1, c.grads + bofs, 0, 1);
}
static void ft_collect(const FtCtx &c, float *out, const float *base, const float *src, int lds, int self, int nb, int masked, int vis = 0) {
    FtCollect a{out, base, src, lds, self, nb, masked, c.mask, c.w.coff, c.w.clist, c.L, c.K, c.ranks ? vis : 0, c.ranks};
    ft_collect_kernel<<<ft_grid_threads((int64_t)c.L * FT_H), TM_THREADS, 0, c.st>>>(a);
}
static void ft_csr(const FtCtx &c, const int32_t *keys, int n, int nbins, int32_t *cnt, int32_t *cur, int32_t *off, int32_t *list) {
    (void)hipMemsetAsync(cnt, 0, (size_t)(nbins + 1) * 4, c.st);
    if (n > 0) ft_csr_count_kernel<<<ft_grid_threads(n), TM_THREADS, 0, c.st>>>(keys, n, nbins, cnt);
    ft_csr_scan_kernel<<<1, TM_THREADS, 0, c.st>>>(cnt, nbins, off, cur);
    if (n > 0) ft_csr_fill_kernel<<<ft_grid_threads(n), TM_THREADS, 0, c.st>>>(keys, n, nbins, cur, list);
    ft_csr_sort_kernel<<<ft_grid_threads(nbins), TM_THREADS, 0, c.st>>>(off, nbins, list);
}

// the 3 edge-level inputs of a message: [h_V_i | h_E | h_V_j] (encoder), [h_V_i | h_E | h_S_j | h_V_j] x mask_i (decoder)
static FtA ft_msg_in(const FtCtx &c, const float *hV, const float *hE, const float *hS) {
    FtA a{};
    a.K = c.K;
    a.eidx = c.w.eidx;
    a.mask = c.mask;
    a.s[0] = ft_seg(hV, FT_H, FT_H, 1, 0, c.L);
    a.s[1] = ft_seg(hE, FT_H, FT_H, 0, hS ? 1 : 0, (int)c.E);
    if (hS) {
        a.s[2] = ft_seg(hS, FT_H, FT_H, 2, 1, c.L);
        a.s[3] = ft_seg(hV, FT_H, FT_H, 2, 1, c.L);
        a.n_seg = 4;
        if (c.ranks) {                            // the order-masked decoder: vis h_S_j | (vis ? h_V_j : h_V^enc_j)
            a.ranks = c.ranks;
            a.s[2].vis = 1;
            a.s[3].vis = 2;
            a.s[3].p2 = c.w.enc[2].out;
        }
    } else {
        a.s[2] = ft_seg(hV, FT_H, FT_H, 2, 0, c.L);
        a.n_seg = 3;
    }
    return a;
}

// three-layer message forward: a1 = W1 in + b1, a2 = W2 gelu(a1) + b2, out = W3 gelu(a2) + b3
static void ft_mlp3_fwd(const FtCtx &c, const FtA &in, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                        const float *b3, float *a1, float *a2, float *out) {
    const int E = (int)c.E;
    ft_linear(c, in, W1, b1, a1, FT_H, E, FT_H);
    ft_linear(c, ft_plain(a1, FT_H, FT_H, E, 2), W2, b2, a2, FT_H, E, FT_H);
    ft_linear(c, ft_plain(a2, FT_H, FT_H, E, 2), W3, b3, out, FT_H, E, FT_H);
}
// its backward from dout [E,128]: weight gradients, then dIn [E, width(in)] into c.w.dA
static void ft_mlp3_bwd(const FtCtx &c, const FtA &in, const float *dout, int64_t oW1, int64_t ob1, int64_t oW2, int64_t ob2, int64_t oW3,
                        int64_t ob3, const float *a1, const float *a2) {
    const int E = (int)c.E;
    int Kin = 0;
    for (int s = 0; s < in.n_seg; ++s) Kin += in.s[s].width;
    ft_wgrad(c, dout, FT_H, ft_plain(a2, FT_H, FT_H, E, 2), E, FT_H, c.grads + oW3, c.grads + ob3);
    ft_linear_t(c, dout, FT_H, c.params + oW3, FT_H, c.w.t1, FT_H, E, FT_H, FT_H, a2);            // d a2
    ft_wgrad(c, c.w.t1, FT_H, ft_plain(a1, FT_H, FT_H, E, 2), E, FT_H, c.grads + oW2, c.grads + ob2);
    ft_linear_t(c, c.w.t1, FT_H, c.params + oW2, FT_H, c.w.t2, FT_H, E, FT_H, FT_H, a1);          // d a1
    ft_wgrad(c, c.w.t2, FT_H, in, E, FT_H, c.grads + oW1, c.grads + ob1);
    ft_linear_t(c, c.w.t2, FT_H, c.params + oW1, Kin, c.w.dA, Kin, E, FT_H, Kin);                 // d in
}

// node update after the message: hV1 = LN1(hV + drop(dh)), out = mask LN2(hV1 + drop(W_out gelu(W_in hV1 + b_in) + b_out))
static void ft_node_fwd(const FtCtx &c, const float *hV, const float *dh, int site1, int site2, const float *n1w, const float *n1b,
                        const float *Win, const float *bin, const float *Wout, const float *bout, const float *n2w, const float *n2b,
                        float *x1, float *mu1, float *rs1, float *hV1, float *fa, float *x2, float *mu2, float *rs2, float *out) {
    const int L = c.L;
    ft_ln_fwd(c, hV, dh, site1, n1w, n1b, nullptr, x1, hV1, mu1, rs1, L);
    ft_linear(c, ft_plain(hV1, FT_H, FT_H, L), Win, bin, fa, 4 * FT_H, L, 4 * FT_H);
    ft_linear(c, ft_plain(fa, 4 * FT_H, 4 * FT_H, L, 2), Wout, bout, c.w.fdF, FT_H, L, FT_H);
    ft_ln_fwd(c, hV1, c.w.fdF, site2, n2w, n2b, c.mask, x2, out, mu2, rs2, L);
}
// its backward: dout (grad of out) -> c.w.dV2 = grad of hV (residual path only) and c.w.dh1 = grad of dh (after dropout1's backward)
static void ft_node_bwd(const FtCtx &c, const float *dout, int site1, int site2, int64_t on1w, int64_t on1b, int64_t oWin, int64_t obin,
                        int64_t oWout, int64_t obout, int64_t on2w, int64_t on2b, const float *x1, const float *mu1, const float *rs1,
                        const float *hV1, const float *fa, const float *x2, const float *mu2, const float *rs2) {
    const int L = c.L;
    float *dhV1 = c.w.dV2, *dF = c.w.dF;
    ft_ln_bwd(c, dout, c.mask, x2, mu2, rs2, on2w, on2b, dhV1, 0, dF, site2, L);
    ft_wgrad(c, dF, FT_H, ft_plain(fa, 4 * FT_H, 4 * FT_H, L, 2), L, FT_H, c.grads + oWout, c.grads + obout);
    ft_linear_t(c, dF, FT_H, c.params + oWout, 4 * FT_H, c.w.dG, 4 * FT_H, L, FT_H, 4 * FT_H, fa);   // d fa
    ft_wgrad(c, c.w.dG, 4 * FT_H, ft_plain(hV1, FT_H, FT_H, L), L, 4 * FT_H, c.grads + oWin, c.grads + obin);
    ft_linear_t(c, c.w.dG, 4 * FT_H, c.params + oWin, FT_H, dhV1, FT_H, L, 4 * FT_H, FT_H, nullptr, 1);
    ft_ln_bwd(c, dhV1, nullptr, x1, mu1, rs1, on1w, on1b, dhV1, 0, c.w.dh1, site1, L);
}

int ft_forward(const FtCtx &c) {
    const FtWs &w = c.w;
    const FtLayout &S = c.lay;
    const float *P = c.params;
    const int L = c.L, E = (int)c.E;
    ft_embed_kernel<<<ft_grid_threads((int64_t)L * FT_H), TM_THREADS, 0, c.st>>>(P + S.Ws, c.S, L, w.hS);
    if (c.nf > 0) {
        // the segments of the row space: one protein [0, L], or what the packed entry has written into w.offs from its caller's offsets
        if (!c.seg_offsets) ft_offsets_kernel<<<1, TM_THREADS, 0, c.st>>>(w.offs, L);
        FT_TRY(launch_knn(c.X, c.mask, w.offs, c.n_prot, L, c.max_len, c.K, w.E48, w.D48, c.status ? c.status : w.status, c.st));
        FtGraph g{c.X, c.ridx, c.cenc, w.E48, w.D48, P + S.posw, P + S.posb, w.eidx, w.cls, w.Ein, L, c.K, w.offs, c.n_prot};
        ft_graph_kernel<<<ft_grid_threads(E), TM_THREADS, 0, c.st>>>(g);
        ft_linear(c, ft_plain(w.Ein, 416, 416, E), P + S.edgew, nullptr, w.E0, FT_H, E, FT_H);
        FtLnF ln{w.E0, nullptr, 0, P + S.new_, P + S.neb, nullptr, w.ftm, w.En, w.nemu, w.ners, E, c.drop};   // xs = E0 again (temporary)
        ln.d.mode = 0;
        ft_ln_fwd_kernel<<<ft_grid_items(E), TM_THREADS, 0, c.st>>>(ln);
        ft_linear(c, ft_plain(w.En, FT_H, FT_H, E), P + S.Wew, P + S.Web, w.hE[0], FT_H, E, FT_H);
        (void)hipMemsetAsync(w.hV0, 0, (size_t)L * FT_H * 4, c.st);
        const float *hV = w.hV0;
        for (int l = 0; l < 3; ++l) {
            const FtEncP &p = S.enc[l];
            const FtEncS &s = w.enc[l];
            ft_mlp3_fwd(c, ft_msg_in(c, hV, w.hE[l], nullptr), P + p.W1, P + p.b1, P + p.W2, P + p.b2, P + p.W3, P + p.b3, s.a1, s.a2, w.ftm);
            ft_msg_sum_kernel<<<ft_grid_threads((int64_t)L * FT_H), TM_THREADS, 0, c.st>>>(w.ftm, c.mask, w.eidx, 1, L, c.K, w.fdh);
            ft_node_fwd(c, hV, w.fdh, 3 * l, 3 * l + 1, P + p.n1w, P + p.n1b, P + p.Win, P + p.bin, P + p.Wout, P + p.bout, P + p.n2w, P + p.n2b,
                        s.x1, s.mu1, s.rs1, s.hV1, s.fa, s.x2, s.mu2, s.rs2, s.out);
            ft_mlp3_fwd(c, ft_msg_in(c, s.out, w.hE[l], nullptr), P + p.W11, P + p.b11, P + p.W12, P + p.b12, P + p.W13, P + p.b13, s.b1, s.b2,
                        w.ftm);
            ft_ln_fwd(c, w.hE[l], w.ftm, 3 * l + 2, P + p.n3w, P + p.n3b, nullptr, s.x3, w.hE[l + 1], s.mu3, s.rs3, E);
            hV = s.out;
        }
        for (int l = 0; l < 3; ++l) {
            const FtDecP &p = S.dec[l];
            const FtDecS &s = w.dec[l];
            ft_mlp3_fwd(c, ft_msg_in(c, hV, w.hE[3], w.hS), P + p.W1, P + p.b1, P + p.W2, P + p.b2, P + p.W3, P + p.b3, s.a1, s.a2, w.ftm);
            ft_msg_sum_kernel<<<ft_grid_threads((int64_t)L * FT_H), TM_THREADS, 0, c.st>>>(w.ftm, c.mask, w.eidx, 0, L, c.K, w.fdh);
            ft_node_fwd(c, hV, w.fdh, 9 + 2 * l, 10 + 2 * l, P + p.n1w, P + p.n1b, P + p.Win, P + p.bin, P + p.Wout, P + p.bout, P + p.n2w,
                        P + p.n2b, s.x1, s.mu1, s.rs1, s.hV1, s.fa, s.x2, s.mu2, s.rs2, s.out);
            hV = s.out;
        }
    }
    if (c.seq) {                                  // logits = W_out h_V + b, log_probs = log_softmax(logits) (kept for the backward)
        ft_linear(c, ft_plain(w.dec[2].out, FT_H, FT_H, L), P + S.Wo, P + S.bo, w.lp, TMPNN_VOCAB, L, TMPNN_VOCAB);
        sq_logsoftmax_kernel<<<ft_grid_threads(L), TM_THREADS, 0, c.st>>>(w.lp, L);
        return TMPNN_OK;
    }
    FtHeadRows hr{{w.dec[0].out, w.dec[1].out, w.dec[2].out}, w.hS, c.pos, w.headX, w.rows_id, c.M, L, c.nf};
    ft_head_rows_kernel<<<ft_grid_threads((int64_t)c.M * FT_H * (c.nf + 1)), TM_THREADS, 0, c.st>>>(hr);
    return TMPNN_OK;
}

void ft_backward(const FtCtx &c) {
    const FtWs &w = c.w;
    const FtLayout &S = c.lay;
    const int L = c.L, E = (int)c.E;
    if (c.seq) {
        // the seed: dlogits = dlp - softmax sum(dlp); W_out's gradients; d h_V^dec3 = dlogits W_out. Nothing else reaches h_S or the
        // earlier decoder outputs from outside, and the encoder output's own gradient starts at 0.
        sq_dlogits_kernel<<<ft_grid_threads(L), TM_THREADS, 0, c.st>>>(c.dlp, w.lp, L, w.dlg);
        ft_wgrad(c, w.dlg, TMPNN_VOCAB, ft_plain(w.dec[2].out, FT_H, FT_H, L), L, TMPNN_VOCAB, c.grads + S.Wo, c.grads + S.bo);
        ft_linear_t(c, w.dlg, TMPNN_VOCAB, c.params + S.Wo, FT_H, w.dH[2], FT_H, L, TMPNN_VOCAB, FT_H);
        for (float *z : {w.dH[0], w.dH[1], w.dhS, w.dVe}) (void)hipMemsetAsync(z, 0, (size_t)L * FT_H * 4, c.st);
    } else {
        ft_csr(c, c.pos, c.M, L, w.mcnt, w.mcur, w.moff, w.mlist);
        FtHeadScatter hs{w.dheadX, w.moff, w.mlist, {w.dH[0], w.dH[1], w.dH[2]}, w.dhS, L, c.nf};
        ft_head_scatter_kernel<<<ft_grid_threads((int64_t)L * FT_H * (c.nf + 1)), TM_THREADS, 0, c.st>>>(hs);
    }
    if (c.nf > 0) {
        for (int l = 0; l < 3; ++l)                   // the decoder outputs the head does not read get no gradient from it
            if (l < 3 - c.nf) (void)hipMemsetAsync(w.dH[l], 0, (size_t)L * FT_H * 4, c.st);
        ft_csr(c, w.eidx, E, L, w.cnt, w.cur, w.coff, w.clist);
        (void)hipMemsetAsync(w.dEd, 0, (size_t)E * FT_H * 4, c.st);
        // dV: the gradient of the current layer's output
        (void)hipMemcpyAsync(w.dV, w.dH[2], (size_t)L * FT_H * 4, hipMemcpyDeviceToDevice, c.st);
        for (int l = 2; l >= 0; --l) {
            const FtDecP &p = S.dec[l];
            const FtDecS &s = w.dec[l];
            const float *hVin = l > 0 ? w.dec[l - 1].out : w.enc[2].out;
            ft_node_bwd(c, w.dV, 9 + 2 * l, 10 + 2 * l, p.n1w, p.n1b, p.Win, p.bin, p.Wout, p.bout, p.n2w, p.n2b, s.x1, s.mu1, s.rs1, s.hV1,
                        s.fa, s.x2, s.mu2, s.rs2);
            ft_msg_expand_kernel<<<ft_grid_threads((int64_t)E * FT_H), TM_THREADS, 0, c.st>>>(w.dh1, c.mask, w.eidx, 0, L, c.K, w.tm);
            const FtA in = ft_msg_in(c, hVin, w.hE[3], w.hS);
            ft_mlp3_bwd(c, in, w.tm, p.W1, p.b1, p.W2, p.b2, p.W3, p.b3, s.a1, s.a2);
            // dA = [d hV_i | d h_E | d h_S_j | d h_V_j] (the last three before the mask_i factor)
            ft_edge_add_kernel<<<ft_grid_threads((int64_t)E * FT_H), TM_THREADS, 0, c.st>>>(w.dEd, nullptr, w.dA, 4 * FT_H, FT_H, c.mask, 1, E, c.K);
            // under an order (c.ranks): d h_S_j and the layer's d h_V_j take the visible edges only; d h_V_j of an invisible edge
            // belongs to the encoder output and is summed into dVe, layer 2 first, then 1, then 0
            ft_collect(c, w.dhS, w.dhS, w.dA, 4 * FT_H, -1, 2 * FT_H, 1, 1);
            // grad of the layer input = residual + self + neighbour terms (+ the head's, for an earlier decoder layer)
            ft_collect(c, w.dV2, w.dV2, w.dA, 4 * FT_H, 0, -1, 0);
            ft_collect(c, w.dV, w.dV2, w.dA, 4 * FT_H, -1, 3 * FT_H, 1, 1);
            if (c.ranks) ft_collect(c, w.dVe, w.dVe, w.dA, 4 * FT_H, -1, 3 * FT_H, 1, 2);
            if (l > 0) ft_edge_add_kernel<<<ft_grid_threads((int64_t)L * FT_H), TM_THREADS, 0, c.st>>>(w.dV, nullptr, w.dH[l - 1], FT_H, 0, c.mask, 0, L, 1);
        }
        // encoder: dV = grad of the encoder output, dE = grad of h_E after the last encoder layer
        if (c.ranks) ft_edge_add_kernel<<<ft_grid_threads((int64_t)L * FT_H), TM_THREADS, 0, c.st>>>(w.dV, nullptr, w.dVe, FT_H, 0, c.mask, 0, L, 1);
        (void)hipMemcpyAsync(w.dE, w.dEd, (size_t)E * FT_H * 4, hipMemcpyDeviceToDevice, c.st);
        for (int l = 2; l >= 0; --l) {
            const FtEncP &p = S.enc[l];
            const FtEncS &s = w.enc[l];
            const float *hVin = l > 0 ? w.enc[l - 1].out : w.hV0;
            // edge update: h_E' = LN3(h_E + drop3(W13 gelu(W12 gelu(W11 [out_i | h_E | out_j]))))
            ft_ln_bwd(c, w.dE, nullptr, s.x3, s.mu3, s.rs3, p.n3w, p.n3b, w.dE2, 0, w.tm, 3 * l + 2, E);
            const FtA ein = ft_msg_in(c, s.out, w.hE[l], nullptr);
            ft_mlp3_bwd(c, ein, w.tm, p.W11, p.b11, p.W12, p.b12, p.W13, p.b13, s.b1, s.b2);
            ft_edge_add_kernel<<<ft_grid_threads((int64_t)E * FT_H), TM_THREADS, 0, c.st>>>(w.dE, w.dE2, w.dA, 3 * FT_H, FT_H, c.mask, 0, E, c.K);
            ft_collect(c, w.dV2, w.dV, w.dA, 3 * FT_H, 0, 2 * FT_H, 0);
            (void)hipMemcpyAsync(w.dV, w.dV2, (size_t)L * FT_H * 4, hipMemcpyDeviceToDevice, c.st);
            // node update and message
            ft_node_bwd(c, w.dV, 3 * l, 3 * l + 1, p.n1w, p.n1b, p.Win, p.bin, p.Wout, p.bout, p.n2w, p.n2b, s.x1, s.mu1, s.rs1, s.hV1, s.fa,
                        s.x2, s.mu2, s.rs2);
            ft_msg_expand_kernel<<<ft_grid_threads((int64_t)E * FT_H), TM_THREADS, 0, c.st>>>(w.dh1, c.mask, w.eidx, 1, L, c.K, w.tm);
            const FtA min_ = ft_msg_in(c, hVin, w.hE[l], nullptr);
            ft_mlp3_bwd(c, min_, w.tm, p.W1, p.b1, p.W2, p.b2, p.W3, p.b3, s.a1, s.a2);
            ft_edge_add_kernel<<<ft_grid_threads((int64_t)E * FT_H), TM_THREADS, 0, c.st>>>(w.dE, nullptr, w.dA, 3 * FT_H, FT_H, c.mask, 0, E, c.K);
            if (l > 0) ft_collect(c, w.dV, w.dV2, w.dA, 3 * FT_H, 0, 2 * FT_H, 0);
        }
        // h_E0 = W_e LN(edge_embedding(Ein)) + b_e
        ft_wgrad(c, w.dE, FT_H, ft_plain(w.En, FT_H, FT_H, E), E, FT_H, c.grads + S.Wew, c.grads + S.Web);
        ft_linear_t(c, w.dE, FT_H, c.params + S.Wew, FT_H, w.dE2, FT_H, E, FT_H, FT_H);
        ft_ln_bwd(c, w.dE2, nullptr, w.E0, w.nemu, w.ners, S.new_, S.neb, w.t1, 0, nullptr, 0, E);
        ft_wgrad(c, w.t1, FT_H, ft_plain(w.Ein, 416, 416, E), E, FT_H, c.grads + S.edgew, nullptr);
        ft_linear_t(c, w.t1, FT_H, c.params + S.edgew, 416, w.dEp, 16, E, FT_H, 16);             // d E_pos = dE0 W_edge[:, :16]
        ft_class_sum(c, w.cls, w.dEp, 16, 0, E, 16, 66, c.grads + S.posw, 1, 66);                  // d W_pos[d, class]
        ft_class_sum(c, nullptr, w.dEp, 16, 0, E, 16, 1, c.grads + S.posb, 0, 1);
        if (c.dX) {
            // d RBF = dE0 W_edge[:, 16:416] into dA (dead after the encoder loop); tmpnn_coordgrad.hip takes it to dX through tm (dead too)
            ft_linear_t(c, w.t1, FT_H, c.params + S.edgew + 16, 416, w.dA, 400, E, FT_H, 400);
            ft_coord_grad(c, w.dA);
        }
    } else if (c.dX) {
        (void)hipMemsetAsync(c.dX, 0, (size_t)L * 12 * 4, c.st);     // no ProteinMPNN layer: the head never reads the structure
    }
    ft_class_sum(c, c.S, w.dhS, FT_H, 0, L, FT_H, TMPNN_VOCAB, c.grads + S.Ws, FT_H, 1);        // d W_s[a] = sum over S_i = a
}

// keep_in / keep_out of L rows at K neighbours: the 15 sites in order, each [rows, 128] (one protein: K = min(48, L), whatever k_neighbors)
int64_t ft_mask_numel(int64_t L, int64_t K) { return (12 * L + 3 * L * K) * FT_H; }
static int64_t ft_k48(int64_t L) { return L < TM_KS ? L : TM_KS; }
static int64_t ft_mask_numel(int64_t L) { return ft_mask_numel(L, ft_k48(L)); }

static void ft_mask_offsets(int64_t L, int64_t K, int64_t *off) {
    const int64_t node = L * FT_H, edge = L * K * FT_H;
    int64_t o = 0;
    for (int s = 0; s < FT_SITES; ++s) {
        off[s] = o;
        o += (s < 9 && s % 3 == 2) ? edge : node;
    }
}

extern "C" int64_t tmpnn_finetune_slab_numel(int n_final, int lightattn, int n_layers, const int32_t *dims) {
    if (!ft_dims_ok(n_final, n_layers, dims)) return -1;
    return ft_layout(n_final).head + tmpnn_head_slab_numel(n_final, lightattn, n_layers, dims);
}

extern "C" int64_t tmpnn_finetune_mask_numel(int64_t L) { return L < 2 || L > FT_L_MAX ? -1 : ft_mask_numel(L); }

extern "C" size_t tmpnn_finetune_workspace_bytes(int64_t L, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims) {
    if (L < 2 || L > FT_L_MAX || M < 1 || M > FT_M_MAX || !ft_dims_ok(n_final, n_layers, dims)) return 0;
    return ft_carve(nullptr, L, M, lightattn, n_layers, dims).bytes;
}

static int ft_check(const char *what, const float *X, const int32_t *S, const float *mask, const int32_t *ridx, const int32_t *cenc, int64_t L,
                    const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn, int n_layers,
                    const int32_t *dims, const float *params, int64_t slab_numel) {
    FT_REQUIRE(ft_dims_ok(n_final, n_layers, dims),
               "%s: dims must run from 128 * num_final_layers + 128 to 21 over 1..8 layers (num_final_layers 0..3)", what);
    FT_REQUIRE(L >= 2 && L <= FT_L_MAX, "%s: protein length %lld outside [2, %lld]", what, (long long)L, (long long)FT_L_MAX);
    FT_REQUIRE(M >= 1 && M <= FT_M_MAX, "%s: bad number of mutants %lld", what, (long long)M);
    const int64_t need_slab = tmpnn_finetune_slab_numel(n_final, lightattn, n_layers, dims);
    FT_REQUIRE(slab_numel == need_slab, "%s: parameter slab holds %lld floats, this model needs %lld", what, (long long)slab_numel,
               (long long)need_slab);
    FT_REQUIRE(X && S && mask && ridx && cenc && pos && mut && wt && params, "%s: null pointer", what);
    return TMPNN_OK;
}

static int ft_check_ws(const char *what, int64_t L, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims, void *workspace,
                       size_t workspace_bytes) {
    const size_t need = tmpnn_finetune_workspace_bytes(L, M, n_final, lightattn, n_layers, dims);
    if (!workspace || workspace_bytes < need)
        return tm_set_error(TMPNN_E_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    return TMPNN_OK;
}

static FtCtx ft_ctx(const float *X, const int32_t *S, const float *mask, const int32_t *ridx, const int32_t *cenc, int64_t L, const int32_t *pos,
                    const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims,
                    int subtract, const float *params, float *grads, void *ws, hipStream_t st) {
    FtCtx c{};
    c.L = (int)L;
    c.K = (int)ft_k48(L);
    c.n_prot = 1;
    c.min_len = c.max_len = c.L;
    c.E = (int64_t)c.L * c.K;
    c.M = (int)M;
    c.nf = n_final;
    c.lightattn = lightattn;
    c.n_layers = n_layers;
    c.subtract = subtract;
    c.dims = dims;
    c.X = X; c.S = S; c.mask = mask; c.ridx = ridx; c.cenc = cenc; c.pos = pos; c.mut = mut; c.wt = wt;
    c.params = params;
    c.grads = grads;
    c.lay = ft_layout(n_final);
    c.w = ft_carve(ws, L, M, lightattn, n_layers, dims);
    c.st = st;
    return c;
}

// ProteinMPNN's dropout of one call: the injected masks (keep_in), the stated generator keyed on (seed, step) when p > 0, else none
void ft_set_drop(FtCtx &c, int64_t L, int64_t K, float p_mpnn, const float *keep_in, float *keep_out, uint64_t seed, uint64_t step) {
    const uint32_t thr = (uint32_t)llround((double)p_mpnn * 16777216.0);
    c.drop.mode = keep_in ? 1 : thr > 0 ? 2 : 0;
    c.drop.keep_in = keep_in;
    c.drop.keep_out = c.drop.mode == 2 ? keep_out : nullptr;
    c.drop.thr = thr;
    c.drop.scale = (float)(1.0 / (1.0 - (double)thr / 16777216.0));
    ft_mask_offsets(L, K, c.drop.off);
    {   // k2 of the stated generator, formed on the host in the same 64-bit arithmetic
        auto mix = [](uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x; };
        c.drop.k2 = mix(mix(seed ^ 0x9E3779B97F4A7C15ull) + step);
    }
}

extern "C" int tmpnn_finetune_step(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                   int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, const float *target, int64_t M,
                                   int n_final, int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params,
                                   float *grads, int64_t slab_numel, float p_mpnn, float p_head, const float *keep_in, float *keep_out,
                                   const float *head_keep_in, uint64_t seed, uint64_t step, float *loss, float *pred_opt,
                                   int32_t *E_idx_opt, float *rows_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    FT_TRY(ft_check("finetune_step", X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, params,
                    slab_numel));
    FT_REQUIRE(target && grads && loss, "finetune_step: null pointer");
    FT_REQUIRE(p_mpnn >= 0.f && p_mpnn < 1.f && p_head >= 0.f && p_head < 1.f, "finetune_step: dropout probability outside [0, 1)");
    FT_REQUIRE(!(keep_in && keep_out), "finetune_step: keep_in (injected masks) and keep_out (drawn masks) exclude each other");
    FT_REQUIRE(lightattn || (p_head == 0.f && !head_keep_in), "finetune_step: head dropout needs LightAttention (lightattn)");
    FT_REQUIRE(!(E_idx_opt || keep_in || keep_out) || n_final > 0, "finetune_step: num_final_layers 0 runs no ProteinMPNN layer");
    FT_TRY(ft_check_ws("finetune_step", L, M, n_final, lightattn, n_layers, dims, workspace, workspace_bytes));
    FtCtx c = ft_ctx(X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, subtract_mut, params, grads,
                     workspace, (hipStream_t)stream);
    ft_set_drop(c, L, ft_k48(L), p_mpnn, keep_in, keep_out, seed, step);
    if (keep_out && c.drop.mode != 2) (void)hipMemsetAsync(keep_out, 0, (size_t)ft_mask_numel(L) * 4, c.st);
    FT_TRY(ft_forward(c));
    const int64_t D0 = dims[0];
    const int rc = tm_head_train_core(c.w.headX, M, c.w.rows_id, mut, wt, target, M, lightattn, n_layers, dims, subtract_mut,
                                      params + c.lay.head, grads + c.lay.head, p_head, head_keep_in, nullptr, seed, step, loss, pred_opt,
                                      c.w.head_ws, c.st, c.w.dheadX, nullptr);
    if (rc != TMPNN_OK) return rc;
    ft_backward(c);
    if (E_idx_opt) (void)hipMemcpyAsync(E_idx_opt, c.w.eidx, (size_t)c.E * 4, hipMemcpyDeviceToDevice, c.st);
    if (rows_opt) (void)hipMemcpyAsync(rows_opt, c.w.headX, (size_t)M * D0 * 4, hipMemcpyDeviceToDevice, c.st);
    return tm_check_launch("finetune_step");
}

extern "C" int tmpnn_finetune_eval(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                   int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn,
                                   int n_layers, const int32_t *dims, int subtract_mut, const float *params, int64_t slab_numel, float *pred,
                                   int32_t *E_idx_opt, float *rows_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    FT_TRY(ft_check("finetune_eval", X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, params,
                    slab_numel));
    FT_REQUIRE(pred, "finetune_eval: null pointer");
    FT_REQUIRE(!E_idx_opt || n_final > 0, "finetune_eval: num_final_layers 0 builds no graph");
    FT_TRY(ft_check_ws("finetune_eval", L, M, n_final, lightattn, n_layers, dims, workspace, workspace_bytes));
    FtCtx c = ft_ctx(X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, subtract_mut, params, nullptr,
                     workspace, (hipStream_t)stream);
    ft_mask_offsets(L, ft_k48(L), c.drop.off);
    FT_TRY(ft_forward(c));
    FT_TRY(tmpnn_head_eval(c.w.headX, M, c.w.rows_id, mut, wt, M, n_final, lightattn, n_layers, dims, subtract_mut, params + c.lay.head,
                           slab_numel - c.lay.head, pred, c.w.head_ws, c.w.head_bytes, stream));
    if (E_idx_opt) (void)hipMemcpyAsync(E_idx_opt, c.w.eidx, (size_t)c.E * 4, hipMemcpyDeviceToDevice, c.st);
    if (rows_opt) (void)hipMemcpyAsync(rows_opt, c.w.headX, (size_t)M * dims[0] * 4, hipMemcpyDeviceToDevice, c.st);
    return tm_check_launch("finetune_eval");
}

// ---- the step split in two: forward into a saved buffer, backward from any dL / dpred ---------------------------------------------
extern "C" size_t tmpnn_finetune_saved_bytes(int64_t L, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims) {
    if (L < 2 || L > FT_L_MAX || M < 1 || M > FT_M_MAX || !ft_dims_ok(n_final, n_layers, dims)) return 0;
    return ft_carve2(nullptr, nullptr, true, L, M, lightattn, n_layers, dims).saved_bytes;
}

extern "C" size_t tmpnn_finetune_scratch_bytes(int64_t L, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims) {
    if (L < 2 || L > FT_L_MAX || M < 1 || M > FT_M_MAX || !ft_dims_ok(n_final, n_layers, dims)) return 0;
    return ft_carve2(nullptr, nullptr, true, L, M, lightattn, n_layers, dims).scratch_bytes;
}

static int ft_check_split(const char *what, int n_final, int lightattn, float p_mpnn, float p_head, const float *keep_in,
                          const float *head_keep_in) {
    FT_REQUIRE(p_mpnn >= 0.f && p_mpnn < 1.f && p_head >= 0.f && p_head < 1.f, "%s: dropout probability outside [0, 1)", what);
    FT_REQUIRE(lightattn || (p_head == 0.f && !head_keep_in), "%s: head dropout needs LightAttention (lightattn)", what);
    FT_REQUIRE(!keep_in || n_final > 0, "%s: num_final_layers 0 runs no ProteinMPNN layer", what);
    return TMPNN_OK;
}

int ft_check_buf(const char *what, const char *which, void *buf, size_t bytes, size_t need) {
    if (!buf || bytes < need) return tm_set_error(TMPNN_E_WORKSPACE, "%s: %s buffer %zu < %zu bytes", what, which, bytes, need);
    return TMPNN_OK;
}

extern "C" int tmpnn_finetune_forward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                      int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn,
                                      int n_layers, const int32_t *dims, int subtract_mut, const float *params, int64_t slab_numel, float p_mpnn,
                                      float p_head, const float *keep_in, float *keep_out, const float *head_keep_in, uint64_t seed, uint64_t step,
                                      float *pred, int32_t *E_idx_opt, float *rows_opt, void *saved, size_t saved_bytes, tmpnn_stream_t stream) {
    FT_TRY(ft_check("finetune_forward", X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, params,
                    slab_numel));
    FT_REQUIRE(pred, "finetune_forward: null pointer");
    FT_TRY(ft_check_split("finetune_forward", n_final, lightattn, p_mpnn, p_head, keep_in, head_keep_in));
    FT_REQUIRE(!(keep_in && keep_out), "finetune_forward: keep_in (injected masks) and keep_out (drawn masks) exclude each other");
    FT_REQUIRE(!(E_idx_opt || keep_out) || n_final > 0, "finetune_forward: num_final_layers 0 runs no ProteinMPNN layer");
    FT_TRY(ft_check_buf("finetune_forward", "saved", saved, saved_bytes,
                        tmpnn_finetune_saved_bytes(L, M, n_final, lightattn, n_layers, dims)));
    FtCtx c = ft_ctx(X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, subtract_mut, params, nullptr,
                     nullptr, (hipStream_t)stream);
    c.w = ft_carve2(saved, nullptr, true, L, M, lightattn, n_layers, dims);
    ft_set_drop(c, L, ft_k48(L), p_mpnn, keep_in, keep_out, seed, step);
    if (keep_out && c.drop.mode != 2) (void)hipMemsetAsync(keep_out, 0, (size_t)ft_mask_numel(L) * 4, c.st);
    FT_TRY(ft_forward(c));
    FT_TRY(tm_head_forward(c.w.headX, M, c.w.rows_id, mut, wt, M, lightattn, n_layers, dims, subtract_mut, params + c.lay.head, p_head,
                           head_keep_in, nullptr, seed, step, pred, c.w.head_ws, c.st));
    if (E_idx_opt) (void)hipMemcpyAsync(E_idx_opt, c.w.eidx, (size_t)c.E * 4, hipMemcpyDeviceToDevice, c.st);
    if (rows_opt) (void)hipMemcpyAsync(rows_opt, c.w.headX, (size_t)M * dims[0] * 4, hipMemcpyDeviceToDevice, c.st);
    return tm_check_launch("finetune_forward");
}

// both backwards of the split step: what = "finetune_backward" (dX null) or "finetune_backward_x" (dX [L,4,3], written whole)
static int ft_backward_entry(const char *what, bool want_dx, const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                             const int32_t *chain_enc, int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M,
                             int n_final, int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params,
                             int64_t slab_numel, float p_mpnn, float p_head, const float *keep_in, const float *head_keep_in, uint64_t seed,
                             uint64_t step, const float *dpred, float *grads, float *dX, int mpnn_grads, const void *saved, size_t saved_bytes,
                             void *scratch, size_t scratch_bytes, tmpnn_stream_t stream) {
    FT_TRY(ft_check(what, X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, params, slab_numel));
    FT_REQUIRE(dpred && grads, "%s: null pointer", what);
    if (want_dx) {
        FT_REQUIRE(dX, "%s: dX is null (tmpnn_finetune_backward is the entry without it)", what);
        FT_REQUIRE(mpnn_grads, "%s: dX needs the ProteinMPNN backward (mpnn_grads = 1)", what);
    }
    FT_TRY(ft_check_split(what, n_final, lightattn, p_mpnn, p_head, keep_in, head_keep_in));
    FT_TRY(ft_check_buf(what, "saved", (void *)saved, saved_bytes, tmpnn_finetune_saved_bytes(L, M, n_final, lightattn, n_layers, dims)));
    FT_TRY(ft_check_buf(what, "scratch", scratch, scratch_bytes, tmpnn_finetune_scratch_bytes(L, M, n_final, lightattn, n_layers, dims)));
    FtCtx c = ft_ctx(X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims, subtract_mut, params, grads,
                     nullptr, (hipStream_t)stream);
    // the saved part is only read: its one writer is the forward
    c.w = ft_carve2(const_cast<void *>(saved), scratch, true, L, M, lightattn, n_layers, dims);
    c.dX = dX;
    ft_set_drop(c, L, ft_k48(L), p_mpnn, keep_in, nullptr, seed, step);
    FT_TRY(tm_head_train_core(c.w.headX, M, c.w.rows_id, mut, wt, nullptr, M, lightattn, n_layers, dims, subtract_mut, params + c.lay.head,
                              grads + c.lay.head, p_head, head_keep_in, nullptr, seed, step, nullptr, nullptr, c.w.head_ws_b, c.st,
                              mpnn_grads ? c.w.dheadX : nullptr, dpred));
    if (mpnn_grads) ft_backward(c);
    return tm_check_launch(what);
}

extern "C" int tmpnn_finetune_backward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                       int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn,
                                       int n_layers, const int32_t *dims, int subtract_mut, const float *params, int64_t slab_numel, float p_mpnn,
                                       float p_head, const float *keep_in, const float *head_keep_in, uint64_t seed, uint64_t step,
                                       const float *dpred, float *grads, int mpnn_grads, const void *saved, size_t saved_bytes, void *scratch,
                                       size_t scratch_bytes, tmpnn_stream_t stream) {
    return ft_backward_entry("finetune_backward", false, X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers, dims,
                             subtract_mut, params, slab_numel, p_mpnn, p_head, keep_in, head_keep_in, seed, step, dpred, grads, nullptr,
                             mpnn_grads, saved, saved_bytes, scratch, scratch_bytes, stream);
}

extern "C" int tmpnn_finetune_backward_x(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                                         const int32_t *chain_enc, int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M,
                                         int n_final, int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params,
                                         int64_t slab_numel, float p_mpnn, float p_head, const float *keep_in, const float *head_keep_in,
                                         uint64_t seed, uint64_t step, const float *dpred, float *grads, float *dX, int mpnn_grads,
                                         const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream) {
    return ft_backward_entry("finetune_backward_x", true, X, S, mask, residue_idx, chain_enc, L, pos, mut, wt, M, n_final, lightattn, n_layers,
                             dims, subtract_mut, params, slab_numel, p_mpnn, p_head, keep_in, head_keep_in, seed, step, dpred, grads, dX,
                             mpnn_grads, saved, saved_bytes, scratch, scratch_bytes, stream);
}

// ---- the sequence loss: log p(S | X) under a decoding order, and its gradient ------------------------------------------------------
extern "C" int64_t tmpnn_seqloss_slab_numel(void) { return sq_layout().total; }

extern "C" size_t tmpnn_seqloss_saved_bytes(int64_t L) {
    return L < 2 || L > FT_L_MAX ? 0 : ft_carve2(nullptr, nullptr, true, L, 0, 0, 0, nullptr, true).saved_bytes;
}

extern "C" size_t tmpnn_seqloss_scratch_bytes(int64_t L) {
    return L < 2 || L > FT_L_MAX ? 0 : ft_carve2(nullptr, nullptr, true, L, 0, 0, 0, nullptr, true).scratch_bytes;
}

static int sq_check(const char *what, const float *X, const int32_t *S, const float *mask, const int32_t *ridx, const int32_t *cenc, int64_t L,
                    int k_neighbors, const float *params, int64_t slab_numel, float p_mpnn, const void *saved, size_t saved_bytes) {
    FT_REQUIRE(L >= 2 && L <= FT_L_MAX, "%s: protein length %lld outside [2, %lld]", what, (long long)L, (long long)FT_L_MAX);
    FT_REQUIRE(k_neighbors >= 1 && k_neighbors <= TM_KS, "%s: k_neighbors %d outside [1, %d]", what, k_neighbors, TM_KS);
    FT_REQUIRE(slab_numel == sq_layout().total, "%s: parameter slab holds %lld floats, ProteinMPNN with W_out needs %lld", what,
               (long long)slab_numel, (long long)sq_layout().total);
    FT_REQUIRE(X && S && mask && ridx && cenc && params, "%s: null pointer", what);       // (ranks may be null: every neighbour visible)
    FT_REQUIRE(p_mpnn >= 0.f && p_mpnn < 1.f, "%s: dropout probability outside [0, 1)", what);
    return ft_check_buf(what, "saved", (void *)saved, saved_bytes, tmpnn_seqloss_saved_bytes(L));
}

static FtCtx sq_ctx(const float *X, const int32_t *S, const float *mask, const int32_t *ridx, const int32_t *cenc, int64_t L, int k_neighbors,
                    const int32_t *ranks, const float *params, float *grads, void *saved, void *scratch, hipStream_t st) {
    FtCtx c{};
    c.L = (int)L;
    c.K = (int)(L < k_neighbors ? L : k_neighbors);
    c.n_prot = 1;
    c.min_len = c.max_len = c.L;
    c.E = (int64_t)c.L * c.K;
    c.nf = 3;
    c.seq = 1;
    c.X = X; c.S = S; c.mask = mask; c.ridx = ridx; c.cenc = cenc; c.ranks = ranks;
    c.params = params;
    c.grads = grads;
    c.lay = sq_layout();
    c.w = ft_carve2(saved, scratch, true, L, 0, 0, 0, nullptr, true);     // carved for K = 48: the buffers of a smaller K fit inside
    c.st = st;
    return c;
}

extern "C" int tmpnn_seqloss_forward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                     int64_t L, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                                     const float *keep_in, float *keep_out, uint64_t seed, uint64_t step, float *log_probs,
                                     int32_t *E_idx_opt, void *saved, size_t saved_bytes, tmpnn_stream_t stream) {
    FT_TRY(sq_check("seqloss_forward", X, S, mask, residue_idx, chain_enc, L, k_neighbors, params, slab_numel, p_mpnn, saved, saved_bytes));
    FT_REQUIRE(log_probs, "seqloss_forward: null pointer");
    FT_REQUIRE(!(keep_in && keep_out), "seqloss_forward: keep_in (injected masks) and keep_out (drawn masks) exclude each other");
    FtCtx c = sq_ctx(X, S, mask, residue_idx, chain_enc, L, k_neighbors, ranks, params, nullptr, saved, nullptr, (hipStream_t)stream);
    ft_set_drop(c, L, ft_k48(L), p_mpnn, keep_in, keep_out, seed, step);
    if (keep_out) (void)hipMemsetAsync(keep_out, 0, (size_t)ft_mask_numel(L) * 4, c.st);   // (K < 48 leaves the edge sites' tails unwritten)
    FT_TRY(ft_forward(c));
    (void)hipMemcpyAsync(log_probs, c.w.lp, (size_t)L * TMPNN_VOCAB * 4, hipMemcpyDeviceToDevice, c.st);
    if (E_idx_opt) (void)hipMemcpyAsync(E_idx_opt, c.w.eidx, (size_t)c.E * 4, hipMemcpyDeviceToDevice, c.st);
    return tm_check_launch("seqloss_forward");
}

static int sq_backward_entry(const char *what, bool want_dx, const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                             const int32_t *chain_enc, int64_t L, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel,
                             float p_mpnn, const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs, float *grads, float *dX,
                             const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream) {
    FT_TRY(sq_check(what, X, S, mask, residue_idx, chain_enc, L, k_neighbors, params, slab_numel, p_mpnn, saved, saved_bytes));
    FT_REQUIRE(dlog_probs && grads, "%s: null pointer", what);
    FT_REQUIRE(!want_dx || dX, "%s: dX is null (tmpnn_seqloss_backward is the entry without it)", what);
    FT_TRY(ft_check_buf(what, "scratch", scratch, scratch_bytes, tmpnn_seqloss_scratch_bytes(L)));
    // the saved part is only read: its one writer is the forward
    FtCtx c = sq_ctx(X, S, mask, residue_idx, chain_enc, L, k_neighbors, ranks, params, grads, const_cast<void *>(saved), scratch,
                     (hipStream_t)stream);
    c.dlp = dlog_probs;
    c.dX = dX;
    ft_set_drop(c, L, ft_k48(L), p_mpnn, keep_in, nullptr, seed, step);
    ft_backward(c);
    return tm_check_launch(what);
}

extern "C" int tmpnn_seqloss_backward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                      int64_t L, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                                      const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs, float *grads,
                                      const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream) {
    return sq_backward_entry("seqloss_backward", false, X, S, mask, residue_idx, chain_enc, L, k_neighbors, ranks, params, slab_numel, p_mpnn,
                             keep_in, seed, step, dlog_probs, grads, nullptr, saved, saved_bytes, scratch, scratch_bytes, stream);
}

extern "C" int tmpnn_seqloss_backward_x(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                        int64_t L, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                                        const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs, float *grads, float *dX,
                                        const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream) {
    return sq_backward_entry("seqloss_backward_x", true, X, S, mask, residue_idx, chain_enc, L, k_neighbors, ranks, params, slab_numel, p_mpnn,
                             keep_in, seed, step, dlog_probs, grads, dX, saved, saved_bytes, scratch, scratch_bytes, stream);
}
