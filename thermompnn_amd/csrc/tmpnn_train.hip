// Training of the ddG head with ProteinMPNN frozen (gfx950): head forward with dropout, backward, fused AdamW.
//
// Reference semantics (/root/reference): train_thermompnn.py:48-62 (one protein per step, loss = mean over labelled mutants of
// (pred - ddG)^2), :88-113 (AdamW over light_attention + both_out + ddg_out, default betas / eps / weight_decay 0.01), and the
// head of transfer_model.py:86-120 evaluated once per MUTANT: x = [h_dec(last) | ... | W_s[S]][pos] (the row head_concat_kernel
// builds), LightAttention on a length-1 sequence (:148-155) = o = Wc[:, :, 4] x + bc, then nn.Dropout(0.25) on o in training
// (:129, :138, :150); the softmax over a size-1 axis is exactly 1, so the attention convolution and the 8 non-centre taps of the
// feature convolution get exactly zero gradient. both_out = [ReLU, Linear] x (len(hidden_dims) + 1) (:67-71); ddg_out = Linear(1, 1)
// on each of the 21 outputs (:73, :108); subtract_mut: ddG = out[mut] - out[wt] from the SAME forward (:110-116).
//
// Every matrix product runs on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32). Weight gradients are reduced over the mutant
// rows in a fixed order: each wavefront sums one block of rows into a partial (a k-ordered fma chain inside the MFMA), a second
// kernel adds the partials in block order. No floating-point atomics: two identical steps are bit-identical.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

#include "tmpnn_common.h"
#include "tmpnn_internal.h"

#define TR_REQUIRE(cond, ...) do { if (!(cond)) return tm_set_error(TMPNN_E_INVALID, __VA_ARGS__); } while (0)
#define TR_TRY(expr) do { int rc_ = (expr); if (rc_ != TMPNN_OK) return rc_; } while (0)

static const int TR_MAX_LAYERS = 8;
static const int TR_MAX_SEG = 32;
static const int TR_MAX_PARTS = 16;
static const int64_t TR_M_MAX = 1 << 22;

// ---- dropout generator ------------------------------------------------------------------------------
// Stated 64-bit mix (splitmix64's finaliser, a bijection of uint64): k1 = mix(seed ^ 0x9E3779B97F4A7C15), k2 = mix(k1 + step),
// h = mix(k2 ^ (row << 32 | col)); the element is KEPT when (h >> 40) >= thr, thr = round(p * 2^24). Keep probability is exactly
// 1 - thr / 2^24 (0.75 for p = 0.25). tests/test_gpu_train.py restates it in numpy bit for bit.
__device__ __forceinline__ uint64_t tr_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// ---- dense layer: Y[m, n] = epi(b[n] + sum_k act(X[row(m), k]) W[n * ldw + wk0 + k * wks]) ------------------------------------
// act: ReLU when relu_in (both_out's ReLU sits in FRONT of each Linear). Epilogue, in this order: gate (Y *= G[m, n] > 0: the
// ReLU derivative of the backward pass), dropout (Y *= keep * scale; keep from keep_in, or drawn and written to keep_out).
// The backward data pass is the same kernel with W read transposed (ldw <-> wks) and no bias.
// Work item = one 16-row tile x one 16-column block per wavefront; lane (m, q) holds Y[tile + m, n0 + 4q + r], r = 0..3.
struct TrDense {
    const float *X; const int32_t *xrows; int n_xrows; const float *W; const float *b; float *Y; const float *gate;
    const float *keep_in; float *keep_out; uint64_t seed, step; uint32_t thr; float scale; int drop;   // drop: 0 off, 1 keep_in, 2 drawn
    int M, K, N, ldw, wks, wk0, relu_in;
};

__global__ __launch_bounds__(TM_THREADS) void tr_dense_kernel(TrDense a) {
    const int lane = tm_tid() & 63, wv = tm_wave(tm_tid()), m = lane & 15, q = lane >> 4;
    const int n_tiles = (a.M + 15) / 16, n_cb = (a.N + 15) / 16;
    uint64_t k2 = 0;
    if (a.drop == 2) k2 = tr_mix(tr_mix(a.seed ^ 0x9E3779B97F4A7C15ull) + a.step);
    for (int item = tm_bid() * 4 + wv; item < n_tiles * n_cb; item += tm_nblk() * 4) {
        const int tile = item / n_cb, n0 = (item - tile * n_cb) * 16;
        const int row = tile * 16 + m;
        const bool row_ok = row < a.M;
        int src = row_ok ? row : 0;
        if (a.xrows) src = min(max(a.xrows[src], 0), a.n_xrows - 1);
        const float *x = a.X + (size_t)src * a.K;
        const int wrow = n0 + m;
        const bool w_ok = wrow < a.N;
        const float *w = a.W + (size_t)(w_ok ? wrow : 0) * a.ldw + a.wk0;
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < a.K; k += 4) {
            const int kk = k + q;
            const bool k_ok = kk < a.K;
            float xv = row_ok && k_ok ? x[kk] : 0.f;
            if (a.relu_in) xv = fmaxf(xv, 0.f);
            const float wvv = w_ok && k_ok ? w[(size_t)kk * a.wks] : 0.f;
            acc = mfma16(wvv, xv, acc);
        }
        if (!row_ok) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int col = n0 + 4 * q + r;
            if (col >= a.N) continue;
            const size_t e = (size_t)row * a.N + col;
            float y = a.b ? acc[r] + a.b[col] : acc[r];
            if (a.gate && !(a.gate[e] > 0.f)) y = 0.f;
            if (a.drop) {
                float keep;
                if (a.drop == 1) {
                    keep = a.keep_in[e];
                } else {
                    const uint64_t h = tr_mix(k2 ^ (((uint64_t)(uint32_t)row << 32) | (uint32_t)col));
                    keep = (uint32_t)(h >> 40) >= a.thr ? 1.f : 0.f;
                    if (a.keep_out) a.keep_out[e] = keep;
                }
                y = y * (keep * a.scale);
            }
            a.Y[e] = y;
        }
    }
}

// ---- weight gradient: partial P[part][n][k] = sum over the part's rows m of dY[m, n] act(A[row(m), k]), column k = K is 1 ----------
// (the bias). MFMA operands: A-op lane (i, q) = dY[m0 + q, n0 + i], B-op lane (j, q) = act(A[m0 + q, k0 + j]); the accumulator of
// lane (j, q) holds P[n0 + 4q + r][k0 + j]. The rows of one part are summed in ascending order.
struct TrWgrad { const float *dY; const float *A; const int32_t *arows; int n_arows; float *P; int M, N, K, relu_in, rows_per_part, n_parts; };

__global__ __launch_bounds__(TM_THREADS) void tr_wgrad_kernel(TrWgrad a) {
    const int lane = tm_tid() & 63, wv = tm_wave(tm_tid()), i = lane & 15, q = lane >> 4;
    const int K1 = a.K + 1, n_nb = (a.N + 15) / 16, n_kb = (K1 + 15) / 16;
    for (int item = tm_bid() * 4 + wv; item < n_nb * n_kb * a.n_parts; item += tm_nblk() * 4) {
        const int part = item / (n_nb * n_kb), rest = item - part * (n_nb * n_kb), nb = rest / n_kb, kb = rest - nb * n_kb;
        const int n0 = nb * 16, k0 = kb * 16, m_beg = part * a.rows_per_part, m_end = min(a.M, m_beg + a.rows_per_part);
        const int n = n0 + i, k = k0 + i;
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
        for (int m0 = m_beg; m0 < m_end; m0 += 4) {
            const int mm = m0 + q;
            const bool m_ok = mm < m_end;
            const float dy = m_ok && n < a.N ? a.dY[(size_t)mm * a.N + n] : 0.f;
            float av = 0.f;
            if (m_ok && k < a.K) {
                const int src = a.arows ? min(max(a.arows[mm], 0), a.n_arows - 1) : mm;
                av = a.A[(size_t)src * a.K + k];
                if (a.relu_in) av = fmaxf(av, 0.f);
            } else if (m_ok && k == a.K) {
                av = 1.f;
            }
            acc = mfma16(dy, av, acc);
        }
        float *P = a.P + (size_t)part * a.N * K1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int nn = n0 + 4 * q + r;
            if (nn < a.N && k < K1) P[(size_t)nn * K1 + k] = acc[r];
        }
    }
}

// G[n * ldw + wk0 + k * wks] = sum_p P[p][n][k] (k < K), Gb[n] = sum_p P[p][n][K]: partials added in part order.
__global__ __launch_bounds__(TM_THREADS) void tr_wsum_kernel(const float *__restrict__ P, int n_parts, int N, int K, float *__restrict__ G,
                                                             int ldw, int wks, int wk0, float *__restrict__ Gb) {
    const int K1 = K + 1;
    const int64_t total = (int64_t)N * K1, stride = (int64_t)tm_nblk() * TM_THREADS;
    for (int64_t e = (int64_t)tm_bid() * TM_THREADS + tm_tid(); e < total; e += stride) {
        float s = P[e];
        for (int p = 1; p < n_parts; ++p) s += P[(size_t)p * total + e];
        const int n = (int)(e / K1), k = (int)(e - (int64_t)n * K1);
        if (k < K) G[(size_t)n * ldw + wk0 + (size_t)k * wks] = s;
        else Gb[n] = s;
    }
}

// ---- residual: pred, loss, dZ, ddg_out gradients (one workgroup, fixed-order reduction) ----------------------------------------
// pred_i = (w z[mut] + b) - (w z[wt] + b) (subtract_mut) | w z[mut] + b; d_i = 2 (pred_i - t_i) / n (F.mse_loss per mutant, then the
// mean of the stack, train_thermompnn.py:52-62); dZ[i, mut] += w d_i, dZ[i, wt] -= w d_i; dw = sum d_i (z[mut] - z[wt]);
// db = sum d_i, or 0 under subtract_mut (the bias cancels). loss = sum (pred - t)^2 / n.
struct TrResid { const float *Z; const int32_t *mut, *wt; const float *t; const float *ddg_w, *ddg_b; int M, subtract;
                 float *dZ, *g_ddg_w, *g_ddg_b, *loss, *pred; };

__device__ __forceinline__ float tr_pred(const float *Z, int i, int mut, int wt, float dw, float db, int subtract, float *zm, float *zw) {
    mut = min(max(mut, 0), TMPNN_VOCAB - 1);
    wt = min(max(wt, 0), TMPNN_VOCAB - 1);
    *zm = Z[(size_t)i * TMPNN_VOCAB + mut];
    *zw = Z[(size_t)i * TMPNN_VOCAB + wt];
    return subtract ? (dw * *zm + db) - (dw * *zw + db) : dw * *zm + db;
}

__global__ __launch_bounds__(TM_THREADS) void tr_resid_kernel(TrResid a) {
    __shared__ float red[3][TM_THREADS];
    const int tid = tm_tid();
    const float dw = a.ddg_w[0], db = a.ddg_b[0], inv_n = 1.f / (float)a.M;
    float sl = 0.f, sw = 0.f, sb = 0.f;
    for (int i = tid; i < a.M; i += TM_THREADS) {
        float zm, zw;
        const float p = tr_pred(a.Z, i, a.mut[i], a.wt[i], dw, db, a.subtract, &zm, &zw);
        const float r = p - a.t[i], d = 2.f * r * inv_n;
        if (a.pred) a.pred[i] = p;
        const int mut = min(max(a.mut[i], 0), TMPNN_VOCAB - 1), wt = min(max(a.wt[i], 0), TMPNN_VOCAB - 1);
        for (int c = 0; c < TMPNN_VOCAB; ++c) {
            float g = 0.f;
            if (c == mut) g += dw * d;
            if (a.subtract && c == wt) g -= dw * d;
            a.dZ[(size_t)i * TMPNN_VOCAB + c] = g;
        }
        sl += r * r;
        sw += a.subtract ? d * (zm - zw) : d * zm;
        sb += d;
    }
    red[0][tid] = sl;
    red[1][tid] = sw;
    red[2][tid] = sb;
    __syncthreads();
    for (int s = TM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int j = 0; j < 3; ++j) red[j][tid] += red[j][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        a.loss[0] = red[0][0] * inv_n;
        a.g_ddg_w[0] = red[1][0];
        a.g_ddg_b[0] = a.subtract ? 0.f : red[2][0];
    }
}

__global__ __launch_bounds__(TM_THREADS) void tr_pred_kernel(TrResid a) {
    const float dw = a.ddg_w[0], db = a.ddg_b[0];
    for (int i = tm_bid() * TM_THREADS + tm_tid(); i < a.M; i += tm_nblk() * TM_THREADS) {
        float zm, zw;
        a.pred[i] = tr_pred(a.Z, i, a.mut[i], a.wt[i], dw, db, a.subtract, &zm, &zw);
    }
}

// The residual's backward half seeded from a caller's d_i = dpred[i] (= dL / dpred_i) instead of the MSE form: the same dZ, the same
// per-thread sums and the same tree as tr_resid_kernel, so dpred[i] = 2 (pred_i - t_i) (1 / n) formed in fp32 gives its bits.
__global__ __launch_bounds__(TM_THREADS) void tr_seed_kernel(TrResid a, const float *__restrict__ dpred) {
    __shared__ float red[2][TM_THREADS];
    const int tid = tm_tid();
    const float dw = a.ddg_w[0], db = a.ddg_b[0];
    float sw = 0.f, sb = 0.f;
    for (int i = tid; i < a.M; i += TM_THREADS) {
        float zm, zw;
        (void)tr_pred(a.Z, i, a.mut[i], a.wt[i], dw, db, a.subtract, &zm, &zw);
        const float d = dpred[i];
        const int mut = min(max(a.mut[i], 0), TMPNN_VOCAB - 1), wt = min(max(a.wt[i], 0), TMPNN_VOCAB - 1);
        for (int c = 0; c < TMPNN_VOCAB; ++c) {
            float g = 0.f;
            if (c == mut) g += dw * d;
            if (a.subtract && c == wt) g -= dw * d;
            a.dZ[(size_t)i * TMPNN_VOCAB + c] = g;
        }
        sw += a.subtract ? d * (zm - zw) : d * zm;
        sb += d;
    }
    red[0][tid] = sw;
    red[1][tid] = sb;
    __syncthreads();
    for (int s = TM_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int j = 0; j < 2; ++j) red[j][tid] += red[j][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        a.g_ddg_w[0] = red[0][0];
        a.g_ddg_b[0] = a.subtract ? 0.f : red[1][0];
    }
}

// ---- fused AdamW over one flat slab -----------------------------------------------------------------------------------------
// torch/optim/adam.py with decoupled decay (AdamW), per element in torch's order: p *= 1 - lr wd; m = lerp(m, g, 1 - beta1);
// v = v beta2 + (1 - beta2) g g; p += -lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps). The scalars are formed on the
// host in double, as torch forms them in Python. Segment kinds: 1 = every element updates; 2 = only the centre taps (offset % 9 == 4)
// of a [N, K, 9] convolution weight do; 0 = none does. Elements that do not update have a structurally zero gradient, hence m = v = 0
// for ever: the full update reduces to p *= 1 - lr wd bit for bit (m / (0 + eps) = 0), so only the decay runs and m, v, g are not read.
struct TrSeg { int64_t begin, end; int block0, kind; float decay, step_size, bc2_sqrt; };
struct TrAdam { float *p; const float *g; float *m; float *v; float lerp_w, beta2, omb2, eps; int n_seg; TrSeg seg[TR_MAX_SEG]; };

static const int TR_ADAM_PER_BLOCK = TM_THREADS * 8;

__global__ __launch_bounds__(TM_THREADS) void tr_adamw_kernel(TrAdam a) {
    const int b = tm_bid();
    int s = 0;
    while (s + 1 < a.n_seg && a.seg[s + 1].block0 <= b) ++s;
    const TrSeg sg = a.seg[s];
    const int64_t beg = sg.begin + (int64_t)(b - sg.block0) * TR_ADAM_PER_BLOCK;
    const int64_t end = min(sg.end, beg + TR_ADAM_PER_BLOCK);
    for (int64_t e = beg + tm_tid(); e < end; e += TM_THREADS) {
        float p = a.p[e] * sg.decay;
        const bool upd = sg.kind == 1 || (sg.kind == 2 && (e - sg.begin) % 9 == 4);
        if (upd) {
            const float g = a.g[e];
            const float m = a.m[e] + a.lerp_w * (g - a.m[e]);
            const float v = a.v[e] * a.beta2 + a.omb2 * g * g;
            a.m[e] = m;
            a.v[e] = v;
            p = p + sg.step_size * (m / (sqrtf(v) / sg.bc2_sqrt + a.eps));
        }
        a.p[e] = p;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
static int tr_dims_ok(int n_final, int n_layers, const int32_t *dims) {
    if (n_final < 0 || n_final > 3 || n_layers < 1 || n_layers > TR_MAX_LAYERS || !dims) return 0;
    if (dims[0] != TMPNN_HID * n_final + TMPNN_HID || dims[n_layers] != TMPNN_VOCAB) return 0;
    for (int l = 1; l < n_layers; ++l)
        if (dims[l] < 1 || dims[l] > 4096) return 0;
    return 1;
}

// slab offsets in state-dict order (weights.head_param_shapes): [conv_w, conv_b, att_w, att_b,] (W_l, b_l) x n_layers, ddg_w, ddg_b
struct TrLayout { int64_t conv_w, conv_b, att_w, att_b, W[TR_MAX_LAYERS], b[TR_MAX_LAYERS], ddg_w, ddg_b, total; };

static TrLayout tr_layout(int lightattn, int n_layers, const int32_t *dims) {
    TrLayout L{};
    int64_t o = 0;
    const int64_t D0 = dims[0];
    if (lightattn) {
        L.conv_w = o; o += D0 * D0 * 9;
        L.conv_b = o; o += D0;
        L.att_w = o; o += D0 * D0 * 9;
        L.att_b = o; o += D0;
    }
    for (int l = 0; l < n_layers; ++l) {
        L.W[l] = o; o += (int64_t)dims[l + 1] * dims[l];
        L.b[l] = o; o += dims[l + 1];
    }
    L.ddg_w = o++;
    L.ddg_b = o++;
    L.total = o;
    return L;
}

static int tr_parts(int64_t M) {
    const int64_t p = (M + 63) / 64;
    return (int)(p < 1 ? 1 : p > TR_MAX_PARTS ? TR_MAX_PARTS : p);
}

struct TrWs { float *H[TR_MAX_LAYERS + 1]; float *mask, *dA, *dB, *P; size_t bytes; };

static TrWs tr_carve(void *base, int64_t M, int lightattn, int n_layers, const int32_t *dims) {
    TrWs w{};
    Carver c(base, false);                           // (base == nullptr measures; the entries compare with `bytes` first)
    int widest = dims[0];
    for (int l = 1; l <= n_layers; ++l) widest = dims[l] > widest ? dims[l] : widest;
    w.H[0] = lightattn ? c.take<float>((size_t)M * dims[0]) : nullptr;
    for (int l = 1; l <= n_layers; ++l) w.H[l] = c.take<float>((size_t)M * dims[l]);
    w.mask = lightattn ? c.take<float>((size_t)M * dims[0]) : nullptr;
    w.dA = c.take<float>((size_t)M * widest);
    w.dB = c.take<float>((size_t)M * widest);
    size_t pmax = 0;
    for (int l = 0; l < n_layers; ++l) pmax = std::max(pmax, (size_t)dims[l + 1] * (dims[l] + 1));
    if (lightattn) pmax = std::max(pmax, (size_t)dims[0] * (dims[0] + 1));
    w.P = c.take<float>(pmax * tr_parts(M));
    w.bytes = c.used + 256;
    return w;
}

static int tr_grid(int64_t wave_items) {
    const int64_t b = (wave_items + 3) / 4, cap = (int64_t)tm_num_cus() * 8;
    return (int)(b < 1 ? 1 : b < cap ? b : cap);
}

static void tr_launch_dense(const TrDense &d, hipStream_t st) {
    const int64_t items = (int64_t)((d.M + 15) / 16) * ((d.N + 15) / 16);
    tr_dense_kernel<<<tr_grid(items), TM_THREADS, 0, st>>>(d);
}

// dW (strided into the slab) and db from dY [M, N] and the layer input A [M, K] (rows through arows when given)
static void tr_launch_wgrad(const float *dY, const float *A, const int32_t *arows, int n_arows, int relu_in, int M, int N, int K,
                            float *G, int ldw, int wks, int wk0, float *Gb, float *P, hipStream_t st) {
    const int parts = tr_parts(M), rpp = (((M + parts - 1) / parts) + 3) & ~3;
    TrWgrad w{dY, A, arows, n_arows, P, M, N, K, relu_in, rpp, parts};
    const int64_t items = (int64_t)((N + 15) / 16) * ((K + 1 + 15) / 16) * parts;
    tr_wgrad_kernel<<<tr_grid(items), TM_THREADS, 0, st>>>(w);
    const int64_t total = (int64_t)N * (K + 1), blocks = (total + TM_THREADS - 1) / TM_THREADS, cap = (int64_t)tm_num_cus() * 8;
    tr_wsum_kernel<<<(int)(blocks < cap ? blocks : cap), TM_THREADS, 0, st>>>(P, parts, N, K, G, ldw, wks, wk0, Gb);
}

// forward through the head: H[0] = dropout(centre tap) (LightAttention) and H[l + 1] = Linear_l(ReLU(H[l])); -> Z = H[n_layers]
static void tr_forward(const float *feat, const int32_t *rows, int n_feat, int M, int lightattn, int n_layers, const int32_t *dims,
                       const float *slab, const TrLayout &L, const TrWs &w, int drop, const float *keep_in, float *keep_out, uint64_t seed,
                       uint64_t step, uint32_t thr, float scale, hipStream_t st) {
    const int D0 = dims[0];
    if (lightattn) {
        TrDense d{feat, rows, n_feat, slab + L.conv_w, slab + L.conv_b, w.H[0], nullptr, keep_in, keep_out, seed, step, thr, scale, drop,
                  M, D0, D0, 9 * D0, 9, 4, 0};
        tr_launch_dense(d, st);
    }
    for (int l = 0; l < n_layers; ++l) {
        const float *in = l == 0 && !lightattn ? feat : w.H[l];
        const int32_t *in_rows = l == 0 && !lightattn ? rows : nullptr;
        TrDense d{in, in_rows, n_feat, slab + L.W[l], slab + L.b[l], w.H[l + 1], nullptr, nullptr, nullptr, 0, 0, 0, 1.f, 0,
                  M, dims[l], dims[l + 1], dims[l], 1, 0, 1};
        tr_launch_dense(d, st);
    }
}

static int tr_check_common(const float *feat, const int32_t *rows, const int32_t *mut, const int32_t *wt, int64_t M, int64_t n_feat,
                           int n_final, int lightattn, int n_layers, const int32_t *dims, const float *params, int64_t slab_numel,
                           const char *what) {
    TR_REQUIRE(tr_dims_ok(n_final, n_layers, dims),
               "%s: dims must run from 128 * num_final_layers + 128 to 21 over 1..8 layers (num_final_layers 0..3)", what);
    TR_REQUIRE(M >= 0 && M <= TR_M_MAX, "%s: bad number of mutants %lld", what, (long long)M);
    TR_REQUIRE(n_feat >= 1 && n_feat <= TR_M_MAX * 16, "%s: bad number of feature rows %lld", what, (long long)n_feat);
    const TrLayout L = tr_layout(lightattn, n_layers, dims);
    TR_REQUIRE(slab_numel == L.total, "%s: parameter slab holds %lld floats, this head needs %lld", what, (long long)slab_numel,
               (long long)L.total);
    TR_REQUIRE(feat && rows && mut && wt && params, "%s: null pointer", what);
    return TMPNN_OK;
}

extern "C" int64_t tmpnn_head_slab_numel(int n_final, int lightattn, int n_layers, const int32_t *dims) {
    if (!tr_dims_ok(n_final, n_layers, dims)) return -1;
    return tr_layout(lightattn, n_layers, dims).total;
}

extern "C" size_t tmpnn_head_train_workspace_bytes(int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims) {
    if (M < 0 || M > TR_M_MAX || !tr_dims_ok(n_final, n_layers, dims)) return 0;
    return tr_carve(nullptr, M, lightattn, n_layers, dims).bytes;
}

extern "C" int tmpnn_head_train_step(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt,
                                     const float *target, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims,
                                     int subtract_mut, const float *params, float *grads, int64_t slab_numel, float p_drop,
                                     const float *keep_in, float *keep_out, uint64_t seed, uint64_t step, float *loss, float *pred_opt,
                                     void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    TR_TRY(tr_check_common(feat, rows, mut, wt, M, n_feat, n_final, lightattn, n_layers, dims, params, slab_numel, "head_train_step"));
    TR_REQUIRE(target && grads && loss, "head_train_step: null pointer");
    TR_REQUIRE(M >= 1, "head_train_step: a step needs at least one labelled mutant");
    TR_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "head_train_step: dropout probability %g outside [0, 1)", (double)p_drop);
    TR_REQUIRE(lightattn || (p_drop == 0.f && !keep_in && !keep_out), "head_train_step: dropout needs LightAttention (lightattn)");
    TR_REQUIRE(!(keep_in && keep_out), "head_train_step: keep_in (injected mask) and keep_out (drawn mask) exclude each other");
    const size_t need = tmpnn_head_train_workspace_bytes(M, n_final, lightattn, n_layers, dims);
    if (!workspace || workspace_bytes < need)
        return tm_set_error(TMPNN_E_WORKSPACE, "head_train_step: workspace %zu < %zu bytes", workspace_bytes, need);
    return tm_head_train_core(feat, n_feat, rows, mut, wt, target, M, lightattn, n_layers, dims, subtract_mut, params, grads, p_drop,
                              keep_in, keep_out, seed, step, loss, pred_opt, workspace, (hipStream_t)stream, nullptr, nullptr);
}

// The launches of one head training step (arguments already validated). dfeat [M, D0] (may be null): d loss / d feature row of
// every mutant, for a caller that back-propagates further (tmpnn_finetune.hip); it needs rows[i] == i (feat holds the mutants' rows).
// dpred [M] (may be null): the backward starts from d_i = dpred[i] instead of the MSE residual; target, loss and pred_opt are then
// not used.
int tm_head_train_core(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt,
                       const float *target, int64_t M, int lightattn, int n_layers, const int32_t *dims, int subtract_mut,
                       const float *params, float *grads, float p_drop, const float *keep_in, float *keep_out, uint64_t seed,
                       uint64_t step, float *loss, float *pred_opt, void *workspace, hipStream_t st, float *dfeat, const float *dpred) {
    const TrLayout L = tr_layout(lightattn, n_layers, dims);
    const TrWs w = tr_carve(workspace, M, lightattn, n_layers, dims);
    const int D0 = dims[0], Mi = (int)M, nf = (int)n_feat;
    const int drop = keep_in ? 1 : p_drop > 0.f ? 2 : 0;
    const uint32_t thr = (uint32_t)llround((double)p_drop * 16777216.0);
    const float scale = (float)(1.0 / (1.0 - (double)p_drop));
    float *mask = drop == 2 ? (keep_out ? keep_out : w.mask) : nullptr;
    tr_forward(feat, rows, nf, Mi, lightattn, n_layers, dims, params, L, w, drop, keep_in, mask, seed, step, thr, scale, st);

    float *dY = w.dA, *dX = w.dB;
    TrResid r{w.H[n_layers], mut, wt, target, params + L.ddg_w, params + L.ddg_b, Mi, subtract_mut, dY, grads + L.ddg_w,
              grads + L.ddg_b, loss, pred_opt};
    if (dpred) tr_seed_kernel<<<1, TM_THREADS, 0, st>>>(r, dpred);
    else tr_resid_kernel<<<1, TM_THREADS, 0, st>>>(r);
    for (int l = n_layers - 1; l >= 0; --l) {
        const bool raw_in = l == 0 && !lightattn;      // layer 0 reads the feature rows themselves
        const float *A = raw_in ? feat : w.H[l];
        tr_launch_wgrad(dY, A, raw_in ? rows : nullptr, nf, 1, Mi, dims[l + 1], dims[l], grads + L.W[l], dims[l], 1, 0, grads + L.b[l],
                        w.P, st);
        if (l == 0 && !lightattn) break;
        // dX = (dY W_l) * [H_l > 0]; for H[0] also * keep / (1 - p) (dropout backward)
        const float *keep = l == 0 ? (drop == 1 ? keep_in : mask) : nullptr;
        TrDense d{dY, nullptr, Mi, params + L.W[l], nullptr, dX, w.H[l], keep, nullptr, 0, 0, 0, scale, keep ? 1 : 0,
                  Mi, dims[l + 1], dims[l], 1, dims[l], 0, 0};
        tr_launch_dense(d, st);
        std::swap(dY, dX);
    }
    if (lightattn)   // centre tap of feature_convolution, strided into the [D0, D0, 9] weight: ldw 9 D0, wks 9, wk0 4
        tr_launch_wgrad(dY, feat, rows, nf, 0, Mi, D0, D0, grads + L.conv_w, 9 * D0, 9, 4, grads + L.conv_b, w.P, st);
    if (dfeat && lightattn) {   // dfeat = dY Wc[:, :, 4]: the centre tap read transposed (element (n, k) at n 9 D0 + 9 k + 4)
        TrDense d{dY, nullptr, Mi, params + L.conv_w, nullptr, dfeat, nullptr, nullptr, nullptr, 0, 0, 0, 1.f, 0, Mi, D0, D0, 9, 9 * D0, 4, 0};
        tr_launch_dense(d, st);
    } else if (dfeat) {         // dfeat = (dY W_0) * [feat > 0]: both_out's first ReLU reads the feature row itself
        TrDense d{dY, nullptr, Mi, params + L.W[0], nullptr, dfeat, feat, nullptr, nullptr, 0, 0, 0, 1.f, 0, Mi, dims[1], D0, 1, D0, 0, 0};
        tr_launch_dense(d, st);
    }
    return tm_check_launch("head_train_step");
}

// The training forward alone (arguments already validated): pred [M] with the head's dropout drawn or read as tm_head_train_core
// does (same kernels, same order: the bits of its pred_opt). keep_out may be null.
int tm_head_forward(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt, int64_t M,
                    int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params, float p_drop,
                    const float *keep_in, float *keep_out, uint64_t seed, uint64_t step, float *pred, void *workspace, hipStream_t st) {
    const TrLayout L = tr_layout(lightattn, n_layers, dims);
    const TrWs w = tr_carve(workspace, M, lightattn, n_layers, dims);
    const int drop = keep_in ? 1 : p_drop > 0.f ? 2 : 0;
    const uint32_t thr = (uint32_t)llround((double)p_drop * 16777216.0);
    const float scale = (float)(1.0 / (1.0 - (double)p_drop));
    float *mask = drop == 2 ? (keep_out ? keep_out : w.mask) : nullptr;
    tr_forward(feat, rows, (int)n_feat, (int)M, lightattn, n_layers, dims, params, L, w, drop, keep_in, mask, seed, step, thr, scale, st);
    TrResid r{w.H[n_layers], mut, wt, nullptr, params + L.ddg_w, params + L.ddg_b, (int)M, subtract_mut, nullptr, nullptr, nullptr,
              nullptr, pred};
    const int64_t blocks = (M + TM_THREADS - 1) / TM_THREADS, cap = (int64_t)tm_num_cus() * 4;
    tr_pred_kernel<<<(int)(blocks < cap ? blocks : cap), TM_THREADS, 0, st>>>(r);
    return tm_check_launch("head_forward");
}

extern "C" int tmpnn_head_eval(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt, int64_t M,
                               int n_final, int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params,
                               int64_t slab_numel, float *pred, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    if (M == 0) return TMPNN_OK;
    TR_TRY(tr_check_common(feat, rows, mut, wt, M, n_feat, n_final, lightattn, n_layers, dims, params, slab_numel, "head_eval"));
    TR_REQUIRE(pred, "head_eval: null pointer");
    const size_t need = tmpnn_head_train_workspace_bytes(M, n_final, lightattn, n_layers, dims);
    if (!workspace || workspace_bytes < need)
        return tm_set_error(TMPNN_E_WORKSPACE, "head_eval: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const TrLayout L = tr_layout(lightattn, n_layers, dims);
    const TrWs w = tr_carve(workspace, M, lightattn, n_layers, dims);
    tr_forward(feat, rows, (int)n_feat, (int)M, lightattn, n_layers, dims, params, L, w, 0, nullptr, nullptr, 0, 0, 0, 1.f, st);
    TrResid r{w.H[n_layers], mut, wt, nullptr, params + L.ddg_w, params + L.ddg_b, (int)M, subtract_mut, nullptr, nullptr, nullptr,
              nullptr, pred};
    const int64_t blocks = (M + TM_THREADS - 1) / TM_THREADS, cap = (int64_t)tm_num_cus() * 4;
    tr_pred_kernel<<<(int)(blocks < cap ? blocks : cap), TM_THREADS, 0, st>>>(r);
    return tm_check_launch("head_eval");
}

extern "C" int tmpnn_adamw_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t numel, int n_seg,
                                const int64_t *seg_begin, const int32_t *seg_kind, const double *seg_lr, double beta1, double beta2,
                                double eps, double weight_decay, int64_t step, tmpnn_stream_t stream) {
    TR_REQUIRE(n_seg >= 1 && n_seg <= TR_MAX_SEG, "adamw_step: %d segments outside [1, %d]", n_seg, TR_MAX_SEG);
    TR_REQUIRE(seg_begin && seg_kind && seg_lr, "adamw_step: null segment table");
    TR_REQUIRE(numel >= 1 && seg_begin[0] == 0 && seg_begin[n_seg] == numel, "adamw_step: segments must cover [0, numel)");
    TR_REQUIRE(step >= 1, "adamw_step: step counts from 1");
    TR_REQUIRE(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0 && weight_decay >= 0, "adamw_step: bad hyper-parameters");
    TR_REQUIRE(params && grads && exp_avg && exp_avg_sq, "adamw_step: null pointer");
    TrAdam a{params, grads, exp_avg, exp_avg_sq, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, n_seg, {}};
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    int blocks = 0;
    for (int s = 0; s < n_seg; ++s) {
        TR_REQUIRE(seg_begin[s + 1] >= seg_begin[s], "adamw_step: segment %d has negative length", s);
        TR_REQUIRE(seg_kind[s] >= 0 && seg_kind[s] <= 2, "adamw_step: segment %d has unknown kind %d", s, seg_kind[s]);
        TR_REQUIRE(seg_lr[s] >= 0, "adamw_step: segment %d has a negative learning rate", s);
        const int64_t n = seg_begin[s + 1] - seg_begin[s], nb = (n + TR_ADAM_PER_BLOCK - 1) / TR_ADAM_PER_BLOCK;
        a.seg[s] = TrSeg{seg_begin[s], seg_begin[s + 1], blocks, seg_kind[s], (float)(1.0 - seg_lr[s] * weight_decay),
                         (float)(-(seg_lr[s] / bc1)), (float)sqrt(bc2)};
        blocks += (int)nb;
    }
    if (blocks == 0) return TMPNN_OK;
    tr_adamw_kernel<<<blocks, TM_THREADS, 0, (hipStream_t)stream>>>(a);
    return tm_check_launch("adamw_step");
}
