// The C-alpha-only edge featurizer (gfx950): ProteinMPNN's ca_only flavour. Siblings of featurize_kernel / featurize_split_kernel
// (tmpnn_graph.hip): one residue and its 48 edge slots per tile, 8 wavefronts, the same GEMM / LayerNorm helpers.
//
// Reference semantics: CA_ProteinFeatures (/root/reference/protein_mpnn_utils.py:911-1081). Per edge (i, j = E_idx[i,k]) the 167 inputs
// are [posenc 16 | 9 x 16 RBF | dU 3 | Q 4] -> edge_embedding (128 x 167, no bias) -> norm_edges; W_e (:1229) follows in the same launch.
// The k-NN graph is the full-backbone one (_dist on the C-alpha atoms, :1008-1020): knn_kernel is reused unchanged, and X stays
// [T,4,3] with only slot 1 read. AD_features (:973-983) is computed by the reference and never used: not built here.
//
// SEGMENTS. The reference shifts and differences C-alpha along the padded length axis: Ca_0[t] = Ca[t-1], Ca_2[t] = Ca[t+1]
// (:1046-1050) and dX[t] = Ca[t+1] - Ca[t] (:961), with ZERO coordinates in front of row 0 and behind row L-1, and O = 0 on rows 0,
// L-2 and L-1 (the F.pad of :989). Here a segment is one protein of the packed residue axis, [offsets[p], offsets[p+1]). A padded
// [B, L] batch laid out as B segments of L rows (padding rows carry coordinates 0, as tied_featurize leaves them) therefore
// reproduces the reference's padded result, and a ragged batch reproduces every protein run alone. A segment of fewer than 3 rows
// (the reference itself fails there) has zero frames; nothing is ever read outside a row's segment.
//
// GEMM 1 has 151 feature columns, padded to K = 160 with zero columns of the weight image (tmpnn_weights::edge_ca); the positional
// term arrives as the accumulators' initial value (pos_table). K order: 144 Gaussians, then dU, Q, 9 zeros — the Gaussian loop keeps
// the 4-centres-per-thread shape of the full featurizer. Every input lies in [-1, 1]: the f16x2 split needs no range handling.
#include "tmpnn_common.h"
#include "tmpnn_internal.h"
#include "tmpnn_split.h"

#define CA_K 160          // GEMM-1 depth: 151 columns + 9 of zero padding
#define CA_RS 192         // row length (floats) of the swizzled fp32 feature tile: 40 chunks used, the XOR swizzle reaches chunk 47
#define CA_ROWB 512       // row pitch (bytes) of a 16-bit feature plane: 20 chunks used, the swizzle reaches chunk 31

// ------------------------------------------------------------------------------------------------
// Frames and orientation features. sign(), the 3.6 / 4.0 window and relu() make the reference's result a discontinuous function of
// rounding, so the operands that feed them are computed in the association of the torch expressions — products rounded before they
// are added (no fma contraction: __fmul_rn / __fadd_rn / __fsub_rn), row . column sums left to right, squared norms as
// x^2 + y^2 + z^2 — by ONE set of functions that the pre-pass and both edge kernels share.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ca_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}
// F.normalize: x / max(|x|, 1e-12)
__device__ __forceinline__ void ca_normalize3(float (&v)[3]) {
    const float d = fmaxf(sqrtf(ca_dot3(v[0], v[1], v[2], v[0], v[1], v[2])), 1e-12f);
    v[0] = v[0] / d; v[1] = v[1] / d; v[2] = v[2] / d;
}
__device__ __forceinline__ void ca_cross(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
    c[0] = __fsub_rn(__fmul_rn(a[1], b[2]), __fmul_rn(a[2], b[1]));
    c[1] = __fsub_rn(__fmul_rn(a[2], b[0]), __fmul_rn(a[0], b[2]));
    c[2] = __fsub_rn(__fmul_rn(a[0], b[1]), __fmul_rn(a[1], b[0]));
}
// U = normalize(dX), dX = b - a zeroed unless 3.6 < |dX| < 4.0 (:961-965: C-alpha to C-alpha jumps excluded)
__device__ __forceinline__ void ca_step(const float *__restrict__ a, const float *__restrict__ b, float (&u)[3]) {
    u[0] = __fsub_rn(b[0], a[0]); u[1] = __fsub_rn(b[1], a[1]); u[2] = __fsub_rn(b[2], a[2]);
    const float n = sqrtf(ca_dot3(u[0], u[1], u[2], u[0], u[1], u[2]));
    const bool keep = 3.6f < n && n < 4.0f;
    u[0] = keep ? u[0] : 0.f; u[1] = keep ? u[1] : 0.f; u[2] = keep ? u[2] : 0.f;
    ca_normalize3(u);
}
// protein p with offsets[p] <= t < offsets[p+1] -> [s, e)
__device__ __forceinline__ void ca_segment(const int32_t *__restrict__ offsets, int N, int t, int &s, int &e) {
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= t) lo = mid; else hi = mid;
    }
    s = offsets[lo];
    e = offsets[lo + 1];
}
// O_t = rows (o, n, o x n), o = normalize(U[t-1] - U[t]), n = normalize(U[t-1] x U[t]) for rows 1 .. n-3 of the segment [s, e), else 0
// (:986-989). Reads the C-alpha atoms of rows t-1, t, t+1 — all inside the segment for the rows that have a frame.
__device__ __forceinline__ void ca_frame(const float *__restrict__ X, int s, int e, int t, float (&O)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) O[k] = 0.f;
    if (t - s < 1 || t > e - 3) return;
    float u0[3], u1[3], o[3], n[3], b[3];
    ca_step(X + (size_t)(t - 1) * 12 + 3, X + (size_t)t * 12 + 3, u0);
    ca_step(X + (size_t)t * 12 + 3, X + (size_t)(t + 1) * 12 + 3, u1);
    o[0] = __fsub_rn(u0[0], u1[0]); o[1] = __fsub_rn(u0[1], u1[1]); o[2] = __fsub_rn(u0[2], u1[2]);
    ca_normalize3(o);
    ca_cross(u0, u1, n);
    ca_normalize3(n);
    ca_cross(o, n, b);
#pragma unroll
    for (int k = 0; k < 3; ++k) { O[k] = o[k]; O[3 + k] = n[k]; O[6 + k] = b[k]; }
}
__device__ __forceinline__ float ca_sign(float x) { return (float)((x > 0.f) - (x < 0.f)); }
// out = [dU 3 | Q 4]: dU = normalize(O_i . dX) (:998-1000), Q = _quaternions(O_i^T O_j) (:932-958, :1001-1002)
__device__ __forceinline__ void ca_orient(const float (&Oi)[9], const float (&Oj)[9], const float (&dX)[3], float (&out)[7]) {
    float dU[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) dU[r] = ca_dot3(Oi[3 * r], Oi[3 * r + 1], Oi[3 * r + 2], dX[0], dX[1], dX[2]);
    ca_normalize3(dU);
    float R[3][3];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) R[x][y] = ca_dot3(Oi[x], Oi[3 + x], Oi[6 + x], Oj[y], Oj[3 + y], Oj[6 + y]);
    const float Rxx = R[0][0], Ryy = R[1][1], Rzz = R[2][2];
    const float mx = 0.5f * sqrtf(fabsf(__fadd_rn(1.f, __fsub_rn(__fsub_rn(Rxx, Ryy), Rzz))));
    const float my = 0.5f * sqrtf(fabsf(__fadd_rn(1.f, __fsub_rn(__fadd_rn(-Rxx, Ryy), Rzz))));
    const float mz = 0.5f * sqrtf(fabsf(__fadd_rn(1.f, __fadd_rn(__fsub_rn(-Rxx, Ryy), Rzz))));
    float q[4];
    q[0] = ca_sign(__fsub_rn(R[2][1], R[1][2])) * mx;
    q[1] = ca_sign(__fsub_rn(R[0][2], R[2][0])) * my;
    q[2] = ca_sign(__fsub_rn(R[1][0], R[0][1])) * mz;
    q[3] = sqrtf(fmaxf(__fadd_rn(1.f, __fadd_rn(__fadd_rn(Rxx, Ryy), Rzz)), 0.f)) / 2.f;
    const float nq = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(q[0], q[0]), __fmul_rn(q[1], q[1])), __fmul_rn(q[2], q[2])), __fmul_rn(q[3], q[3]));
    const float d = fmaxf(sqrtf(nq), 1e-12f);
    out[0] = dU[0]; out[1] = dU[1]; out[2] = dU[2];
    out[3] = q[0] / d; out[4] = q[1] / d; out[5] = q[2] / d; out[6] = q[3] / d;
}

// ------------------------------------------------------------------------------------------------
// ca_frames: O [T,9], one thread per residue (the pre-pass of a CA forward: a frame is computed once per residue, the edge kernels
// gather O_j beside E_idx)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_THREADS) void ca_frames_kernel(const float *__restrict__ X, const int32_t *__restrict__ offsets, int N, int T,
                                                               float *__restrict__ O) {
    const int t = tm_bid() * TM_THREADS + tm_tid();
    if (t >= T) return;
    int s, e;
    ca_segment(offsets, N, t, s, e);
    float o[9];
    ca_frame(X, s, e, t, o);
#pragma unroll
    for (int k = 0; k < 9; ++k) O[(size_t)t * 9 + k] = o[k];
}

// ------------------------------------------------------------------------------------------------
// the edge kernels
// ------------------------------------------------------------------------------------------------
struct CaFeatArgs {
    const float *edge_ca;    // [128,160]: edge_embedding.weight[:, 16:167] + 9 zero columns
    const float *pos_table;  // [66,128]
    const float *ln_w, *ln_b, *We_w, *We_b;
    const float *X;          // [T,4,3], slot 1 read
    const float *O;          // [T,9] (ca_frames_kernel)
    const int32_t *offsets;  // [N+1]
    const int32_t *ridx, *cenc, *E_idx;
    const float *D_nb;
    float *hE, *E_opt;
    int N, T;
    float mu[16];            // torch.linspace(2, 22, 16)
    const char *img_e[2];    // fragment images of edge_ca's K blocks 0..127 and 128..159 ...
    const char *img_we;      // ... and of W_e (f16x2 handles; null otherwise)
};

// What lane mm < 48 of wavefront 0 holds of one tile between its loads (issued a tile ahead) and `ca_publish`
struct CaRaw {
    int j, dpos;             // E_idx entry (< 0: no neighbour), PositionalEncodings index
    float d0;                // masked C-alpha distance from _dist
    float ci[3][3], cj[3][3];   // Ca_0, Ca_1, Ca_2 of the residue and of the neighbour (zero outside the segment)
    float oi[9], oj[9];
};
__device__ __forceinline__ void ca_row(const float *__restrict__ X, int t, int s, int e, float (&c)[3]) {
    const bool in = t >= s && t < e;
    const float *p = X + (size_t)(in ? t : s) * 12 + 3;
    const float x = p[0], y = p[1], z = p[2];
    c[0] = in ? x : 0.f; c[1] = in ? y : 0.f; c[2] = in ? z : 0.f;
}
// the loads of tile i for slot mm, given its list entry j (loaded a tile earlier still, so nothing here waits for it)
__device__ __forceinline__ void ca_load(const CaFeatArgs &a, int i, int mm, int j, CaRaw &r) {
    int s, e;
    ca_segment(a.offsets, a.N, i, s, e);
    const int jj = (j < s || j >= e) ? i : j;               // (an entry outside the residue's own protein never comes from knn_kernel)
    r.j = j;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        ca_row(a.X, i - 1 + d, s, e, r.ci[d]);
        ca_row(a.X, jj - 1 + d, s, e, r.cj[d]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) { r.oi[k] = a.O[(size_t)i * 9 + k]; r.oj[k] = a.O[(size_t)jj * 9 + k]; }
    const int off = a.ridx[i] - a.ridx[jj];                  // PositionalEncodings index (:903-905, :1070-1075)
    r.dpos = a.cenc[i] == a.cenc[jj] ? min(max(off + 32, 0), 64) : 65;
    r.d0 = a.D_nb[(size_t)i * TM_KS + mm];
}
// _get_rbf's distance (:1034): sqrt(sum((A - B)^2) + 1e-6)
__device__ __forceinline__ float ca_dist(const float (&A)[3], const float (&B)[3]) {
    const float dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
    return sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
}
// the 9 distances in the reference's block order (:1055-1066) and the 7 orientation features of slot mm -> LDS
__device__ __forceinline__ void ca_publish(const CaRaw &r, float *dist /*[12]*/, float *orient /*[8]*/, int *ix_j, int *ix_pos) {
    dist[0] = r.d0;                                          // (1,1): D_neighbors
    dist[1] = ca_dist(r.ci[0], r.cj[0]);
    dist[2] = ca_dist(r.ci[2], r.cj[2]);
    dist[3] = ca_dist(r.ci[0], r.cj[1]);
    dist[4] = ca_dist(r.ci[0], r.cj[2]);
    dist[5] = ca_dist(r.ci[1], r.cj[0]);
    dist[6] = ca_dist(r.ci[1], r.cj[2]);
    dist[7] = ca_dist(r.ci[2], r.cj[0]);
    dist[8] = ca_dist(r.ci[2], r.cj[1]);
    float dX[3], f[7];
#pragma unroll
    for (int k = 0; k < 3; ++k) dX[k] = __fsub_rn(r.cj[1][k], r.ci[1][k]);
    ca_orient(r.oi, r.oj, dX, f);
#pragma unroll
    for (int k = 0; k < 7; ++k) orient[k] = f[k];
    orient[7] = 0.f;
    *ix_j = r.j;
    *ix_pos = r.dpos;
}

// fp32 MFMA form ("fp32" handles)
__global__ __launch_bounds__(512, 2) void featurize_ca_kernel(CaFeatArgs a) {
    constexpr int NW = 8, NT = 64 * NW, RPW = TM_TILE / NW;
    __shared__ __attribute__((aligned(16))) float feat[TM_TILE * CA_RS];
    __shared__ __attribute__((aligned(16))) float tA[TM_TILE * TM_H];
    __shared__ __attribute__((aligned(16))) float tB[TM_TILE * TM_H];
    __shared__ __attribute__((aligned(16))) float s_dist[TM_TILE][12];
    __shared__ __attribute__((aligned(16))) float s_or[TM_TILE][8];
    __shared__ int s_ix[2][2][TM_TILE];                      // [buffer][neighbour index | positional index][neighbour]
    const int tid = tm_tid(), lane = tid & 63, wv = tid >> 6, m = lane & 15, q = lane >> 4;
    const int c32 = lane & 31;
    const int col0 = (TM_H / NW) * wv, chunk0 = (32 / NW) * wv;

    float wedge[1][CA_K / 4], we[1][32];
    load_wfrag<CA_K / 16>(a.edge_ca, CA_K, col0, 0, TM_H, wedge[0], lane);
    load_wfrag<8>(a.We_w, TM_H, col0, 0, TM_H, we[0], lane);
    const f4 be = ld4(a.We_b + col0 + 4 * q);
    const f4 g4 = ld4(a.ln_w + 4 * c32), b4 = ld4(a.ln_b + 4 * c32);

    const TileRange tr = xcd_tile_range(a.T);
    int i = tr.begin, cur = 0, jn = -1;
    CaRaw raw;
    if (tid < TM_TILE && i < tr.end) {
        ca_load(a, i, tid, a.E_idx[(size_t)i * TM_KS + tid], raw);
        if (i + tr.step < tr.end) jn = a.E_idx[(size_t)(i + tr.step) * TM_KS + tid];
    }
    for (; i < tr.end; i += tr.step) {
        const int inext = i + tr.step;
        if (tid < TM_TILE) {
            ca_publish(raw, s_dist[tid], s_or[tid], &s_ix[cur][0][tid], &s_ix[cur][1][tid]);
            if (inext < tr.end) {                                // the next tile's rows, one tile ahead; its list entry came a tile earlier
                ca_load(a, inext, tid, jn, raw);
                if (inext + tr.step < tr.end) jn = a.E_idx[(size_t)(inext + tr.step) * TM_KS + tid];
            }
        }
        __syncthreads();
        for (int e = tid; e < TM_TILE * 36; e += NT) {           // 16 Gaussians per distance, 4 per thread-iteration (:1022-1031)
            const int mm = e / 36, c = e - mm * 36;
            const float D = s_dist[mm][c >> 2];
            const int r0 = (c & 3) * 4;
            f4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t = (D - a.mu[r0 + r]) * 0.8f;       // / sigma, sigma = 1.25
                v[r] = __expf(-(t * t));
            }
            st4(feat + chunk_off<CA_RS>(mm, c), v);
        }
        if (tid < TM_TILE * 4) {                                 // K columns 144..159: dU, Q, zeros
            const int row = tid >> 2, c = tid & 3;
            st4(feat + chunk_off<CA_RS>(row, 36 + c), c < 2 ? ld4(&s_or[row][4 * c]) : f4{0.f, 0.f, 0.f, 0.f});
        }
        __syncthreads();

        f4 acc[3][1];
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) acc[rb][0] = ld4(a.pos_table + s_ix[cur][1][16 * rb + m] * TM_H + col0 + 4 * q);
        mma_tile<CA_K / 16, 1, CA_RS>(feat, wedge, acc, lane);
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) st4(tA + chunk_off(16 * rb + m, chunk0 + q), acc[rb][0]);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < RPW / 2; ++it) {                   // norm_edges (:1079)
            const int row = RPW * wv + 2 * it + (lane >> 5);
            float *p = tA + chunk_off(row, c32);
            const f4 y = layer_norm_row(ld4(p), g4, b4);
            st4(p, y);
            if (a.E_opt) st4(a.E_opt + ((size_t)i * TM_KS + row) * TM_H + 4 * c32, s_ix[cur][0][row] >= 0 ? y : f4{0.f, 0.f, 0.f, 0.f});
        }
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) acc[rb][0] = be;
        mma_tile<8, 1>(tA, we, acc, lane);                       // W_e (:1229)
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) st4(tB + chunk_off(16 * rb + m, chunk0 + q), acc[rb][0]);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < RPW / 2; ++it) {
            const int row = RPW * wv + 2 * it + (lane >> 5);
            const f4 y = s_ix[cur][0][row] >= 0 ? ld4(tB + chunk_off(row, c32)) : f4{0.f, 0.f, 0.f, 0.f};
            st4(a.hE + ((size_t)i * TM_KS + row) * TM_H + 4 * c32, y);
        }
        cur ^= 1;
        // no barrier here: the next tile's publish writes s_dist / s_or (last read two barriers ago) and the OTHER s_ix buffer; tB is
        // rewritten four barriers from now
    }
}

// Split-precision form ("f16x2" and "bf16x3" handles): both GEMMs on the 16-bit matrix cores (tmpnn_split.h). The features are split
// into planes as they are generated; LayerNorm statistics are taken in the GEMM-1 epilogue and its output goes straight into the
// GEMM-2 operand planes; h_E rows leave from the accumulators.
template <typename SP>
__global__ __launch_bounds__(512, 2) void featurize_ca_split_kernel(CaFeatArgs a) {
    constexpr int PLB = TM_TILE * CA_ROWB;                   // bytes per feature plane
    __shared__ __attribute__((aligned(16))) char planes[SP::NP * PLB];
    __shared__ __attribute__((aligned(16))) char s_tA[SP::NP * SPLIT_PLANE_BYTES];
    __shared__ __attribute__((aligned(16))) float s_stat[TM_TILE][TM_STAT8_LD];
    __shared__ __attribute__((aligned(16))) float s_dist[TM_TILE][12];
    __shared__ __attribute__((aligned(16))) float s_or[TM_TILE][8];
    __shared__ int s_ix[2][2][TM_TILE];
    const int tid = tm_tid(), lane = tid & 63, wv = tid >> 6, m = lane & 15, q = lane >> 4;
    const int ncol = 16 * wv + 4 * q, c4 = 4 * wv + q;

    WFragS<SP> wedge[1][CA_K / 32], we[1][4];
    if constexpr (SP::NP == 2) {                             // f16x2: from the fragment images (coalesced 1 KB loads)
#pragma unroll
        for (int st = 0; st < CA_K / 32; ++st) {
            const char *p = a.img_e[st >> 2] + (size_t)wv * 8192 + (st & 3) * 2048 + lane * 16;
            wedge[0][st].p[0] = *reinterpret_cast<const u4 *>(p);
            wedge[0][st].p[1] = *reinterpret_cast<const u4 *>(p + 1024);
        }
    } else {
        load_wfrag_split<SP, CA_K / 32>(a.edge_ca, CA_K, 16 * wv, 0, CA_K, wedge[0], lane);
    }
    load_wfrag_auto<SP>(a.img_we, a.We_w, TM_H, wv, lane, we[0]);
    const f4 be = ld4(a.We_b + ncol), g4 = ld4(a.ln_w + ncol), b4 = ld4(a.ln_b + ncol);
    f4 mu4;                                                   // this thread's 4 Gaussian centres: (tid & 3) is fixed (36 and 512 are multiples of 4)
#pragma unroll
    for (int r = 0; r < 4; ++r) mu4[r] = a.mu[(tid & 3) * 4 + r];

    const TileRange tr = xcd_tile_range(a.T);
    int i = tr.begin, cur = 0, jn = -1;
    CaRaw raw;
    if (tid < TM_TILE && i < tr.end) {
        ca_load(a, i, tid, a.E_idx[(size_t)i * TM_KS + tid], raw);
        if (i + tr.step < tr.end) jn = a.E_idx[(size_t)(i + tr.step) * TM_KS + tid];
    }
    for (; i < tr.end; i += tr.step) {
        const int inext = i + tr.step;
        if (tid < TM_TILE) {
            ca_publish(raw, s_dist[tid], s_or[tid], &s_ix[cur][0][tid], &s_ix[cur][1][tid]);
            if (inext < tr.end) {
                ca_load(a, inext, tid, jn, raw);
                if (inext + tr.step < tr.end) jn = a.E_idx[(size_t)(inext + tr.step) * TM_KS + tid];
            }
        }
        __syncthreads();
        for (int e = tid; e < TM_TILE * 36; e += 512) {          // 16 Gaussians per distance, 4 per thread-iteration (:1022-1031)
            const int mm = e / 36, c = e - mm * 36;
            const float D = s_dist[mm][c >> 2];
            // exp(-((D - mu) / 1.25)^2) = exp2(-(t t)), t = (D - mu) * 0.8 sqrt(log2 e)
            const f2 t01 = (f2{D, D} - f2{mu4.x, mu4.y}) * 0.96089795f, t23 = (f2{D, D} - f2{mu4.z, mu4.w}) * 0.96089795f;
            const f2 e01 = -(t01 * t01), e23 = -(t23 * t23);
            store_split<SP, TM_TILE, CA_ROWB>(planes, mm, c, f4{__builtin_amdgcn_exp2f(e01.x), __builtin_amdgcn_exp2f(e01.y),
                                                                 __builtin_amdgcn_exp2f(e23.x), __builtin_amdgcn_exp2f(e23.y)});
        }
        if (tid < TM_TILE * 4) {                                 // K columns 144..159: dU, Q, zeros
            const int row = tid >> 2, c = tid & 3;
            store_split<SP, TM_TILE, CA_ROWB>(planes, row, 36 + c, c < 2 ? ld4(&s_or[row][4 * c]) : f4{0.f, 0.f, 0.f, 0.f});
        }
        __syncthreads();

        f4 acc[3][1];
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) acc[rb][0] = ld4(a.pos_table + s_ix[cur][1][16 * rb + m] * TM_H + ncol);
        mma_tile_split<SP, CA_K / 32, 1, 3, TM_TILE, CA_ROWB>(planes, wedge, acc, lane);
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) row_stats_partial1b(acc[rb][0], &s_stat[16 * rb + m][2 * wv], q);
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) {                         // norm_edges (:1079)
            const int row = 16 * rb + m;
            float mean, rstd;
            row_stats_finish8b(&s_stat[row][0], mean, rstd);
            const f4 y = (acc[rb][0] - mean) * rstd * g4 + b4;
            store_split<SP>(s_tA, row, c4, y);
            if (a.E_opt) st4(a.E_opt + ((size_t)i * TM_KS + row) * TM_H + ncol, s_ix[cur][0][row] >= 0 ? y : f4{0.f, 0.f, 0.f, 0.f});
        }
        __syncthreads();
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) acc[rb][0] = be;
        mma_tile_split<SP, 4, 1>(s_tA, we, acc, lane);           // W_e (:1229)
#pragma unroll
        for (int rb = 0; rb < 3; ++rb) {
            const int row = 16 * rb + m;
            st4(a.hE + ((size_t)i * TM_KS + row) * TM_H + ncol, s_ix[cur][0][row] >= 0 ? acc[rb][0] : f4{0.f, 0.f, 0.f, 0.f});
        }
        cur ^= 1;
        // no barrier here: the next publish writes s_dist / s_or (last read three barriers ago) and the OTHER s_ix buffer; the
        // feature planes, s_stat and s_tA are rewritten one, two and three barriers from now
    }
}

// ------------------------------------------------------------------------------------------------
// derived data of a CA handle: the positional table (as prep_pos_table_kernel, with the 167-column weight) and edge_ca
// ------------------------------------------------------------------------------------------------
__global__ void prep_ca_tables_kernel(const float *__restrict__ pos_w, const float *__restrict__ pos_b, const float *__restrict__ edge_w,
                                      float *__restrict__ table, float *__restrict__ edge_ca) {
    const int b = tm_bid(), n = tm_tid();       // 66 + 128 workgroups x 128 threads
    if (b < 66) {
        float s = 0.f;
        for (int p = 0; p < 16; ++p) s += (pos_w[p * 66 + b] + pos_b[p]) * edge_w[n * 167 + p];
        table[b * TM_H + n] = s;
    } else {
        const int r = b - 66;
        for (int k = n; k < CA_K; k += TM_H) edge_ca[r * CA_K + k] = k < 151 ? edge_w[r * 167 + 16 + k] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
int launch_prep_ca(tmpnn_weights *w, hipStream_t st) {
    prep_ca_tables_kernel<<<66 + TM_H, TM_H, 0, st>>>(w->pos_w, w->pos_b, w->edge_w, w->pos_table, w->edge_ca);
    return tm_check_launch("prep_ca_tables");
}

int launch_ca_frames(const float *X, const int32_t *offsets, int N, int64_t T, float *O, hipStream_t st) {
    tm_prof_begin("ca_frames", st);
    ca_frames_kernel<<<(int)((T + TM_THREADS - 1) / TM_THREADS), TM_THREADS, 0, st>>>(X, offsets, N, (int)T, O);
    tm_prof_end(st);
    return tm_check_launch("ca_frames");
}

int launch_featurize_ca(const tmpnn_weights *w, const float *X, const float *O, const int32_t *offsets, int N, const int32_t *ridx,
                        const int32_t *cenc, const int32_t *E_idx, const float *D_nb, int64_t T, float *h_E, float *E_opt, hipStream_t st) {
    CaFeatArgs a;
    a.edge_ca = w->edge_ca; a.pos_table = w->pos_table; a.ln_w = w->norm_edges_w; a.ln_b = w->norm_edges_b; a.We_w = w->We_w; a.We_b = w->We_b;
    a.X = X; a.O = O; a.offsets = offsets; a.ridx = ridx; a.cenc = cenc; a.E_idx = E_idx; a.D_nb = D_nb; a.hE = h_E; a.E_opt = E_opt;
    a.N = N; a.T = (int)T;
    for (int i = 0; i < 16; ++i)   // torch.linspace(2, 22, 16): double arithmetic, symmetric halves, cast to fp32
        a.mu[i] = i < 8 ? (float)(2.0 + (20.0 / 15.0) * i) : (float)(22.0 - (20.0 / 15.0) * (15 - i));
    a.img_e[0] = w->feat_img.edge[0]; a.img_e[1] = w->feat_img.edge[1]; a.img_we = w->feat_img.we;
    if (w->mode == TM_MM_F16X2 && (!a.img_e[0] || !a.img_e[1] || !a.img_we))
        return tm_set_error(TMPNN_E_INVALID, "edge_featurize: f16x2 CA handle without the fragment images of W_edge / W_e");
    const int64_t cap = tm_num_cus();
    const int grid = (int)(T < cap ? T : cap);
    tm_prof_begin("featurize_ca", st);
    if (w->mode == TM_MM_F16X2) featurize_ca_split_kernel<SplitH2><<<grid, 512, 0, st>>>(a);
    else if (w->mode == TM_MM_BF16X3) featurize_ca_split_kernel<SplitBF3><<<grid, 512, 0, st>>>(a);
    else featurize_ca_kernel<<<grid, 512, 0, st>>>(a);
    tm_prof_end(st);
    return tm_check_launch("edge_featurize_ca");
}
