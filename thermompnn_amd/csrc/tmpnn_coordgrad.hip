// Gradients with respect to the backbone coordinates (gfx950): the stage that tmpnn_finetune_backward_x / tmpnn_seqloss_backward_x /
// tmpnn_seqloss_batch_backward_x add at the tail of ft_backward (tmpnn_finetune.hip). ft_backward has formed dE0 = dL / d(edge_embedding
// output) and, with ft_linear_t, dRBF [E,400] = dE0 W_edge[:, 16:416]; the two kernels here take dRBF through the 16 RBFs, the 25
// atom-pair distances and the virtual Cb to dX [L,4,3]. Reference: the featurizer of model_utils.py:314-381 (= protein_mpnn_utils.py:
// 1101-1168), which torch differentiates there. No float atomics, fixed summation orders: reruns give identical bits.
#include <math.h>
#include <stdint.h>

#include "tmpnn_ft.h"

// The graph (eidx) and D_max of _dist are constants: pair 0 of a masked (i, j) has the constant distance D_max and gives nothing; the
// other 24 pairs of a masked neighbour go through its coordinates like any other's.
//
// One wavefront per edge e = (i, k), j = eidx[e]. Lane l of pass t reads column 64 t + l of dRBF [E,400] and of the saved RBF (Ein + 16):
// whole lines; the 16 lanes of a group hold the 16 centres of pair p = 4 t + (l >> 4), and a 16-lane butterfly leaves
//   dD_p = sum_r dRBF[e, 16 p + r] RBF[e, 16 p + r] (-1.28 (D_p - mu_r))          (d exp(-(0.8 (D - mu))^2) / dD)
// in all of them. cf_p = dD_p / D_p (pair 0: mask_i mask_j dD_0 / sqrt(|Ca_i - Ca_j|^2 + 1e-6)). Lane o < 15 then sums, p = 0..24 in
// order, the pairs whose first atom is o / 3 into out[e][o] (row i's atoms N, Ca, C, O, Cb), lane 15 + o the pairs whose second atom is
// o / 3 into out[e][15 + o] (row j's): + / - cf_p (A - B). out [E,32], 30 used.
struct FtDxEdge { const float *X, *mask, *D48, *Ein, *dR; const int32_t *eidx; float *out; int L, K; };

__global__ __launch_bounds__(TM_THREADS) void ft_dx_edge_kernel(FtDxEdge a) {
    __shared__ float s_at[4][32], s_cf[4][28];
    const int lane = tm_tid() & 63, wv = tm_wave(tm_tid()), g = lane >> 4, r = lane & 15;
    const int64_t E = (int64_t)a.L * a.K;
    const float mu = r < 8 ? (float)(2.0 + (20.0 / 15.0) * r) : (float)(22.0 - (20.0 / 15.0) * (15 - r));
    for (int64_t e0 = (int64_t)tm_bid() * 4; e0 < E; e0 += (int64_t)tm_nblk() * 4) {       // (uniform over the workgroup: barriers inside)
        const bool ok = e0 + wv < E;
        const int64_t e = ok ? e0 + wv : E - 1;
        const int i = (int)(e / a.K), k = (int)(e - (int64_t)i * a.K);
        const int j = min(max(a.eidx[e], 0), a.L - 1);
        if (lane < 30) {                                          // the 5 atoms of row i, then of row j
            float o[3];
            const int row = lane < 15 ? i : j, q = lane < 15 ? lane : lane - 15;
            ft_atom(a.X + (size_t)row * 12, q / 3, o);
            s_at[wv][lane] = o[q % 3];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const int p = 4 * t + g, col = 64 * t + lane;
            float v = 0.f, D = 1.f, Dt = 1.f;
            if (p < 25) {
                const float *A = &s_at[wv][3 * c_ft_pa[p]], *B = &s_at[wv][15 + 3 * c_ft_pb[p]];
                const float dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
                Dt = sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
                D = p == 0 ? a.D48[(size_t)i * TM_KS + k] : Dt;
                v = a.dR[(size_t)e * 400 + col] * a.Ein[(size_t)e * 416 + 16 + col] * (-1.28f * (D - mu));
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (p < 25 && r == 0) s_cf[wv][p] = (p == 0 ? a.mask[i] * a.mask[j] * v : v) / Dt;
        }
        __syncthreads();
        if (lane < 30 && ok) {
            const bool first = lane < 15;
            const int q = first ? lane : lane - 15, at = q / 3, cc = q - 3 * at;
            float s = 0.f;
            for (int p = 0; p < 25; ++p) {
                if ((first ? c_ft_pa[p] : c_ft_pb[p]) != at) continue;
                const float d = s_at[wv][3 * c_ft_pa[p] + cc] - s_at[wv][15 + 3 * c_ft_pb[p] + cc];
                s += s_cf[wv][p] * d;
            }
            a.out[(size_t)e * 32 + lane] = first ? s : -s;
        }
        __syncthreads();
    }
}

// 16 lanes per residue i. Lane o < 15: g[o] = sum_k ge[i K + k][o] + sum over the edges whose neighbour is i (the CSR, ascending e) of
// ge[e][15 + o]. Then the chain rule of Cb = -0.58273431 (b x c) + 0.56802827 b - 0.54067466 c + Ca, b = Ca - N, c = C - Ca, with
// g = g[Cb]:  db = -0.58273431 (c x g) + 0.56802827 g,  dc = -0.58273431 (g x b) - 0.54067466 g;
// dN = g[N] - db, dCa = g[Ca] + g + db - dc, dC = g[C] + dc, dO = g[O]. Lane o < 12 writes dX[i][o].
struct FtDxNode { const float *X, *ge; const int32_t *off, *list; float *dX; int L, K; };

__global__ __launch_bounds__(TM_THREADS) void ft_dx_node_kernel(FtDxNode a) {
    const int o = tm_tid() & 15, grp = tm_tid() >> 4, gl = (tm_tid() & 63) & ~15;        // gl: the group's first lane in its wavefront
    const int n_it = (a.L + tm_nblk() * 16 - 1) / (tm_nblk() * 16);
    for (int it = 0; it < n_it; ++it) {                                                   // (uniform: shuffles inside)
        const int i0 = (it * tm_nblk() + tm_bid()) * 16 + grp;
        const bool ok = i0 < a.L;
        const int i = ok ? i0 : a.L - 1;
        float s = 0.f;
        if (o < 15) {
            for (int k = 0; k < a.K; ++k) s += a.ge[((size_t)i * a.K + k) * 32 + o];
            for (int u = a.off[i]; u < a.off[i + 1]; ++u) s += a.ge[(size_t)a.list[u] * 32 + 15 + o];
        }
        float gc[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) gc[d] = __shfl(s, gl + 12 + d, 64);
        const float *x = a.X + (size_t)i * 12;
        float b[3], c[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) { b[d] = x[3 + d] - x[d]; c[d] = x[6 + d] - x[3 + d]; }
        const float cg[3] = {c[1] * gc[2] - c[2] * gc[1], c[2] * gc[0] - c[0] * gc[2], c[0] * gc[1] - c[1] * gc[0]};
        const float gb[3] = {gc[1] * b[2] - gc[2] * b[1], gc[2] * b[0] - gc[0] * b[2], gc[0] * b[1] - gc[1] * b[0]};
        const int at = o / 3, d = o - 3 * at;
        const float cgd = d == 0 ? cg[0] : d == 1 ? cg[1] : cg[2], gbd = d == 0 ? gb[0] : d == 1 ? gb[1] : gb[2];
        const float gd = d == 0 ? gc[0] : d == 1 ? gc[1] : gc[2];
        const float db = -0.58273431f * cgd + 0.56802827f * gd, dc = -0.58273431f * gbd - 0.54067466f * gd;
        const float out = at == 0 ? s - db : at == 1 ? s + gd + db - dc : at == 2 ? s + dc : s;
        if (ok && o < 12) a.dX[(size_t)i * 12 + o] = out;
    }
}

void ft_coord_grad(const FtCtx &c, const float *dRBF) {
    const FtWs &w = c.w;
    const int64_t cap = (int64_t)tm_num_cus() * 8;
    auto grid = [&](int64_t blocks) { return (int)(blocks < 1 ? 1 : blocks < cap ? blocks : cap); };
    FtDxEdge de{c.X, c.mask, w.D48, w.Ein, dRBF, w.eidx, w.tm, c.L, c.K};
    ft_dx_edge_kernel<<<grid((c.E + 3) / 4), TM_THREADS, 0, c.st>>>(de);                    // 4 wavefronts, 4 edges per workgroup
    FtDxNode dn{c.X, w.tm, w.coff, w.clist, c.dX, c.L, c.K};
    ft_dx_node_kernel<<<grid(((int64_t)c.L + 15) / 16), TM_THREADS, 0, c.st>>>(dn);          // 16 lanes per residue, 16 per workgroup
}
