// Rigid-body superposition of the members of conformer ensembles (gfx950): for every member m of ensemble e the proper rotation and the
// translation that lay its C-alpha atoms on those of the ensemble's member fit_to in the least-squares sense, the RMSD of that fit, the
// per-column deviation, and per axis column the fluctuation of the superposed members around their mean (tmpnn_superpose,
// include/tmpnn.h). It reads what an ensemble scan already holds on the device before its forward runs: the packed backbone X [T,4,3]
// (atom slot 1 only), mask [T] and the row map tmpnn_align_global wrote (or none: the identity map).
//
// Float work: float64 throughout, written with plain operators under `#pragma clang fp contract(off)`, rounded to fp32 once where an
// output is fp32. This file is built WITHOUT -fno-honor-nans (build.py FILE_FLAGS): mask > 0 has to be false for a NaN mask, and NaN
// is a result here. Finiteness of a coordinate is tested on its exponent bits; a NaN result is written as 0x7fc00000.
//
// LAUNCH 1, sup_fit_kernel: one workgroup of 256 threads per member slot g < NM. The workgroup first FINDS its ensemble: the smallest e
// whose descriptor passes the checks and has mem0 <= g < mem0 + M (thread t tests e = t, t + 256, ...; a minimum over the workgroup).
// The host does not know M, so it cannot shape a grid per ensemble; a slot no good ensemble names is left alone. Then three sweeps over
// the member's L columns, thread t taking q = t, t + 256, ... in ascending order:
//   1. n_fit and the two coordinate sums over the fit set -> the centroids
//   2. the 3 x 3 covariance of the centred coordinates
//   3. the residuals |R p_m + t - p_f|: dev per column, their squares' sum -> rmsd
// Every sum is folded the same way: a wavefront folds its 64 lanes at distances 32, 16, .. 1 (lane l takes lane l + distance), the four
// wavefront sums are added in ascending order, and every thread does that last addition itself, so all hold the same bits. Between
// sweeps 2 and 3 thread 0 solves Horn's 4 x 4 quaternion matrix by cyclic Jacobi (rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) per
// sweep, compile-time indices: the two matrices stay in registers) and leaves R, t in LDS. The eigenvector of the largest eigenvalue is
// a unit quaternion, so R is a proper rotation for ANY point set: a mirrored member, collinear points and a single point need no case.
// LAUNCH 2, sup_col_kernel: one thread per (ensemble, column) on a grid of (ceil(max_len / 256), E), as tmpnn_ensemble_stats'; two
// loops over the members in ascending order (the mean, then the squared distances from it) through the xform launch 1 wrote. It writes
// status. No atomics, no workspace: every output word has one writer, and the order of every sum depends on (M, L, the data) only.
#include <stdint.h>

#include "tmpnn_internal.h"

#pragma clang fp contract(off)

#define SUP_THREADS 256
#define SUP_WAVES (SUP_THREADS / 64)
#define SUP_MAX_LEN 8192            // the forward's own bound
#define SUP_MAX_E 65535             // grid.y of launch 2
#define SUP_NAN 0x7fc00000u
#define SUP_MAX_SWEEPS 32

struct SupArgs {
    const float *X;                 // [T, 4, 3]
    const float *mask;              // [T]
    const int32_t *rows;            // [R] or null: the identity map
    const int32_t *desc;            // [E, 6] = (map0, M, L, out_row0, mem0, fit_to)
    int64_t R, T, NM, T_out;
    int E, max_len;
    int32_t *n_fit;                 // [NM]
    float *rmsd;                    // [NM]
    double *xform;                  // [NM, 12]
    float *dev;                     // [R]
    float *rmsf;                    // [T_out]
    int32_t *col_count;             // [T_out]
    int32_t *status;                // [E]
};

struct SupDesc {
    int64_t map0, M, L, out0, mem0, fit;
};

// the descriptor of ensemble e and whether it passes the checks, in 64-bit arithmetic (M, L < 2^31: M L < 2^62)
__device__ __forceinline__ bool sup_desc(const SupArgs &a, int e, SupDesc &d) {
    const int32_t *p = a.desc + 6 * (int64_t)e;
    d.map0 = p[0], d.M = p[1], d.L = p[2], d.out0 = p[3], d.mem0 = p[4], d.fit = p[5];
    return d.map0 >= 0 && d.M >= 0 && d.L >= 0 && d.out0 >= 0 && d.mem0 >= 0 && d.L <= a.max_len && d.map0 + d.M * d.L <= a.R &&
           (a.rows != nullptr || d.map0 + d.M * d.L <= a.T) && d.out0 + d.L <= a.T_out && d.mem0 + d.M <= a.NM &&
           (d.M == 0 || (d.fit >= 0 && d.fit < d.M));
}

__device__ __forceinline__ bool sup_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// (m, q) of a good ensemble -> its C-alpha, or false: the map entry is no row of X, the row is masked or a coordinate is not finite
__device__ __forceinline__ bool sup_point(const SupArgs &a, const SupDesc &d, int64_t m, int64_t q, double &x, double &y, double &z) {
    const int64_t at = d.map0 + m * d.L + q;
    uint32_t r = (uint32_t)at;                                                // (rows null: at < T <= 2^31 - 1, the descriptor check)
    if (a.rows) r = (uint32_t)a.rows[at];
    if (r >= (uint32_t)a.T) return false;
    if (!(a.mask[r] > 0.0f)) return false;
    const float *p = a.X + (int64_t)r * 12 + 3;
    const float fx = p[0], fy = p[1], fz = p[2];
    if (!(sup_finite(fx) && sup_finite(fy) && sup_finite(fz))) return false;
    x = (double)fx, y = (double)fy, z = (double)fz;
    return true;
}

// v[0 .. K) summed over the workgroup; every thread returns with the same bits. red is free again on return.
template <int K> __device__ __forceinline__ void sup_reduce(double (&v)[K], double (*red)[SUP_WAVES]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = v[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_down(s, off, 64);
        if (lane == 0) red[k][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = red[k][0];
#pragma unroll
        for (int w = 1; w < SUP_WAVES; ++w) s = s + red[k][w];
        v[k] = s;
    }
    __syncthreads();
}

// one Jacobi rotation that zeroes A[P][Q] of the symmetric A, accumulated into V's columns P and Q
template <int P, int Q> __device__ __forceinline__ void sup_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));          // (theta^2 = inf: tt = 0, apq is below A's rounding)
    const double t = theta < 0.0 ? -tt : tt;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// S[a][b] = sum (p_m - c_m)_a (p_f - c_f)_b -> the rotation (row-major) of the unit quaternion that is the eigenvector of the largest
// eigenvalue of Horn's matrix (ties: the first column). S = 0 gives the identity.
__device__ __forceinline__ void sup_solve(const double (&S)[9], double (&Rm)[9]) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4], V[4][4];
    A[0][0] = Sxx + Syy + Szz;
    A[1][1] = Sxx - Syy - Szz;
    A[2][2] = Syy - Sxx - Szz;
    A[3][3] = Szz - Sxx - Syy;
    A[0][1] = A[1][0] = Syz - Szy;
    A[0][2] = A[2][0] = Szx - Sxz;
    A[0][3] = A[3][0] = Sxy - Syx;
    A[1][2] = A[2][1] = Sxy + Syx;
    A[1][3] = A[3][1] = Szx + Sxz;
    A[2][3] = A[3][2] = Syz + Szy;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < SUP_MAX_SWEEPS; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3];
        const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
        if (off <= 1e-40 * dia) break;                                        // (|off-diagonal| <= 1e-20 |diagonal|, or both 0)
        sup_rotate<0, 1>(A, V);
        sup_rotate<0, 2>(A, V);
        sup_rotate<0, 3>(A, V);
        sup_rotate<1, 2>(A, V);
        sup_rotate<1, 3>(A, V);
        sup_rotate<2, 3>(A, V);
    }
    double best = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > best) best = A[k][k], w = V[0][k], x = V[1][k], y = V[2][k], z = V[3][k];
    const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);             // (V is orthogonal to rounding: the norm is 1 +- a few ulps)
    w = w * inv, x = x * inv, y = y * inv, z = z * inv;
    Rm[0] = w * w + x * x - y * y - z * z;
    Rm[1] = 2.0 * (x * y - w * z);
    Rm[2] = 2.0 * (x * z + w * y);
    Rm[3] = 2.0 * (x * y + w * z);
    Rm[4] = w * w - x * x + y * y - z * z;
    Rm[5] = 2.0 * (y * z - w * x);
    Rm[6] = 2.0 * (x * z - w * y);
    Rm[7] = 2.0 * (y * z + w * x);
    Rm[8] = w * w - x * x - y * y + z * z;
}

struct SupShared {
    double red[9][SUP_WAVES];
    double xf[12];
    int found[SUP_WAVES];
};

__global__ __launch_bounds__(SUP_THREADS) void sup_fit_kernel(SupArgs a) {
    __shared__ SupShared sh;
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    // the smallest good ensemble that names member slot g
    int e = 0x7fffffff;
    SupDesc d;
    for (int c = tid; c < a.E; c += SUP_THREADS)
        if (sup_desc(a, c, d) && d.mem0 <= g && g < d.mem0 + d.M) {
            e = c;
            break;
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) e = min(e, __shfl_down(e, off, 64));
    if ((tid & 63) == 0) sh.found[tid >> 6] = e;
    __syncthreads();
    e = sh.found[0];
#pragma unroll
    for (int w = 1; w < SUP_WAVES; ++w) e = min(e, sh.found[w]);
    if (e == 0x7fffffff) return;                                              // (uniform)
    sup_desc(a, e, d);
    const int64_t m = g - d.mem0, f = d.fit, L = d.L;
    float *dev = a.dev + d.map0 + m * L;

    // sweep 1: the fit set's size and coordinate sums
    double v1[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t q = tid; q < L; q += SUP_THREADS) {
        double mx, my, mz, fx, fy, fz;
        if (!sup_point(a, d, m, q, mx, my, mz) || !sup_point(a, d, f, q, fx, fy, fz)) continue;
        v1[0] = v1[0] + 1.0;
        v1[1] = v1[1] + mx, v1[2] = v1[2] + my, v1[3] = v1[3] + mz;
        v1[4] = v1[4] + fx, v1[5] = v1[5] + fy, v1[6] = v1[6] + fz;
    }
    sup_reduce<7>(v1, sh.red);
    const int n = (int)v1[0];                                                 // (a sum of at most 8192 ones: exact)
    const bool self = m == f;
    if (n == 0 || self) {                                                     // R = I, t = 0 exactly; the fit target is its own image
        if (tid < 12) a.xform[g * 12 + tid] = (tid == 0 || tid == 4 || tid == 8) ? 1.0 : 0.0;
        if (tid == 0) {
            a.n_fit[g] = n;
            a.rmsd[g] = __uint_as_float(n == 0 ? SUP_NAN : 0u);
        }
        for (int64_t q = tid; q < L; q += SUP_THREADS) {
            double x, y, z;
            dev[q] = __uint_as_float(self && sup_point(a, d, m, q, x, y, z) ? 0u : SUP_NAN);
        }
        return;
    }
    const double dn = (double)n;
    const double cmx = v1[1] / dn, cmy = v1[2] / dn, cmz = v1[3] / dn, cfx = v1[4] / dn, cfy = v1[5] / dn, cfz = v1[6] / dn;

    // sweep 2: the covariance of the centred coordinates
    double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t q = tid; q < L; q += SUP_THREADS) {
        double mx, my, mz, fx, fy, fz;
        if (!sup_point(a, d, m, q, mx, my, mz) || !sup_point(a, d, f, q, fx, fy, fz)) continue;
        mx = mx - cmx, my = my - cmy, mz = mz - cmz;
        fx = fx - cfx, fy = fy - cfy, fz = fz - cfz;
        S[0] = S[0] + mx * fx, S[1] = S[1] + mx * fy, S[2] = S[2] + mx * fz;
        S[3] = S[3] + my * fx, S[4] = S[4] + my * fy, S[5] = S[5] + my * fz;
        S[6] = S[6] + mz * fx, S[7] = S[7] + mz * fy, S[8] = S[8] + mz * fz;
    }
    sup_reduce<9>(S, sh.red);
    if (tid == 0) {
        double Rm[9];
        sup_solve(S, Rm);
#pragma unroll
        for (int k = 0; k < 9; ++k) sh.xf[k] = Rm[k];
        sh.xf[9] = cfx - (Rm[0] * cmx + Rm[1] * cmy + Rm[2] * cmz);
        sh.xf[10] = cfy - (Rm[3] * cmx + Rm[4] * cmy + Rm[5] * cmz);
        sh.xf[11] = cfz - (Rm[6] * cmx + Rm[7] * cmy + Rm[8] * cmz);
    }
    __syncthreads();
    double xf[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) xf[k] = sh.xf[k];
    if (tid < 12) a.xform[g * 12 + tid] = sh.xf[tid];

    // sweep 3: the residuals
    double v3[1] = {0.0};
    for (int64_t q = tid; q < L; q += SUP_THREADS) {
        double mx, my, mz, fx, fy, fz;
        uint32_t bits = SUP_NAN;
        if (sup_point(a, d, m, q, mx, my, mz) && sup_point(a, d, f, q, fx, fy, fz)) {
            const double dx = (xf[0] * mx + xf[1] * my + xf[2] * mz + xf[9]) - fx;
            const double dy = (xf[3] * mx + xf[4] * my + xf[5] * mz + xf[10]) - fy;
            const double dz = (xf[6] * mx + xf[7] * my + xf[8] * mz + xf[11]) - fz;
            const double d2 = dx * dx + dy * dy + dz * dz;
            v3[0] = v3[0] + d2;
            if (n >= 3) bits = __float_as_uint((float)sqrt(d2));
        }
        dev[q] = __uint_as_float(bits);
    }
    sup_reduce<1>(v3, sh.red);
    if (tid == 0) {
        a.n_fit[g] = n;
        a.rmsd[g] = (float)sqrt(v3[0] / dn);
    }
}

__global__ __launch_bounds__(SUP_THREADS) void sup_col_kernel(SupArgs a) {
    const int e = blockIdx.y;
    SupDesc d;
    const bool ok = sup_desc(a, e, d);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[e] = ok ? 0 : -1;
    if (!ok) return;
    const int64_t q = (int64_t)blockIdx.x * SUP_THREADS + threadIdx.x;
    if (q >= d.L) return;
    // pass 1, ascending m: the mean of the superposed members
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int n = 0;
    for (int64_t m = 0; m < d.M; ++m) {
        if (m != d.fit && a.n_fit[d.mem0 + m] < 3) continue;
        double x, y, z;
        if (!sup_point(a, d, m, q, x, y, z)) continue;
        const double *xf = a.xform + (d.mem0 + m) * 12;
        sx = sx + (xf[0] * x + xf[1] * y + xf[2] * z + xf[9]);
        sy = sy + (xf[3] * x + xf[4] * y + xf[5] * z + xf[10]);
        sz = sz + (xf[6] * x + xf[7] * y + xf[8] * z + xf[11]);
        ++n;
    }
    uint32_t bits = SUP_NAN;
    if (n > 0) {
        const double dn = (double)n;
        const double ux = sx / dn, uy = sy / dn, uz = sz / dn;
        // pass 2, ascending m again: the squared distances from it
        double t = 0.0;
        for (int64_t m = 0; m < d.M; ++m) {
            if (m != d.fit && a.n_fit[d.mem0 + m] < 3) continue;
            double x, y, z;
            if (!sup_point(a, d, m, q, x, y, z)) continue;
            const double *xf = a.xform + (d.mem0 + m) * 12;
            const double dx = (xf[0] * x + xf[1] * y + xf[2] * z + xf[9]) - ux;
            const double dy = (xf[3] * x + xf[4] * y + xf[5] * z + xf[10]) - uy;
            const double dz = (xf[6] * x + xf[7] * y + xf[8] * z + xf[11]) - uz;
            t = t + (dx * dx + dy * dy + dz * dz);
        }
        bits = __float_as_uint((float)sqrt(t / dn));
    }
    a.rmsf[d.out0 + q] = __uint_as_float(bits);
    a.col_count[d.out0 + q] = n;
}

// ---- the C-ABI entry ------------------------------------------------------------------------------------------------------------
extern "C" int tmpnn_superpose(const float *X, const float *mask, const int32_t *rows, int64_t R, const int32_t *desc, int E, int64_t T,
                               int64_t NM, int64_t T_out, int max_len, int32_t *n_fit, float *rmsd, double *xform, float *dev, float *rmsf,
                               int32_t *col_count, int32_t *status, tmpnn_stream_t stream) {
    if (E < 0 || T < 0 || T_out < 0 || max_len < 0 || R < 0 || NM < 0)
        return tm_set_error(TMPNN_E_INVALID, "superpose: bad sizes (E=%d, T=%lld, T_out=%lld, max_len=%d, R=%lld, NM=%lld)", E, (long long)T,
                            (long long)T_out, max_len, (long long)R, (long long)NM);
    if ((T > 0 && (!X || !mask)) || (E > 0 && (!desc || !status)) || (R > 0 && !dev) || (NM > 0 && (!n_fit || !rmsd || !xform)) ||
        (T_out > 0 && (!rmsf || !col_count)))
        return tm_set_error(TMPNN_E_INVALID, "superpose: null pointer");
    if (T > (int64_t)0x7fffffff || T_out > (int64_t)0x7fffffff || R > (int64_t)0x7fffffff || NM > (int64_t)0x7fffffff)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "superpose: T=%lld, T_out=%lld, R=%lld or NM=%lld exceeds 2^31 - 1", (long long)T,
                            (long long)T_out, (long long)R, (long long)NM);
    if (max_len > SUP_MAX_LEN) return tm_set_error(TMPNN_E_UNSUPPORTED, "superpose: max_len=%d exceeds %d", max_len, SUP_MAX_LEN);
    if (E > SUP_MAX_E) return tm_set_error(TMPNN_E_UNSUPPORTED, "superpose: E=%d exceeds %d ensembles per call", E, SUP_MAX_E);
    if (E == 0) return TMPNN_OK;
    const SupArgs a{X, mask, rows, desc, R, T, NM, T_out, E, max_len, n_fit, rmsd, xform, dev, rmsf, col_count, status};
    hipStream_t st = (hipStream_t)stream;
    if (NM > 0) {
        tm_prof_begin("sup_fit", st);
        hipLaunchKernelGGL(sup_fit_kernel, dim3((unsigned)NM), dim3(SUP_THREADS), 0, st, a);
        tm_prof_end(st);
        const int rc = tm_check_launch("sup_fit_kernel");
        if (rc != TMPNN_OK) return rc;
    }
    const unsigned gx = max_len > 0 ? (unsigned)((max_len + SUP_THREADS - 1) / SUP_THREADS) : 1u;   // (<= 32; one group still writes status)
    tm_prof_begin("sup_col", st);
    hipLaunchKernelGGL(sup_col_kernel, dim3(gx, (unsigned)E), dim3(SUP_THREADS), 0, st, a);
    tm_prof_end(st);
    return tm_check_launch("sup_col_kernel");
}
