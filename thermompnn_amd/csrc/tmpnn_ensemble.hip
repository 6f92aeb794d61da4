// Per-mutation statistics over conformer ensembles (gfx950): for every ensemble e of M members of L rows each in a packed ddG table,
// and every (position q, letter b), the mean, the population spread, the smallest and the largest ddG with the members that hold them,
// the number of members that take part and the number of those at or below a cutoff (tmpnn_ensemble_stats, include/tmpnn.h). The
// members of an ensemble are exactly a ragged packed batch of the fused forward (whose tables do not depend on the batch), so an
// ensemble scan is one forward plus this one launch; no [E, M, L, 20] view is padded and no table goes to the host.
//
// Float work: a chain of fp32 round-to-nearest adds in ASCENDING member order, a divide, then per member one subtract, one multiply and
// one add that must stay three operations, a divide and a square root. They are written with plain operators under
// `#pragma clang fp contract(off)`: the pragma is lexical, so it does not reach the __fmul_rn / __fadd_rn of the HIP headers, which
// this compiler fuses into one v_fma_f32 when they meet after inlining. The divides and the root are written in double and rounded
// to float: 53 >= 2 * 24 + 2 bits, so the result is the correctly rounded float one (and the compiler may, and does, make the divide
// a correctly rounded fp32 one). This file is built WITHOUT -fno-honor-nans (build.py FILE_FLAGS), as tmpnn_pair_map.hip is: inf - inf is a NaN
// that has to be seen. The NaN tests are made on the bits all the same, and a NaN result is written as 0x7fc00000.
//
// KEYS of member m's value x (hits_ord: tmpnn_hits.h; -0.0 taken as +0.0, +-inf ordinary values):
//     lo    hits_ord(bits(x)) << 32 | m        the smallest key = the smallest value, then the smallest m
//     hi   ~hits_ord(bits(x)) << 32 | m        the smallest key = the largest value, then the smallest m
// The loop runs in ascending m, so a strict compare on the high words alone keeps the first member of a tie.
//
// ONE LAUNCH, a grid of (ceil(20 max_len / 256), E) workgroups of 256 threads: thread i of ensemble e owns output entry (q, b) =
// (i / 20, i % 20). Consecutive lanes read consecutive words of a table row (rows of ld = 21 follow each other with a one-word gap:
// near-coalesced without an LDS stage); pass 1 over the members makes the sum, the keys and the counts, pass 2 re-reads the same words
// (L2 hits) for the deviations. Every thread first checks its ensemble's descriptor in 64-bit arithmetic; an ensemble that fails writes
// status -1 and nothing else. No LDS, no barriers, no workspace, no atomics: every output entry has one writer.
//
// TWO FORMS of the one kernel, templated on the addressing. Plain (tmpnn_ensemble_stats): member m's position q is table row
// row0 + m L + q. Through a row map (tmpnn_ensemble_stats_rows, for members of unequal length that tmpnn_align_global has laid on one
// axis): the row is rows[map0 + m L + q], and the member is out at q unless (uint32)row < T. Everything behind the row is shared, and
// the plain form compiles to the instructions it had before the map form existed.
#include <stdint.h>

#include "tmpnn_internal.h"
#include "tmpnn_hits.h"

#pragma clang fp contract(off)

#define ENS_THREADS 256
#define ENS_MAX_LEN 8192            // the forward's own bound
#define ENS_MAX_E 65535             // grid.y
#define ENS_NAN 0x7fc00000u

struct EnsArgs {
    const float *ddg;               // [T, ld]
    int ld;
    const int32_t *S;               // [T]
    const int32_t *desc;            // [E, 4] = (row0, M, L, out_row0)
    int64_t T, T_out;
    int max_len;
    float cutoff;
    float *mean, *spread, *lo, *hi; // [T_out, 20] each
    int32_t *lo_member, *hi_member, *count, *below;
    int32_t *status;                // [E]
    const int32_t *rows;            // [R]: the form through a row map only (last, so that the plain form's fields stay where they were)
    int64_t R;
};

__device__ __forceinline__ bool ens_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ uint32_t ens_canon(float x) {
    const uint32_t b = __float_as_uint(x);
    return ens_is_nan(b) ? ENS_NAN : b;
}

// Member m's position q -> its table row. The plain form: row0 + m L + q, always a row of the table (the descriptor check). ROWS: the
// entry rows[row0 + m L + q] of the map (row0 is the descriptor's map0), a row when (uint32)r < T; anything else: the member is out.
template <bool ROWS> __device__ __forceinline__ bool ens_row(const EnsArgs &a, int64_t row0, int64_t m, int64_t L, int64_t q, int64_t &row) {
    row = row0 + m * L + q;
    if (ROWS) {
        const uint32_t r = (uint32_t)a.rows[row];
        row = (int64_t)r;
        return r < (uint32_t)a.T;                                             // (T <= 2^31 - 1: the entry's own bound)
    }
    return true;
}

template <bool ROWS> __global__ __launch_bounds__(ENS_THREADS) void ens_stats_kernel(EnsArgs a) {
    const int e = blockIdx.y;
    const int64_t row0 = a.desc[4 * e], M = a.desc[4 * e + 1], L = a.desc[4 * e + 2], out0 = a.desc[4 * e + 3];
    // (M, L < 2^31: M L < 2^62 and the sums below stay inside int64)
    const bool ok = row0 >= 0 && M >= 0 && L >= 0 && out0 >= 0 && L <= a.max_len && row0 + M * L <= (ROWS ? a.R : a.T) && out0 + L <= a.T_out;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.status[e] = ok ? 0 : -1;
    if (!ok) return;
    const int64_t i = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x;
    if (i >= 20 * L) return;
    const int64_t q = i / 20;
    const int b = (int)(i - q * 20);

    // pass 1, ascending m: the order of the sum is the contract
    float s = 0.0f;
    int n = 0, below = 0;
    uint32_t o_lo = 0, o_hi = 0, x_lo = ENS_NAN, x_hi = ENS_NAN;
    int32_t m_lo = -1, m_hi = -1;
    for (int64_t m = 0; m < M; ++m) {
        int64_t row;
        if (!ens_row<ROWS>(a, row0, m, L, q, row)) continue;
        if ((uint32_t)a.S[row] >= 20u) continue;
        const float x = a.ddg[row * a.ld + b];
        const uint32_t xb = __float_as_uint(x);
        if (ens_is_nan(xb)) continue;
        const uint32_t o = hits_ord(xb);
        if (n == 0 || o < o_lo) {
            o_lo = o;
            x_lo = xb;
            m_lo = (int32_t)m;
        }
        if (n == 0 || o > o_hi) {                                             // (~o < ~o_hi)
            o_hi = o;
            x_hi = xb;
            m_hi = (int32_t)m;
        }
        ++n;
        below += x <= a.cutoff ? 1 : 0;
        s = s + x;
    }
    const int64_t at = (out0 + q) * 20 + b;
    uint32_t mean_bits = ENS_NAN, spread_bits = ENS_NAN;
    if (n > 0) {
        const float fn = (float)n;
        const float mean = (float)((double)s / (double)fn);
        mean_bits = ens_canon(mean);
        // pass 2, ascending m again: d = x - mean, t = t + d * d, three roundings per member
        float t = 0.0f;
        for (int64_t m = 0; m < M; ++m) {
            int64_t row;
            if (!ens_row<ROWS>(a, row0, m, L, q, row)) continue;
            if ((uint32_t)a.S[row] >= 20u) continue;
            const float x = a.ddg[row * a.ld + b];
            if (ens_is_nan(__float_as_uint(x))) continue;
            const float d = x - mean;
            const float dd = d * d;                                           // (its own rounding: contraction is off)
            t = t + dd;
        }
        const float var = (float)((double)t / (double)fn);
        spread_bits = ens_canon((float)sqrt((double)var));
    }
    a.mean[at] = __uint_as_float(mean_bits);
    a.spread[at] = __uint_as_float(spread_bits);
    a.lo[at] = __uint_as_float(x_lo);
    a.hi[at] = __uint_as_float(x_hi);
    a.lo_member[at] = m_lo;
    a.hi_member[at] = m_hi;
    a.count[at] = n;
    a.below[at] = below;
}

// ---- the C-ABI entries ----------------------------------------------------------------------------------------------------------
// one body for both entries: `what` names the entry in its messages, by_rows picks the form
static int ens_launch(const char *what, bool by_rows, const float *ddg, int ld, const int32_t *S, const int32_t *rows, int64_t R,
                      const int32_t *desc, int E, int64_t T, int64_t T_out, int max_len, float cutoff, float *mean, float *spread,
                      float *lo, float *hi, int32_t *lo_member, int32_t *hi_member, int32_t *count, int32_t *below, int32_t *status,
                      tmpnn_stream_t stream) {
    if (E < 0 || T < 0 || T_out < 0 || max_len < 0 || R < 0)
        return tm_set_error(TMPNN_E_INVALID, "%s: bad sizes (E=%d, T=%lld, T_out=%lld, max_len=%d, R=%lld)", what, E, (long long)T,
                            (long long)T_out, max_len, (long long)R);
    if (ld < 20) return tm_set_error(TMPNN_E_INVALID, "%s: ld=%d, a ddG table has at least 20 columns", what, ld);
    if (cutoff != cutoff) return tm_set_error(TMPNN_E_INVALID, "%s: the cutoff is NaN", what);
    if ((T > 0 && (!ddg || !S)) || (E > 0 && (!desc || !status)) || (R > 0 && !rows) ||
        (T_out > 0 && (!mean || !spread || !lo || !hi || !lo_member || !hi_member || !count || !below)))
        return tm_set_error(TMPNN_E_INVALID, "%s: null pointer", what);
    if (T > (int64_t)0x7fffffff || T_out > (int64_t)0x7fffffff)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: T=%lld or T_out=%lld exceeds 2^31 - 1", what, (long long)T, (long long)T_out);
    if (max_len > ENS_MAX_LEN) return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: max_len=%d exceeds %d", what, max_len, ENS_MAX_LEN);
    if (E > ENS_MAX_E) return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: E=%d exceeds %d ensembles per call", what, E, ENS_MAX_E);
    if (E == 0) return TMPNN_OK;
    const EnsArgs a{ddg, ld, S, desc, T, T_out, max_len, cutoff, mean, spread, lo, hi, lo_member, hi_member, count, below, status, rows, R};
    hipStream_t st = (hipStream_t)stream;
    const unsigned gx = max_len > 0 ? (unsigned)((20 * (int64_t)max_len + ENS_THREADS - 1) / ENS_THREADS) : 1u;   // (<= 640; one group
    tm_prof_begin(by_rows ? "ens_stats_rows" : "ens_stats", st);                                                  //  still writes status)
    if (by_rows) hipLaunchKernelGGL(ens_stats_kernel<true>, dim3(gx, (unsigned)E), dim3(ENS_THREADS), 0, st, a);
    else hipLaunchKernelGGL(ens_stats_kernel<false>, dim3(gx, (unsigned)E), dim3(ENS_THREADS), 0, st, a);
    tm_prof_end(st);
    return tm_check_launch("ens_stats_kernel");
}

extern "C" int tmpnn_ensemble_stats(const float *ddg, int ld, const int32_t *S, const int32_t *desc, int E, int64_t T, int64_t T_out,
                                    int max_len, float cutoff, float *mean, float *spread, float *lo, float *hi, int32_t *lo_member,
                                    int32_t *hi_member, int32_t *count, int32_t *below, int32_t *status, tmpnn_stream_t stream) {
    return ens_launch("ensemble_stats", false, ddg, ld, S, nullptr, 0, desc, E, T, T_out, max_len, cutoff, mean, spread, lo, hi, lo_member,
                      hi_member, count, below, status, stream);
}

extern "C" int tmpnn_ensemble_stats_rows(const float *ddg, int ld, const int32_t *S, const int32_t *rows, int64_t R, const int32_t *desc,
                                         int E, int64_t T, int64_t T_out, int max_len, float cutoff, float *mean, float *spread, float *lo,
                                         float *hi, int32_t *lo_member, int32_t *hi_member, int32_t *count, int32_t *below,
                                         int32_t *status, tmpnn_stream_t stream) {
    return ens_launch("ensemble_stats_rows", true, ddg, ld, S, rows, R, desc, E, T, T_out, max_len, cutoff, mean, spread, lo, hi,
                      lo_member, hi_member, count, below, status, stream);
}
