// Global alignment of letter-code sequences (gfx950): P pairs (axis a of n codes, member b of m codes) -> for every axis position the
// member position it is aligned to (tmpnn_align_global, include/tmpnn.h). The rule is datasets.global_alignment_map's, the scoring of
// the reference's pairwise2.align.globalxx (datasets.py:229-236): identical columns count 1, gaps are free, so
//     score[i][j] = the LCS length of a[i:], b[j:]     (score[n][.] = score[.][m] = 0, filled from the bottom-right)
// and a trace from (0, 0): diagonal when the letters match and score[i][j] == score[i+1][j+1] + 1, else i += 1 when
// score[i][j] == score[i+1][j], else j += 1. Two codes match iff they are equal and (uint32)code < 20.
// global_alignment_map has a fourth branch, the mismatch column. It cannot fire with this scoring: reaching it needs
// score[i][j] == score[i+1][j+1] while score[i][j] > score[i+1][j], and score[i+1][j] >= score[i+1][j+1] always holds. So every mapped
// pair holds identical letters, and the trace here has three outcomes (2 bits).
//
// ONE LAUNCH, one workgroup of 1024 threads per pair on a persistent grid (a workgroup owns workspace slot blockIdx.x). Per pair:
//   check      every thread checks the descriptor in 64-bit arithmetic before any other access; a bad pair writes status -1 only
//   load       both code strings into LDS as bytes (a code that matches nothing becomes 0xff in a, 0xfe in b), out[.] = -1
//   sweep      anti-diagonals d = n + m - 2 .. 0, cell (i, j = d - i) per thread, three rotating diagonals of 16-bit scores indexed by
//              i, one barrier per diagonal. The 2-bit decision of 16 consecutive cells of a diagonal is folded over 16 lanes (xor
//              shuffles inside the wavefront) and ONE lane stores the whole 32-bit word: every word has one writer, no atomics
//   trace      thread 0 walks at most n + m steps through the decisions and writes the mapped entries of out
// WORKSPACE slot: diagonal-major, every diagonal from a word boundary: diagonal d of a pair starts at word align_diag_word(d, n, m)
// (closed form, below); a slot holds align_slot_words(max_n, max_m) = the words of the largest pair <= ceil(max_n max_m / 16) +
// max_n + max_m. Everything is integer work: results are exact, do not depend on the slot, the grid or the pair's place, and a
// rerun gives the same bits.
#include <stdint.h>

#include "tmpnn_internal.h"

#define ALIGN_THREADS 1024
#define ALIGN_MAX_LEN 8192          // 16-bit scores, and 3 diagonals + 2 strings = 3 * 2 * 8194 + 2 * 8192 = 65 548 bytes of LDS
#define ALIGN_MAX_GRID 1024         // workgroups = workspace slots, at most
#define ALIGN_MAX_WS ((size_t)1 << 30)   // tmpnn_align_workspace_bytes asks for no more slots than fit in this (always one)

struct AlignArgs {
    const int32_t *A, *B;           // [NA], [NB] letter codes
    const int32_t *desc;            // [P, 6] = (a0, n, b0, m, out0, add)
    int64_t NA, NB, NO;
    int P, max_n, max_m;
    int32_t *out;                   // [NO]
    int32_t *aligned, *status;      // [P]
    uint32_t *ws;                   // [grid, slot_words]
    size_t slot_words;
    unsigned lds_diag;              // entries of one diagonal buffer (max_n + 2, even)
};

// F(k) = sum_{t = 1 .. k} ceil(t / 16)
__host__ __device__ __forceinline__ uint32_t align_F(uint32_t k) {
    const uint32_t q = k >> 4, r = k & 15u;
    return 8u * q * (q + 1u) + r * (q + 1u);
}
// the first word of diagonal d (cells i + j == d, 0 <= d <= n + m - 1; n, m >= 1) when every diagonal starts at a word boundary:
// the lengths are 1 .. s (s = min), then s up to d = big - 1 (big = max), then s - 1 .. 1. d = n + m - 1: the words of the pair.
__host__ __device__ __forceinline__ uint32_t align_diag_word(uint32_t d, uint32_t n, uint32_t m) {
    const uint32_t s = n < m ? n : m, big = n < m ? m : n;
    if (d <= s) return align_F(d);
    const uint32_t c = (s + 15u) >> 4;
    if (d <= big) return align_F(s) + (d - s) * c;
    return align_F(s) + (big - s) * c + align_F(s - 1u) - align_F(n + m - 1u - d);
}
static size_t align_slot_words(int max_n, int max_m) {
    return max_n > 0 && max_m > 0 ? (size_t)align_diag_word((uint32_t)(max_n + max_m - 1), (uint32_t)max_n, (uint32_t)max_m) : 0;
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_kernel(AlignArgs g) {
    extern __shared__ __attribute__((aligned(16))) uint16_t align_lds[];
    const int tid = threadIdx.x;
    uint16_t *const diag = align_lds;                                   // [3][lds_diag]
    uint8_t *const la = (uint8_t *)(align_lds + 3 * (size_t)g.lds_diag); // [max_n]
    uint8_t *const lb = la + g.max_n;                                   // [max_m]
    uint32_t *const slot = g.ws + (size_t)blockIdx.x * g.slot_words;

    for (int p = blockIdx.x; p < g.P; p += gridDim.x) {
        const int32_t *dp = g.desc + 6 * (size_t)p;
        const int64_t a0 = dp[0], n64 = dp[1], b0 = dp[2], m64 = dp[3], out0 = dp[4];
        const int32_t add = dp[5];
        const bool ok = a0 >= 0 && n64 >= 0 && b0 >= 0 && m64 >= 0 && out0 >= 0 && n64 <= g.max_n && m64 <= g.max_m &&
                        a0 + n64 <= g.NA && b0 + m64 <= g.NB && out0 + n64 <= g.NO;
        if (!ok) {                                                      // (uniform: every thread read the same descriptor)
            if (tid == 0) g.status[p] = -1;
            continue;
        }
        const int n = (int)n64, m = (int)m64;
        for (int q = tid; q < n; q += ALIGN_THREADS) {
            const uint32_t c = (uint32_t)g.A[a0 + q];
            la[q] = c < 20u ? (uint8_t)c : (uint8_t)0xff;
            g.out[out0 + q] = -1;
        }
        for (int q = tid; q < m; q += ALIGN_THREADS) {
            const uint32_t c = (uint32_t)g.B[b0 + q];
            lb[q] = c < 20u ? (uint8_t)c : (uint8_t)0xfe;
        }
        __syncthreads();
        int count = 0;
        if (n > 0 && m > 0) {
            for (int d = n + m - 2; d >= 0; --d) {
                uint16_t *const cur = diag + (size_t)(d % 3) * g.lds_diag;
                const uint16_t *const p1 = diag + (size_t)((d + 1) % 3) * g.lds_diag;   // diagonal d + 1
                const uint16_t *const p2 = diag + (size_t)((d + 2) % 3) * g.lds_diag;   // diagonal d + 2
                const int i_lo = d - (m - 1) > 0 ? d - (m - 1) : 0;
                const int i_hi = d < n - 1 ? d : n - 1;
                const int len = i_hi - i_lo + 1;
                uint32_t *const words = slot + align_diag_word((uint32_t)d, (uint32_t)n, (uint32_t)m);
                for (int k0 = 0; k0 < len; k0 += ALIGN_THREADS) {       // (uniform trip count: the shuffles below see whole wavefronts)
                    const int k = k0 + tid;
                    uint32_t dec = 0;
                    if (k < len) {
                        const int i = i_lo + k, j = d - i;
                        const bool in_i = i + 1 < n, in_j = j + 1 < m;
                        const uint32_t down = in_i ? p1[i + 1] : 0u;                    // score[i + 1][j]
                        const uint32_t right = in_j ? p1[i] : 0u;                       // score[i][j + 1]
                        const uint32_t dg = in_i && in_j ? p2[i + 1] : 0u;              // score[i + 1][j + 1]
                        const bool match = la[i] == lb[j];
                        uint32_t best = dg + (match ? 1u : 0u);
                        best = down > best ? down : best;
                        best = right > best ? right : best;
                        cur[i] = (uint16_t)best;
                        dec = match && best == dg + 1u ? 0u : best == down ? 1u : 2u;
                    }
                    uint32_t w = dec << (2 * (tid & 15));
                    w |= __shfl_xor(w, 1, 64);
                    w |= __shfl_xor(w, 2, 64);
                    w |= __shfl_xor(w, 4, 64);
                    w |= __shfl_xor(w, 8, 64);
                    if ((tid & 15) == 0 && k < len) words[k >> 4] = w;
                }
                __syncthreads();
            }
            if (tid == 0) {
                int i = 0, j = 0;
                while (i < n && j < m) {
                    const int d = i + j;
                    const int i_lo = d - (m - 1) > 0 ? d - (m - 1) : 0;
                    const int k = i - i_lo;
                    const uint32_t w = slot[align_diag_word((uint32_t)d, (uint32_t)n, (uint32_t)m) + (uint32_t)(k >> 4)];
                    const uint32_t dec = (w >> (2 * (k & 15))) & 3u;
                    if (dec == 0u) {
                        g.out[out0 + i] = add + j;
                        ++count;
                        ++i;
                        ++j;
                    } else if (dec == 1u) {
                        ++i;
                    } else {
                        ++j;
                    }
                }
            }
        }
        if (tid == 0) {
            g.aligned[p] = count;
            g.status[p] = 0;
        }
        __syncthreads();                                                // the strings, the diagonals and the slot are free again
    }
}

// ---- the C-ABI entries -----------------------------------------------------------------------------------------------------------
static size_t align_slot_bytes(int max_n, int max_m) { return tm_align256(align_slot_words(max_n, max_m) * sizeof(uint32_t)); }

extern "C" size_t tmpnn_align_workspace_bytes(int max_n, int max_m, int64_t P) {
    if (max_n < 0 || max_m < 0 || max_n > ALIGN_MAX_LEN || max_m > ALIGN_MAX_LEN || P <= 0) return 0;
    const size_t slot = align_slot_bytes(max_n, max_m);
    if (slot == 0) return 256;
    size_t slots = (size_t)(P < ALIGN_MAX_GRID ? P : ALIGN_MAX_GRID);
    const size_t cap = ALIGN_MAX_WS / slot;
    if (slots > cap) slots = cap > 0 ? cap : 1;
    return slots * slot + 256;
}

extern "C" int tmpnn_align_global(const int32_t *A, int64_t NA, const int32_t *B, int64_t NB, const int32_t *desc, int P, int max_n,
                                  int max_m, int32_t *out, int64_t NO, int32_t *aligned, int32_t *status, void *workspace,
                                  size_t workspace_bytes, tmpnn_stream_t stream) {
    if (P < 0 || NA < 0 || NB < 0 || NO < 0 || max_n < 0 || max_m < 0)
        return tm_set_error(TMPNN_E_INVALID, "align_global: bad sizes (P=%d, NA=%lld, NB=%lld, NO=%lld, max_n=%d, max_m=%d)", P,
                            (long long)NA, (long long)NB, (long long)NO, max_n, max_m);
    if ((NA > 0 && !A) || (NB > 0 && !B) || (NO > 0 && !out) || (P > 0 && (!desc || !aligned || !status)))
        return tm_set_error(TMPNN_E_INVALID, "align_global: null pointer");
    if (max_n > ALIGN_MAX_LEN || max_m > ALIGN_MAX_LEN)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "align_global: max_n=%d or max_m=%d exceeds %d", max_n, max_m, ALIGN_MAX_LEN);
    if (P == 0) return TMPNN_OK;
    const size_t slot = align_slot_bytes(max_n, max_m);
    int grid = P < ALIGN_MAX_GRID ? P : ALIGN_MAX_GRID;
    uint32_t *ws = nullptr;
    if (slot > 0) {
        if (!workspace) return tm_set_error(TMPNN_E_INVALID, "align_global: null pointer (workspace)");
        Carver c(workspace, true);
        ws = c.take<uint32_t>(0);
        const size_t room = workspace_bytes > c.used ? (workspace_bytes - c.used) / slot : 0;
        if (room == 0)
            return tm_set_error(TMPNN_E_WORKSPACE, "align_global: workspace %zu < %zu bytes, one slot", workspace_bytes,
                                tmpnn_align_workspace_bytes(max_n, max_m, 1));
        if ((size_t)grid > room) grid = (int)room;
    }
    const unsigned lds_diag = ((unsigned)max_n + 3u) & ~1u;
    const size_t lds = 3 * (size_t)lds_diag * sizeof(uint16_t) + (size_t)max_n + (size_t)max_m;
    // the attribute is per device; set once per device, not per call
    static bool raised[64] = {false};
    int dev = 0;
    if (lds > 48 * 1024 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && !raised[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  3 * (ALIGN_MAX_LEN + 2) * (int)sizeof(uint16_t) + 2 * ALIGN_MAX_LEN);
        raised[dev] = true;
    }
    const AlignArgs a{A, B, desc, NA, NB, NO, P, max_n, max_m, out, aligned, status, ws, slot / sizeof(uint32_t), lds_diag};
    hipStream_t st = (hipStream_t)stream;
    tm_prof_begin("align_global", st);
    hipLaunchKernelGGL(align_kernel, dim3((unsigned)grid), dim3(ALIGN_THREADS), lds, st, a);
    tm_prof_end(st);
    return tm_check_launch("align_kernel");
}
