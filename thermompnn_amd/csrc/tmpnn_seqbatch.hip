// The sequence loss over a PACKED batch (gfx950): tmpnn_seqloss_batch_forward / _backward run the training forward and the backward of
// tmpnn_finetune.hip (ft_forward / ft_backward, tmpnn_ft.h) once over the T rows of n_proteins proteins, protein b in the rows
// [offsets[b], offsets[b + 1]). The kernels are row-wise (dense layers per 16-row tile, LayerNorm per row, messages per node, weight
// gradients through fixed row blocks), so a protein enters in four places only, and those are what a segment changes:
//   the k-NN graph     launch_knn with the caller's offsets: neighbours from the protein's own rows, E_idx in global rows;
//   the clamps         ft_graph_kernel clamps a neighbour into its residue's segment (the offsets it reads were made safe below), and
//                      every later gather reads that compacted graph, so its own clamp to [0, T) never acts;
//   the dropout rows   the generator's `row` is the packed row (i for a node site, i K + k for an edge site), the flat keep_in / keep_out
//                      has the one-protein layout of T rows at this K;
//   the carve          the offsets array holds n_proteins + 1 entries and the edge arrays are carved for the call's K, not for 48.
// One K for the whole call, K = min(k_neighbors, min_len). The one-protein entries tmpnn_seqloss_* are the n_proteins = 1 case of the
// same two functions and keep their bits and their sizes.
#include <math.h>
#include <stdint.h>

#include "tmpnn_ft.h"

// The largest packed batch. Every kernel the batch reaches indexes its arrays in 64 bits (size_t row * leading dimension: Ein [E,416],
// dA [E,512], the partials P; int64 element counts in the grid-stride loops; int64 dropout offsets). What stays in int32 is: rows and
// edge rows themselves (E = T K <= 48 T), the dropout generator's `row` (the same), the item counts of ft_dense_kernel
// (ceil(E / 16) * ceil(N / 16) <= 2 E at N = 512) and of ft_wgrad_kernel (<= 33 * 8 * 256), and the CSR's counters (<= E). The widest
// is 2 E = 96 T < 2^31, T < 22.3 M; were any row * leading-dimension product still 32-bit, the widest would be dA: T * 48 * 512 < 2^31,
// T <= 87 381. 65 536 is below both, keeps `saved` (0.8 MB per residue at K = 48) at 52 GB, and is a round number to state.
static const int64_t SB_T_MAX = 65536;

// offsets [n + 1] of the caller against what the call promises, by ONE workgroup: offsets[0] == 0, offsets[n] == T, every segment length in
// [min_len, max_len]; otherwise TMPNN_STATUS_MAXLEN. `safe` [n + 1] is what the kernels of the forward read: the caller's offsets when
// they are at least ascending by >= 1 inside [0, T] (a broken promise alone: wrong numbers, no fault), else the even split
// safe[b] = min(b max_len, T), safe[n] = T, which is ascending and inside [0, T] because the host has checked T <= n max_len.
__global__ __launch_bounds__(TM_THREADS) void sq_segments_kernel(const int32_t *__restrict__ offsets, int n, int T, int min_len, int max_len,
                                                                 int32_t *__restrict__ safe, int32_t *__restrict__ status) {
    __shared__ int s_bad, s_unsafe;
    const int tid = tm_tid();
    if (tid == 0) { s_bad = 0; s_unsafe = 0; }
    __syncthreads();
    int bad = 0, unsafe = 0;
    if (tid == 0 && (offsets[0] != 0 || offsets[n] != T)) bad = unsafe = 1;
    for (int b = tid; b < n; b += TM_THREADS) {
        const int64_t len = (int64_t)offsets[b + 1] - offsets[b];
        if (len < min_len || len > max_len) bad = 1;
        if (len < 1 || offsets[b] < 0 || offsets[b + 1] > T) unsafe = 1;
    }
    if (bad) atomicOr(&s_bad, 1);
    if (unsafe) atomicOr(&s_unsafe, 1);
    __syncthreads();
    const int fall_back = s_unsafe;
    for (int b = tid; b <= n; b += TM_THREADS) {
        const int64_t even = (int64_t)b * max_len;
        safe[b] = !fall_back ? offsets[b] : b == n || even > T ? T : (int)even;
    }
    if (tid == 0 && s_bad && status) atomicOr(status, TMPNN_STATUS_MAXLEN);
}

static bool sb_size_ok(int64_t T, int n_proteins, int K) {
    return T >= 2 && T <= SB_T_MAX && n_proteins >= 1 && 2 * (int64_t)n_proteins <= T && K >= 1 && K <= TM_KS && K <= T;
}

extern "C" size_t tmpnn_seqloss_batch_saved_bytes(int64_t T, int n_proteins, int K) {
    return sb_size_ok(T, n_proteins, K) ? ft_carve2(nullptr, nullptr, true, T, 0, 0, 0, nullptr, true, K, n_proteins).saved_bytes : 0;
}

extern "C" size_t tmpnn_seqloss_batch_scratch_bytes(int64_t T, int n_proteins, int K) {
    return sb_size_ok(T, n_proteins, K) ? ft_carve2(nullptr, nullptr, true, T, 0, 0, 0, nullptr, true, K, n_proteins).scratch_bytes : 0;
}

extern "C" int64_t tmpnn_seqloss_batch_mask_numel(int64_t T, int K) { return sb_size_ok(T, 1, K) ? ft_mask_numel(T, K) : -1; }

// every argument error of both entries, before any launch; *K_out = min(k_neighbors, min_len)
static int sb_check(const char *what, const float *X, const int32_t *S, const float *mask, const int32_t *ridx, const int32_t *cenc,
                    const int32_t *offsets, int n_proteins, int64_t T, int min_len, int max_len, int k_neighbors, const float *params,
                    int64_t slab_numel, float p_mpnn, const void *saved, size_t saved_bytes, int *K_out) {
    FT_REQUIRE(X && S && mask && ridx && cenc && offsets && params, "%s: null pointer", what);   // (ranks may be null: every neighbour visible)
    FT_REQUIRE(n_proteins >= 1, "%s: n_proteins %d < 1", what, n_proteins);
    FT_REQUIRE(min_len >= 2 && min_len <= max_len && max_len <= FT_L_MAX, "%s: segment lengths [%d, %d] outside 2 <= min_len <= max_len <= %lld",
               what, min_len, max_len, (long long)FT_L_MAX);
    FT_REQUIRE(T >= (int64_t)n_proteins * min_len && T <= (int64_t)n_proteins * max_len,
               "%s: T = %lld rows cannot hold %d proteins of %d..%d residues", what, (long long)T, n_proteins, min_len, max_len);
    if (T > SB_T_MAX) return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: T = %lld rows, a packed batch holds at most %lld", what, (long long)T,
                                          (long long)SB_T_MAX);
    FT_REQUIRE(k_neighbors >= 1 && k_neighbors <= TM_KS, "%s: k_neighbors %d outside [1, %d]", what, k_neighbors, TM_KS);
    FT_REQUIRE(min_len >= k_neighbors || min_len == max_len,
               "%s: min_len %d < k_neighbors %d needs proteins of one length (min_len == max_len): one K = min(k_neighbors, min_len) serves "
               "the whole call", what, min_len, k_neighbors);
    FT_REQUIRE(slab_numel == sq_layout().total, "%s: parameter slab holds %lld floats, ProteinMPNN with W_out needs %lld", what,
               (long long)slab_numel, (long long)sq_layout().total);
    FT_REQUIRE(p_mpnn >= 0.f && p_mpnn < 1.f, "%s: dropout probability outside [0, 1)", what);
    *K_out = k_neighbors < min_len ? k_neighbors : min_len;
    return ft_check_buf(what, "saved", (void *)saved, saved_bytes, tmpnn_seqloss_batch_saved_bytes(T, n_proteins, *K_out));
}

static FtCtx sb_ctx(const float *X, const int32_t *S, const float *mask, const int32_t *ridx, const int32_t *cenc, const int32_t *offsets,
                    int n_proteins, int64_t T, int min_len, int max_len, int K, const int32_t *ranks, const float *params, float *grads,
                    void *saved, void *scratch, hipStream_t st) {
    FtCtx c{};
    c.L = (int)T;
    c.K = K;
    c.E = T * K;
    c.nf = 3;
    c.seq = 1;
    c.X = X; c.S = S; c.mask = mask; c.ridx = ridx; c.cenc = cenc; c.ranks = ranks;
    c.params = params;
    c.grads = grads;
    c.lay = sq_layout();
    c.w = ft_carve2(saved, scratch, true, T, 0, 0, 0, nullptr, true, K, n_proteins);
    c.st = st;
    c.n_prot = n_proteins; c.min_len = min_len; c.max_len = max_len;
    c.seg_offsets = offsets;
    return c;
}

extern "C" int tmpnn_seqloss_batch_forward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                                           const int32_t *chain_enc, const int32_t *offsets, int n_proteins, int64_t T, int min_len, int max_len,
                                           int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                                           const float *keep_in, float *keep_out, uint64_t seed, uint64_t step, float *log_probs,
                                           int32_t *E_idx_opt, int32_t *status_opt, void *saved, size_t saved_bytes, tmpnn_stream_t stream) {
    int K = 0;
    FT_TRY(sb_check("seqloss_batch_forward", X, S, mask, residue_idx, chain_enc, offsets, n_proteins, T, min_len, max_len, k_neighbors, params,
                    slab_numel, p_mpnn, saved, saved_bytes, &K));
    FT_REQUIRE(log_probs, "seqloss_batch_forward: null pointer");
    FT_REQUIRE(!(keep_in && keep_out), "seqloss_batch_forward: keep_in (injected masks) and keep_out (drawn masks) exclude each other");
    FtCtx c = sb_ctx(X, S, mask, residue_idx, chain_enc, offsets, n_proteins, T, min_len, max_len, K, ranks, params, nullptr, saved, nullptr,
                     (hipStream_t)stream);
    c.status = status_opt ? status_opt : c.w.status;
    (void)hipMemsetAsync(c.status, 0, 4, c.st);
    sq_segments_kernel<<<1, TM_THREADS, 0, c.st>>>(offsets, n_proteins, (int)T, min_len, max_len, c.w.offs, c.status);
    ft_set_drop(c, T, K, p_mpnn, keep_in, keep_out, seed, step);
    if (keep_out && c.drop.mode != 2) (void)hipMemsetAsync(keep_out, 0, (size_t)ft_mask_numel(T, K) * 4, c.st);   // (drawn masks fill it whole)
    FT_TRY(ft_forward(c));
    (void)hipMemcpyAsync(log_probs, c.w.lp, (size_t)T * TMPNN_VOCAB * 4, hipMemcpyDeviceToDevice, c.st);
    if (E_idx_opt) (void)hipMemcpyAsync(E_idx_opt, c.w.eidx, (size_t)c.E * 4, hipMemcpyDeviceToDevice, c.st);
    return tm_check_launch("seqloss_batch_forward");
}

static int sb_backward_entry(const char *what, bool want_dx, const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                             const int32_t *chain_enc, const int32_t *offsets, int n_proteins, int64_t T, int min_len, int max_len,
                             int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn, const float *keep_in,
                             uint64_t seed, uint64_t step, const float *dlog_probs, float *grads, float *dX, const void *saved,
                             size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream) {
    int K = 0;
    FT_TRY(sb_check(what, X, S, mask, residue_idx, chain_enc, offsets, n_proteins, T, min_len, max_len, k_neighbors, params, slab_numel, p_mpnn,
                    saved, saved_bytes, &K));
    FT_REQUIRE(dlog_probs && grads, "%s: null pointer", what);
    FT_REQUIRE(!want_dx || dX, "%s: dX is null (tmpnn_seqloss_batch_backward is the entry without it)", what);
    FT_TRY(ft_check_buf(what, "scratch", scratch, scratch_bytes, tmpnn_seqloss_batch_scratch_bytes(T, n_proteins, K)));
    // the saved part is only read: its one writer is the forward (the graph in it carries the segments: the offsets are not read again)
    FtCtx c = sb_ctx(X, S, mask, residue_idx, chain_enc, offsets, n_proteins, T, min_len, max_len, K, ranks, params, grads,
                     const_cast<void *>(saved), scratch, (hipStream_t)stream);
    c.dlp = dlog_probs;
    c.dX = dX;
    ft_set_drop(c, T, K, p_mpnn, keep_in, nullptr, seed, step);
    ft_backward(c);
    return tm_check_launch(what);
}

extern "C" int tmpnn_seqloss_batch_backward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                                            const int32_t *chain_enc, const int32_t *offsets, int n_proteins, int64_t T, int min_len, int max_len,
                                            int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                                            const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs, float *grads,
                                            const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream) {
    return sb_backward_entry("seqloss_batch_backward", false, X, S, mask, residue_idx, chain_enc, offsets, n_proteins, T, min_len, max_len,
                             k_neighbors, ranks, params, slab_numel, p_mpnn, keep_in, seed, step, dlog_probs, grads, nullptr, saved,
                             saved_bytes, scratch, scratch_bytes, stream);
}

// the same backward with dL / dX [T,4,3]: a row's neighbours lie in its own segment, so protein b's dX depends on its rows only
extern "C" int tmpnn_seqloss_batch_backward_x(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                                              const int32_t *chain_enc, const int32_t *offsets, int n_proteins, int64_t T, int min_len,
                                              int max_len, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel,
                                              float p_mpnn, const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs,
                                              float *grads, float *dX, const void *saved, size_t saved_bytes, void *scratch,
                                              size_t scratch_bytes, tmpnn_stream_t stream) {
    return sb_backward_entry("seqloss_batch_backward_x", true, X, S, mask, residue_idx, chain_enc, offsets, n_proteins, T, min_len, max_len,
                             k_neighbors, ranks, params, slab_numel, p_mpnn, keep_in, seed, step, dlog_probs, grads, dX, saved, saved_bytes,
                             scratch, scratch_bytes, stream);
}
