// What the translation units of the training path share: tmpnn_finetune.hip (the kernels, ft_forward / ft_backward, the carve, the
// one-protein entries tmpnn_finetune_* / tmpnn_seqloss_*), tmpnn_seqbatch.hip (the packed entries tmpnn_seqloss_batch_*, which run the
// same ft_forward / ft_backward over n_proteins segments of one row space) and tmpnn_coordgrad.hip (the last stage of the _x backwards:
// dRBF -> dX).
#pragma once
#include <stdint.h>

#include "tmpnn_common.h"
#include "tmpnn_internal.h"

#define FT_REQUIRE(cond, ...) do { if (!(cond)) return tm_set_error(TMPNN_E_INVALID, __VA_ARGS__); } while (0)
#define FT_TRY(expr) do { int rc_ = (expr); if (rc_ != TMPNN_OK) return rc_; } while (0)

static const int FT_H = 128;
static const int FT_SITES = 15;
static const int FT_MAX_PARTS = 256;     // row blocks of a weight gradient over [L K] rows
static const int FT_CLS_PARTS = 64;      // row blocks of a class-indexed / column sum
static const int FT_MAX_LAYERS = 8;
static const int64_t FT_L_MAX = 8192;    // the k-NN kernel's LDS bound (tmpnn_graph.hip) holds well past this
static const int64_t FT_M_MAX = 1 << 22;

// ---- dropout --------------------------------------------------------------------------------------------------------------------
struct FtDrop { int mode; const float *keep_in; float *keep_out; uint64_t k2; uint32_t thr; float scale; int64_t off[FT_SITES]; };

// Slab offsets: ProteinMPNN's tensors in state-dict order (weights.mpnn_param_shapes) without W_out.weight / W_out.bias (log_probs is
// not in the loss: no gradient, never touched), then the head slab of tmpnn_head_slab_numel. With num_final_layers = 0 the head reads
// W_s[S] only: W_s is then the one ProteinMPNN tensor in the slab.
struct FtEncP { int64_t n1w, n1b, n2w, n2b, n3w, n3b, W1, b1, W2, b2, W3, b3, W11, b11, W12, b12, W13, b13, Win, bin, Wout, bout; };
struct FtDecP { int64_t n1w, n1b, n2w, n2b, W1, b1, W2, b2, W3, b3, Win, bin, Wout, bout; };
struct FtLayout { int64_t posw, posb, edgew, new_, neb, Wew, Web, Ws; FtEncP enc[3]; FtDecP dec[3]; int64_t head, total, Wo, bo; };

// Workspace, in two parts carved in a fixed order. SAVED: what the backward reads from the forward (the graph, the features, every
// saved activation, W_s[S], the head rows) and the head's workspace of the forward. SCRATCH: what only the backward writes (the CSR
// lists, the gradients of activations, the weight-gradient partials) and the head's workspace of the backward. The fused entries take
// one workspace, saved part first; there the forward's temporaries (ftm, fdh, fdF) are the backward's tm, dh1, dF, and both head
// passes share one head workspace. The split entries (tmpnn_finetune_forward / _backward) give the forward its own temporaries in the
// saved part and the backward its own head workspace in the scratch part, so that the backward never writes the saved part.
struct FtEncS { float *a1, *a2, *b1, *b2, *x3, *mu3, *rs3, *x1, *mu1, *rs1, *hV1, *fa, *x2, *mu2, *rs2, *out; };
struct FtDecS { float *a1, *a2, *x1, *mu1, *rs1, *hV1, *fa, *x2, *mu2, *rs2, *out; };
struct FtWs {
    int32_t *offs, *E48, *eidx, *cls, *cnt, *cur, *coff, *clist, *mcnt, *mcur, *moff, *mlist, *rows_id, *status;
    float *D48, *Ein, *E0, *nemu, *ners, *En, *hE[4], *hV0, *hS, *headX, *dheadX;
    FtEncS enc[3];
    FtDecS dec[3];
    float *tm, *t1, *t2, *dA, *dE, *dE2, *dEd, *gx, *gb, *dEp, *dV, *dV2, *dh1, *dF, *dhS, *dH[3], *dG, *P, *CP;
    float *ftm, *fdh, *fdF;                       // the forward's temporaries: message / LayerNorm input, message sum, FFN output
    float *lp, *dlg, *dVe;                        // the sequence loss: saved log_probs [L,21]; d logits; the encoder output's gradient
    void *head_ws, *head_ws_b;                    // the head's workspace of the forward / of the backward
    size_t head_bytes, saved_bytes, scratch_bytes, bytes;
};

// One call's context: sizes, pointers, the dropout description. L is the number of rows: one protein's length, or the packed batch's T
// (then n_prot segments, offsets from the caller in seg_offsets; the one-protein entries have n_prot = 1 and write [0, L] themselves).
struct FtCtx {
    int L, K, M, nf, lightattn, n_layers, subtract, seq;
    int64_t E;
    const int32_t *dims;
    const float *X, *mask;
    const int32_t *S, *ridx, *cenc, *pos, *mut, *wt;
    const float *dlp;                             // the sequence loss: upstream dL / dlog_probs [L,21] (backward)
    const int32_t *ranks;                         // the sequence loss: decoding ranks [L] (null: every neighbour visible, the ddG path)
    const float *params;
    float *grads;
    float *dX;                                    // the _x backwards: dL / dX [L,4,3] (null: ft_backward stops at W_edge / W_pos)
    FtLayout lay;
    FtWs w;
    FtDrop drop;
    hipStream_t st;
    int n_prot, min_len, max_len;                 // segments of the row space and the bounds the caller promises for their lengths
    const int32_t *seg_offsets;                   // the packed entries: the caller's offsets [n_prot + 1] (device), which the entry has
                                                  // checked and copied into w.offs; null: one protein, ft_forward writes [0, L] there
    int32_t *status;                              // the packed entries: the caller's status word (null: the carve's own, never read)
};

// ---- the featurizer's geometry, shared by the forward (ft_graph_kernel) and the coordinates' backward (tmpnn_coordgrad.hip) -------------
static __constant__ int c_ft_pa[25] = {1, 0, 2, 3, 4, 1, 1, 1, 1, 0, 0, 0, 4, 4, 3, 0, 2, 3, 4, 2, 3, 4, 2, 3, 2};   // PAIR_ORDER (:1143-1167)
static __constant__ int c_ft_pb[25] = {1, 0, 2, 3, 4, 0, 2, 3, 4, 2, 3, 4, 2, 3, 2, 1, 1, 1, 1, 0, 0, 0, 4, 4, 3};

__device__ __forceinline__ void ft_atom(const float *x, int a, float *o) {   // N, Ca, C, O, virtual Cb (:1131-1138)
    if (a < 4) { o[0] = x[3 * a]; o[1] = x[3 * a + 1]; o[2] = x[3 * a + 2]; return; }
    float b[3], cc[3];
    for (int k = 0; k < 3; ++k) { b[k] = x[3 + k] - x[k]; cc[k] = x[6 + k] - x[3 + k]; }
    const float ax = b[1] * cc[2] - b[2] * cc[1], ay = b[2] * cc[0] - b[0] * cc[2], az = b[0] * cc[1] - b[1] * cc[0];
    const float av[3] = {ax, ay, az};
    for (int k = 0; k < 3; ++k) o[k] = -0.58273431f * av[k] + 0.56802827f * b[k] - 0.54067466f * cc[k] + x[3 + k];
}

// tmpnn_coordgrad.hip: dRBF [E,400] (= dE0 W_edge[:, 16:416]) -> c.dX [L,4,3], through c.w.tm (30 floats per edge)
void ft_coord_grad(const FtCtx &c, const float *dRBF);

// tmpnn_finetune.hip
FtLayout sq_layout();
// seq: the sequence loss's buffers (no mutants, no head; log_probs and two gradients more). Kc: the neighbour count the edge arrays are
// carved for (0: min(48, L), what every one-protein entry takes); n_prot: the offsets array holds n_prot + 1 entries.
FtWs ft_carve2(void *saved, void *scratch, bool split, int64_t L, int64_t M, int lightattn, int n_layers, const int32_t *dims,
               bool seq = false, int64_t Kc = 0, int64_t n_prot = 1);
int64_t ft_mask_numel(int64_t L, int64_t K);
void ft_set_drop(FtCtx &c, int64_t L, int64_t K, float p_mpnn, const float *keep_in, float *keep_out, uint64_t seed, uint64_t step);
int ft_check_buf(const char *what, const char *which, void *buf, size_t bytes, size_t need);
int ft_forward(const FtCtx &c);
void ft_backward(const FtCtx &c);
