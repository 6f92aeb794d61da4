/*
 * tmpnn.h — C-ABI of the MI355X-native ThermoMPNN inference engine (libtmpnn.so).
 *
 * Drop-in boundary for the ONE hot path of Kuhlman-Lab/ThermoMPNN:
 *   tied_featurize tensors -> kNN graph -> edge featurizer -> 3x EncLayer -> 3x DecLayer -> ddG head.
 * Each entry point names the reference interface it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - extern "C"; every function returns int (0 = TMPNN_OK, negative = error) unless noted;
 *     no exception crosses the boundary; tmpnn_last_error() returns a thread-local message.
 *   - All data pointers are BORROWED DEVICE pointers (e.g. torch tensor.data_ptr()); the caller owns
 *     every buffer including outputs and workspace. The library never allocates device memory and
 *     never synchronises the stream. `stream` is a hipStream_t passed as void*.
 *   - Ragged batch layout: proteins are packed along one residue axis of length T = sum(L_p);
 *     `offsets[N+1]` (int32, device) gives each protein's [start, end). A padded [B, L] batch of the
 *     reference API is the special case offsets = {0, L, 2L, ...} with mask = 0 on padding.
 *   - All floating-point data is fp32 (the reference computes in fp32 throughout); indices handed
 *     across this boundary are int32 except where an entry point mirrors a reference signature that
 *     takes int64 (gather_nodes / gather_edges).
 *   - Neighbour slots: every residue owns TMPNN_KS = 48 edge slots; slot k >= min(K, L_p) is
 *     invalid (E_idx = -1, h_E row = 0). K must be <= 48 (ThermoMPNN uses the v_48_* weights).
 */
#ifndef TMPNN_H
#define TMPNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMPNN_VERSION 200
#define TMPNN_HID 128          /* hidden width (transfer_model.py:19) */
#define TMPNN_KS 48            /* neighbour slots per residue */
#define TMPNN_VOCAB 21
#define TMPNN_N_MPNN_TENSORS 118
#define TMPNN_N_TENSORS 130    /* + 12 TransferModel head tensors */

enum {
    TMPNN_OK = 0,
    TMPNN_E_INVALID = -1,      /* bad argument (null pointer, negative size, K out of range ...) */
    TMPNN_E_UNSUPPORTED = -2,  /* valid request outside what this build supports */
    TMPNN_E_LAUNCH = -3,       /* HIP launch/runtime error (message has hipGetErrorString) */
    TMPNN_E_WORKSPACE = -4,    /* workspace / packed buffer too small */
    TMPNN_E_RANGE = -5         /* a result left the finite range (tmpnn_status_error); retry with precision "bf16x3" */
};

/* Device-side status word (int32, caller-owned device memory, optional): kernels OR these bits in; the library never
 * reads it back (no stream sync). The host copies it after synchronising and passes it to tmpnn_status_error(). */
enum {
    TMPNN_STATUS_RANGE = 1,    /* a ddG / log-probability is inf or NaN: an activation or weight overflowed the fp16 range of
                                  the "f16x2" matrix-core path (|x| >= 65504) */
    TMPNN_STATUS_MAXLEN = 2,   /* a protein is longer than the max_len the caller passed: its neighbour rows were left
                                  empty (E_idx = -1) instead of overrunning the kernel's per-row scratch */
    TMPNN_STATUS_SELFTEST = 4  /* tmpnn_selftest: the library was built with flags that break its overflow detection or its
                                  persistent tile loops (-> TMPNN_E_UNSUPPORTED) */
};

typedef struct tmpnn_weights tmpnn_weights_t;   /* opaque; immutable after create */
typedef void *tmpnn_stream_t;                   /* hipStream_t */

int tmpnn_version(void);
const char *tmpnn_last_error(void);
/* Maps a status word (host copy) to an error: 0 -> TMPNN_OK; TMPNN_STATUS_MAXLEN -> TMPNN_E_INVALID;
 * TMPNN_STATUS_RANGE -> TMPNN_E_RANGE (message in tmpnn_last_error()). */
int tmpnn_status_error(int32_t status);
/* Device self-test of the build (one tiny launch on `stream`, no sync): the f16x2 kernels' GELU must propagate NaN (that is how
 * an fp16 overflow reaches TMPNN_STATUS_RANGE) and the kernels' view of gridDim / blockDim must match the launch. ORs
 * TMPNN_STATUS_SELFTEST into the caller-owned device word `status` on failure; hosts run it once per device before trusting a
 * freshly built library (thermompnn_amd/engine.py does, at the first weight handle). */
int tmpnn_selftest(int32_t *status, tmpnn_stream_t stream);
/* "f16x2" (default), "bf16x3" or "fp32": how the per-edge GEMMs (featurizer, message and edge-update kernels) run on
 * the matrix cores. f16x2 = every fp32 operand kept as two fp16 values x = h + l*2^-11 (22 significant bits), three
 * partial products per term on v_mfma_f32_16x16x32_f16 with fp32 accumulation; bf16x3 = exact three-way bf16 split, six
 * partial products on v_mfma_f32_16x16x32_bf16 (full fp32 range); fp32 = v_mfma_f32_16x16x4_f32. All three are in the
 * same accuracy class (see thermompnn_amd/csrc/tmpnn_split.h) and pass the same parity tests.
 * The precision is a property of the WEIGHT HANDLE (tmpnn_weights_create_p); this call returns the default that
 * handles created without an explicit precision get (environment variable TMPNN_PRECISION, else "f16x2"). */
const char *tmpnn_matmul_mode(void);

/* ---- weights ------------------------------------------------------------------------------------
 * Canonical tensor order = the reference state dict: the 118 ProteinMPNN tensors in module
 * registration order (protein_mpnn_utils.py:1184-1215), then light_attention.{feature,attention}
 * _convolution.{weight,bias}, both_out.{1,3,5}.{weight,bias}, ddg_out.{weight,bias}
 * (transfer_model.py:57-73,131-134). tmpnn_tensor_name(i) spells out entry i so a host can check. */
int tmpnn_num_tensors(void);
const char *tmpnn_tensor_name(int index);       /* NULL if out of range */
int64_t tmpnn_tensor_numel(int index);          /* -1 if out of range */

/* Device bytes the library needs for derived data: positional table, per-decoder-layer sequence tables, centre tap of the
 * feature convolution (0.8 MB) and — for "f16x2" handles only — the f16 fragment images of the weight blocks (7.2 MB).
 * tmpnn_weights_packed_bytes() is the upper bound over the precisions; _p gives the size for one precision (NULL = the
 * default; 0 for an unknown name). */
size_t tmpnn_weights_packed_bytes(void);
size_t tmpnn_weights_packed_bytes_p(const char *precision);

/* Replaces: get_protein_mpnn()'s load_state_dict (transfer_model.py:17-37) and the Lightning
 * checkpoint load (analysis/thermompnn_benchmarking.py:78-84) — the host reads the file, this call
 * takes the tensors. `tensors[i]` = device pointer to tensor i (fp32, contiguous). n_tensors is 118
 * (ProteinMPNN only: head calls then fail with TMPNN_E_INVALID) or 130. The raw tensors must stay
 * alive and unmodified for the handle's lifetime. Derived tables are written into `packed` on
 * `stream`. */
int tmpnn_weights_create(tmpnn_weights_t **out, const float *const *tensors, int n_tensors,
                         void *packed, size_t packed_bytes, tmpnn_stream_t stream);
/* Same, with the matrix-core precision of every call made through this handle: "f16x2" | "bf16x3" | "fp32", or NULL
 * for the default. Unknown names return TMPNN_E_INVALID. Several handles (e.g. one per precision) may share the raw
 * tensors; each needs its own `packed` buffer. */
int tmpnn_weights_create_p(tmpnn_weights_t **out, const float *const *tensors, int n_tensors,
                           void *packed, size_t packed_bytes, const char *precision, tmpnn_stream_t stream);
const char *tmpnn_weights_precision(const tmpnn_weights_t *w);
void tmpnn_weights_destroy(tmpnn_weights_t *w);

/* ---- the C-alpha-only flavour (ProteinMPNN(ca_only=True), ca_model_weights/v_48_*) ----------------------------------------------
 * Replaces CA_ProteinFeatures (protein_mpnn_utils.py:911-1081) behind the constructor switch of :1195-1197. Only the featurizer
 * differs between the flavours: the k-NN graph is the same function of the C-alpha atoms, the encoder, the decoder, W_s and W_out
 * have the same shapes. A CA handle takes the 118 ProteinMPNN tensors in the canonical order with entry 2
 * (features.edge_embedding.weight) of shape 128 x 167 — tmpnn_tensor_numel_ca(i), -1 outside [0, 118). The reference's CA model
 * registers five more parameters (features.node_embedding.weight, features.norm_nodes.{weight,bias}, W_v.{weight,bias}) that its
 * forward never reads: the host drops them. ThermoMPNN has no CA flavour: n_tensors other than 118 is TMPNN_E_INVALID, and so is a
 * ddg output of tmpnn_ssm_forward with a CA handle. `packed` needs tmpnn_weights_ca_packed_bytes_p(precision) bytes (0 = unknown name).
 *
 * X stays [T,4,3] with only slot 1 (C-alpha) read, so tmpnn_knn_topk, the PDB packer and every X argument are as for the full
 * backbone. SEGMENTS: the reference shifts and differences C-alpha along the padded length axis, with zero coordinates in front of
 * row 0 and behind the last row and zero frames on rows 0, L-2 and L-1. Here a segment is one protein [offsets[p], offsets[p+1]) of
 * the packed axis: a padded [B, L] batch laid out as B segments of L rows (padding rows at coordinate 0, as tied_featurize leaves
 * them) reproduces the reference's padded result, a ragged batch reproduces each protein run alone. A segment of fewer than 3 rows
 * (the reference fails there) has zero frames; nothing outside a row's segment is read.
 *
 * tmpnn_encode and tmpnn_ssm_forward read the handle's flavour. With a CA handle they launch: the k-NN kernel, ca_frames, the CA
 * edge kernel (at every launch size: the small-launch form that computes the k-NN rows inside the featurizer is full-backbone
 * only), then the encoder and decoder launches of a full-backbone handle. The frames live in the existing workspace; the sizers
 * return what they return for a full-backbone handle. A protein's result does not depend on the batch it is packed into.
 * Everything that reads an encoded ctx (tmpnn_decode_variants, tmpnn_decode_ordered, tmpnn_sample*) works on a CA ctx as it is.
 * PARITY is judged edge by edge against the reference evaluated in float64 (tests/test_gpu_ca.py). The quaternion's sign() and
 * sqrt(|.|) make an edge ill-conditioned in fp32 for any implementation — the self edge, pairs of parallel frames — when, in float64,
 * one of the three radicands, the three sign differences or 1 + tr R is neither 0 nor at least 1e-3 in magnitude. Well-conditioned
 * edges are within 1e-5; the others within 2.5 x the reference-fp32's own distance from float64. The operands of sign(), of the
 * 3.6 / 4.0 window and of relu() are computed in the association of the torch expressions, without fma contraction, by one set of
 * device functions shared by the pre-pass and the edge kernels of every precision.
 * tmpnn_edge_featurize cannot serve a CA handle (it has no offsets): TMPNN_E_INVALID; use the two entries below.
 * The training entries (tmpnn_finetune_*, tmpnn_seqloss_*, the head trainers) take no handle and are full-backbone only. */
size_t tmpnn_weights_ca_packed_bytes_p(const char *precision);
int tmpnn_weights_create_ca(tmpnn_weights_t **out, const float *const *tensors, int n_tensors /* 118 */, void *packed,
                            size_t packed_bytes, const char *precision, tmpnn_stream_t stream);
int tmpnn_weights_is_ca(const tmpnn_weights_t *w);       /* 1 for a handle of tmpnn_weights_create_ca, else 0 */
int64_t tmpnn_tensor_numel_ca(int index);
/* _orientations_coarse's frames (protein_mpnn_utils.py:960-989): O [T,9] = rows (o, n, o x n) with U = normalize(dX), dX[t] =
 * Ca[t+1] - Ca[t] zeroed unless 3.6 < |dX| < 4.0, o = normalize(U[t-1] - U[t]), n = normalize(U[t-1] x U[t]) on rows 1 .. n-3 of a
 * segment of n rows; 0 on its rows 0, n-2, n-1. */
int tmpnn_ca_frames(const float *X, const int32_t *offsets, int n_proteins, int64_t T, float *O /* [T,9] */,
                    tmpnn_stream_t stream);
/* CA_ProteinFeatures.forward after top-k (protein_mpnn_utils.py:1046-1079: 9 RBF blocks, dU and Q of :998-1002, PositionalEncodings,
 * edge_embedding, norm_edges) fused with W_e (:1229); arguments as tmpnn_edge_featurize plus the segments and O from tmpnn_ca_frames
 * on the same X / offsets. */
int tmpnn_edge_featurize_ca(const tmpnn_weights_t *w, const float *X, const int32_t *residue_idx, const int32_t *chain_enc,
                            const int32_t *offsets, int n_proteins, const int32_t *E_idx, const float *D_nb, const float *O,
                            int64_t T, float *h_E, float *E_opt, tmpnn_stream_t stream);

/* ---- graph construction ------------------------------------------------------------------------
 * Replaces ProteinFeatures._dist + torch.topk (protein_mpnn_utils.py:1101-1109).
 * X [T,4,3] (N,CA,C,O; NaN already zeroed as tied_featurize does, :577), mask [T].
 * E_idx [T,48] receives GLOBAL packed row indices sorted by ascending adjusted distance (ties: lower
 * index first), -1 in invalid slots; D_nb [T,48] the adjusted distances (0 in invalid slots).
 * max_len >= max_p L_p sizes the per-row LDS scratch (1 <= max_len <= 8192). The lengths live in device memory, so the
 * host cannot check them: a protein longer than max_len gets empty rows and TMPNN_STATUS_MAXLEN in *status_opt. */
int tmpnn_knn_topk(const float *X, const float *mask, const int32_t *offsets, int n_proteins,
                   int64_t T, int max_len, int K, int32_t *E_idx, float *D_nb, int32_t *status_opt,
                   tmpnn_stream_t stream);

/* compute_centrality (analysis/thermompnn_benchmarking.py:20-35): out[t] = #{other residues of the same protein
 * with |CA_t - CA_j| < radius}; residues without coordinates (mask 0) get -1 and are never counted. int32 [T]. */
int tmpnn_centrality(const float *X, const float *mask, const int32_t *offsets, int n_proteins, int64_t T,
                     float radius, int32_t *out, tmpnn_stream_t stream);

/* Replaces ProteinFeatures.forward after top-k (protein_mpnn_utils.py:1140-1180: 25 RBF blocks,
 * PositionalEncodings :896-908, edge_embedding, norm_edges) fused with W_e (:1229).
 * residue_idx, chain_enc: int32 [T]. h_E [T,48,128] <- W_e . LN(W_edge . [posenc | RBF]) + b.
 * E_opt (may be NULL) receives the LayerNorm output E [T,48,128] (what ProteinFeatures returns). */
int tmpnn_edge_featurize(const tmpnn_weights_t *w, const float *X, const int32_t *residue_idx,
                         const int32_t *chain_enc, const int32_t *E_idx, const float *D_nb, int64_t T,
                         float *h_E, float *E_opt, tmpnn_stream_t stream);

/* ---- gathers (the "gather HBM GB/s" kernel of BASELINE.json:metric) ------------------------------
 * gather_nodes(nodes[B,N,C], neighbor_idx[B,N,K] int64) -> [B,N,K,C]  (protein_mpnn_utils.py:770-778) */
int tmpnn_gather_nodes(const float *nodes, const int64_t *neighbor_idx, int B, int N, int K, int C,
                       float *out, tmpnn_stream_t stream);
/* Same gather on the engine's own layout: out[r,:] = nodes[idx[r],:], idx int32 global rows
 * (rows with idx < 0 are written as zeros). This is the roofline microbenchmark kernel. */
int tmpnn_gather_rows_i32(const float *nodes, const int32_t *idx, int64_t n_rows, int C, float *out,
                          tmpnn_stream_t stream);
/* gather_edges(edges[B,N,N,C], neighbor_idx[B,N,K] int64) -> [B,N,K,C]  (protein_mpnn_utils.py:763-767) */
int tmpnn_gather_edges(const float *edges, const int64_t *neighbor_idx, int B, int N, int K, int C,
                       float *out, tmpnn_stream_t stream);

/* ---- message-passing layers ---------------------------------------------------------------------
 * Workspace for one layer call / for the fused forward. */
size_t tmpnn_layer_workspace_bytes(int64_t T);
size_t tmpnn_workspace_bytes(int64_t T);

/* EncLayer.forward (protein_mpnn_utils.py:816-839) with mask_attend = mask_i*mask_j (:1232-1233).
 * h_V [T,128] and h_E [T,48,128] are updated in place. */
int tmpnn_enc_layer(const tmpnn_weights_t *w, int layer, float *h_V, float *h_E, const int32_t *E_idx,
                    const float *mask, int64_t T, void *workspace, size_t workspace_bytes,
                    tmpnn_stream_t stream);

/* One decoder step of ProteinMPNN.forward (protein_mpnn_utils.py:1268-1273 + DecLayer.forward
 * :859-880): h_ESV = mask_i * [h_E | W_s[S_j] | h_V_j], no neighbour mask. h_V_out may alias h_V_in. */
int tmpnn_dec_layer(const tmpnn_weights_t *w, int layer, const float *h_V_in, float *h_V_out,
                    const float *h_E, const int32_t *E_idx, const int32_t *S, const float *mask,
                    int64_t T, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);

/* h_S = W_s[S] (protein_mpnn_utils.py:1238). */
int tmpnn_seq_embed(const tmpnn_weights_t *w, const int32_t *S, int64_t T, float *h_S,
                    tmpnn_stream_t stream);
/* log_softmax(W_out h_V + b) (protein_mpnn_utils.py:1275-1276) -> [T,21]. */
int tmpnn_log_probs(const tmpnn_weights_t *w, const float *h_V, int64_t T, float *log_probs,
                    int32_t *status_opt, tmpnn_stream_t stream);

/* ---- ddG head ------------------------------------------------------------------------------------
 * TransferModel.forward's per-mutation body (transfer_model.py:86-120) evaluated once per POSITION:
 * x = [hV_last | hV_prev | W_s[S]], y = centre tap of LightAttention's feature conv (:148-155 on a
 * length-1 sequence), z = both_out(y) (:67-71). ddg [T,21]: ddg[t,a] = (w z_a + b) - (w z_S[t] + b)
 * (:110-116); z_opt (may be NULL) receives z [T,21]. */
int tmpnn_ddg_head(const tmpnn_weights_t *w, const float *hV_last, const float *hV_prev,
                   const int32_t *S, int64_t T, float *ddg, float *z_opt, int32_t *status_opt,
                   tmpnn_stream_t stream);

/* The same head for ANY configuration the reference constructor accepts (transfer_model.py:45-73): num_final_layers
 * n_final in 0..3 (hidden[0] = last decoder state, hidden[1] the one before, ... as all_mpnn_hid[:n] :84-85), LightAttention
 * on (conv_w [D0, D0, 9] + conv_b [D0], D0 = 128 n_final + 128; only the centre tap acts on a length-1 sequence) or off
 * (conv_w = conv_b = NULL, :106-108), any hidden_dims: dims[0] = D0, dims[1..n_layers-1] = hidden_dims, dims[n_layers] = 21;
 * mlp_w[l] [dims[l+1], dims[l]], mlp_b[l] = both_out's Linear l (ReLU in FRONT of each, :69-71). hidden, mlp_w, mlp_b, dims are
 * HOST arrays (of device pointers / ints); everything they point to, S and the outputs are device memory. ddg [T,21] as
 * tmpnn_ddg_head; z_opt [T,21]. The released configuration runs the specialised kernels behind tmpnn_ddg_head /
 * tmpnn_ssm_forward; this entry keeps retrained heads runnable (fp32 matrix cores, operands from global memory). */
size_t tmpnn_head_generic_workspace_bytes(int64_t T, int n_final, int n_layers, const int32_t *dims);   /* 0 = bad dims */
int tmpnn_ddg_head_generic(const float *const *hidden, int n_final, const float *Ws, const int32_t *S, int64_t T,
                           const float *conv_w, const float *conv_b, int n_layers, const float *const *mlp_w,
                           const float *const *mlp_b, const int32_t *dims, const float *ddg_w, const float *ddg_b, float *ddg,
                           float *z_opt, void *workspace, size_t workspace_bytes, int32_t *status_opt, tmpnn_stream_t stream);

/* ---- training of the ddG head with ProteinMPNN frozen (train_thermompnn.py:48-113; thermompnn_amd/train.py drives it) ----
 * Parameters, gradients and the AdamW moments each live in ONE flat fp32 slab holding the head's trainable tensors in state-dict
 * order: [light_attention.feature_convolution.weight [D0,D0,9], .bias, attention_convolution.weight, .bias] (lightattn only),
 * both_out Linear l weight [dims[l+1], dims[l]] + bias for l < n_layers, ddg_out.weight, ddg_out.bias. dims as
 * tmpnn_ddg_head_generic (HOST array). tmpnn_head_slab_numel -> its length (-1 = bad dims). */
int64_t tmpnn_head_slab_numel(int n_final, int lightattn, int n_layers, const int32_t *dims);
size_t tmpnn_head_train_workspace_bytes(int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims);   /* 0 = bad */
/* One training step's forward + backward over M labelled mutants of one protein: mutant i reads feature row rows[i] of feat
 * [n_feat, D0] (the [h_dec(last) | ... | W_s[S]] rows of head_concat; indices are clamped to [0, n_feat)), mutant / wild-type
 * amino-acid indices mut[i], wt[i] (< 21) and target[i]. Dropout on the centre-tap output (LightAttention only): keep_in [M, D0]
 * (0 / 1, an injected mask) or, with keep_in NULL and p_drop > 0, the in-kernel counter-based generator keyed on (seed, step,
 * mutant row, column) — keep_out [M, D0] (may be NULL) receives its mask. Writes loss[0] = mean (pred - target)^2, pred_opt [M],
 * and every gradient entry that can be non-zero into grads (the 8 non-centre taps and the attention convolution are never
 * written: zero the slab once). Deterministic: no floating-point atomics. All of feat..target, params, grads, keep_*, loss, pred
 * are device memory. */
int tmpnn_head_train_step(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt,
                          const float *target, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims,
                          int subtract_mut, const float *params, float *grads, int64_t slab_numel, float p_drop,
                          const float *keep_in, float *keep_out, uint64_t seed, uint64_t step, float *loss, float *pred_opt,
                          void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);
/* Eval-mode predictions (no dropout) pred [M] for the same mutant description. */
int tmpnn_head_eval(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt, int64_t M,
                    int n_final, int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params,
                    int64_t slab_numel, float *pred, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);
/* torch.optim.AdamW (decoupled decay, torch/optim/adam.py's order) over the slab: segment s = [seg_begin[s], seg_begin[s+1])
 * with learning rate seg_lr[s] and kind seg_kind[s]: 1 = full update, 2 = only the centre taps (offset % 9 == 4) of a
 * convolution weight have a gradient, 0 = structurally zero gradient (decay only; m, v stay 0 and are not read). step counts
 * from 1. seg_begin [n_seg + 1], seg_kind, seg_lr are HOST arrays; n_seg <= 32. */
int tmpnn_adamw_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t numel, int n_seg,
                     const int64_t *seg_begin, const int32_t *seg_kind, const double *seg_lr, double beta1, double beta2,
                     double eps, double weight_decay, int64_t step, tmpnn_stream_t stream);


/* ---- fine-tuning of ProteinMPNN together with the head (freeze_weights: false, train_thermompnn.py:88-113; thermompnn_amd/finetune.py)
 * ONE flat fp32 slab: ProteinMPNN's tensors in state-dict order without W_out.weight / W_out.bias (not in the loss: never touched),
 * then the head slab of tmpnn_head_slab_numel. With num_final_layers 0 the head reads W_s[S] only, and W_s is the one ProteinMPNN
 * tensor in the slab. tmpnn_finetune_slab_numel -> its length (-1 = bad dims). */
int64_t tmpnn_finetune_slab_numel(int n_final, int lightattn, int n_layers, const int32_t *dims);
/* Length of the flat dropout-mask buffer of one protein of length L (keep_in / keep_out below; -1 = bad L): the 15 sites of
 * csrc/tmpnn_finetune.hip in site order, [L, 128] per node site and [L K, 128] per edge site, K = min(48, L). */
int64_t tmpnn_finetune_mask_numel(int64_t L);
size_t tmpnn_finetune_workspace_bytes(int64_t L, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims);  /* 0 = bad */
/* One training step of one protein (L residues: X [L,4,3], S, mask, residue_idx, chain_enc as tied_featurize gives them) over M
 * labelled mutants at residues pos[i] (mut / wt / target as tmpnn_head_train_step): the training forward (ProteinMPNN in train mode,
 * dropout p_mpnn at its 15 sites; the head's centre-tap dropout p_head), loss[0] = mean (pred - target)^2, pred_opt [M], and every
 * gradient of the slab into grads. ProteinMPNN's dropout: keep_in (0 / 1, injected) or the counter-based generator keyed on
 * (seed, step, site, row, col), whose masks keep_out receives (may be NULL); the head's: head_keep_in [M, D0] or its own generator
 * (tmpnn_head_train_step's, same seed / step). E_idx_opt [L, K] receives the k-NN graph and rows_opt [M, D0] the head rows
 * [h_dec(last) | ... | W_s[S]]. Deterministic: no floating-point atomics, bit-identical reruns. All data pointers are device memory. */
int tmpnn_finetune_step(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                        int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, const float *target, int64_t M,
                        int n_final, int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params,
                        float *grads, int64_t slab_numel, float p_mpnn, float p_head, const float *keep_in, float *keep_out,
                        const float *head_keep_in, uint64_t seed, uint64_t step, float *loss, float *pred_opt, int32_t *E_idx_opt,
                        float *rows_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);
/* Eval-mode predictions (no dropout anywhere) pred [M] with the slab's weights; E_idx_opt / rows_opt as above. */
int tmpnn_finetune_eval(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                        int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn,
                        int n_layers, const int32_t *dims, int subtract_mut, const float *params, int64_t slab_numel, float *pred,
                        int32_t *E_idx_opt, float *rows_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);

/* tmpnn_finetune_step split in two calls, for a host autograd (thermompnn_amd/autograd.py): the forward fills a SAVED buffer that the
 * backward only reads, so the saved state stays alive between them (and a second backward over it gives the same bits), while the
 * backward's SCRATCH buffer may be shared by every backward. Sizes as tmpnn_finetune_workspace_bytes (0 = bad arguments); the saved
 * part holds the graph, the features, every activation the backward reads and the head rows. */
size_t tmpnn_finetune_saved_bytes(int64_t L, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims);
size_t tmpnn_finetune_scratch_bytes(int64_t L, int64_t M, int n_final, int lightattn, int n_layers, const int32_t *dims);
/* The training forward of tmpnn_finetune_step (same description, same dropout: keep_in / the generator keyed on (seed, step) at p_mpnn,
 * head_keep_in / the head's generator at p_head): pred [M] equals tmpnn_finetune_step's pred_opt bit for bit. keep_out, E_idx_opt and
 * rows_opt as there. */
int tmpnn_finetune_forward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                           int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn,
                           int n_layers, const int32_t *dims, int subtract_mut, const float *params, int64_t slab_numel, float p_mpnn,
                           float p_head, const float *keep_in, float *keep_out, const float *head_keep_in, uint64_t seed, uint64_t step,
                           float *pred, int32_t *E_idx_opt, float *rows_opt, void *saved, size_t saved_bytes, tmpnn_stream_t stream);
/* The backward of the forward that filled `saved` (same arguments, same params, saved untouched since), seeded from any upstream
 * gradient dpred [M] = dL / dpred (device). The dropout masks are recomputed (or keep_in / head_keep_in read again). Writes the
 * gradient entries of the slab that can be non-zero into grads, as tmpnn_finetune_step does (the caller zeroes the slab); with
 * mpnn_grads = 0 only the head's part of the slab is written and the ProteinMPNN backward does not run (frozen encoder).
 * Contract: with dpred[i] = 2 * (pred[i] - t[i]) * (1.0f / M) formed in fp32, forward then backward give the same pred and grads as
 * tmpnn_finetune_step, bit for bit. Deterministic; `saved` is never written. */
int tmpnn_finetune_backward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                            int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn,
                            int n_layers, const int32_t *dims, int subtract_mut, const float *params, int64_t slab_numel, float p_mpnn,
                            float p_head, const float *keep_in, const float *head_keep_in, uint64_t seed, uint64_t step,
                            const float *dpred, float *grads, int mpnn_grads, const void *saved, size_t saved_bytes, void *scratch,
                            size_t scratch_bytes, tmpnn_stream_t stream);

/* ---- ProteinMPNN's own training objective: log p(sequence | structure) under a decoding order, and its gradient -----------------
 * The training forward of tmpnn_finetune_forward (exact fp32, dropout at the same 15 sites with the same generator, keep_in / keep_out
 * layout and tmpnn_finetune_mask_numel) with the ORDER-MASKED decoder of the reference's training flavour and the output layer:
 * ranks [L] int32, edge (i, k) with j = E_idx[i, k] is visible iff ranks[j] < ranks[i] (equal ranks are not: the self edge never is;
 * all ranks equal = no sequence information; ranks NULL = every neighbour visible, the self edge too: the order mask of ones under
 * which tmpnn_ssm_forward computes its log_probs), and the decoder message input of every layer l for that edge is
 *     mask_i * [ h_V^l_i | h_E_ik | vis * h_S_j | (vis ? h_V^l_j : h_V^enc_j) ],
 * h_V^enc the last encoder output. log_probs [L,21] = log_softmax(W_out h_V^dec3 + b); rows with mask 0 are finite (h_V is 0 there).
 * K = min(k_neighbors, L) neighbours, k_neighbors in [1, 48]; E_idx_opt [L, K]. With K < min(48, L) an edge dropout site uses the
 * first L K rows of its [L min(48, L), 128] part of keep_in / keep_out. The slab holds ProteinMPNN's tensors in state-dict order,
 * W_out.weight and W_out.bias included, and no head: tmpnn_seqloss_slab_numel floats. The backward takes ANY upstream gradient
 * dlog_probs [L,21] (rows with mask 0 included: a loss multiplies by its own mask): dlogits = dlp - softmax * sum(dlp), W_out's
 * gradients, then the decoder, W_s, encoder and featurizer backward of tmpnn_finetune_backward, where d h_S_j is collected over the
 * visible edges only and d h_V_j of an invisible edge goes to the encoder output (summed over decoder layers 2, 1, 0 in that order,
 * added before the encoder loop). As tmpnn_finetune_backward it writes the entries of grads that can be non-zero (the caller zeroes the
 * slab). Deterministic, no float atomics;
 * `saved` is written by the forward only, so a second backward over it gives the same bits. L in [2, 8192]; the sizers return 0
 * outside it. Error codes before any launch as tmpnn_finetune_*. */
int64_t tmpnn_seqloss_slab_numel(void);
size_t tmpnn_seqloss_saved_bytes(int64_t L);
size_t tmpnn_seqloss_scratch_bytes(int64_t L);
int tmpnn_seqloss_forward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                          int64_t L, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                          const float *keep_in, float *keep_out, uint64_t seed, uint64_t step, float *log_probs, int32_t *E_idx_opt,
                          void *saved, size_t saved_bytes, tmpnn_stream_t stream);
int tmpnn_seqloss_backward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                           int64_t L, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                           const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs, float *grads,
                           const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream);

/* ---- the same objective over a packed batch: one forward, one backward for n_proteins proteins ---------------------------------
 * X [T,4,3], S, mask, residue_idx, chain_enc, ranks [T] packed as tmpnn_encode takes them; protein b owns the rows
 * [offsets[b], offsets[b+1]) (offsets: device int32 [n_proteins + 1], offsets[0] = 0, offsets[n_proteins] = T). The caller promises
 * every segment length in [min_len, max_len], 2 <= min_len <= max_len <= 8192, so n_proteins min_len <= T <= n_proteins max_len.
 * Neighbours come from the protein's own rows (the k-NN kernel of tmpnn_knn_topk with these offsets: a protein's graph does not depend
 * on the batch it is packed into); E_idx_opt [T, K] holds global rows. ranks are compared inside a protein only (a neighbour is always
 * in the same segment). ONE K serves the call: K = min(k_neighbors, min_len). A call with min_len < k_neighbors is accepted only when
 * min_len == max_len (the padded [B, L] pack, B segments of L rows); otherwise TMPNN_E_INVALID, the message names both numbers.
 * log_probs [T,21]: the rows of protein b are bit for bit what tmpnn_seqloss_forward gives for that protein alone at this K without
 * dropout. grads receives the gradient of the whole batch, the sum over proteins, written as tmpnn_seqloss_backward writes it (the
 * entries that can be non-zero, into a slab the caller has zeroed); the fixed row blocks of a weight gradient run over the packed
 * rows, so it equals the sum of the proteins' own gradients to rounding, not bit for bit, except at n_proteins = 1, which is
 * tmpnn_seqloss_* exactly. Deterministic as the one-protein entries: no float atomics, bit-identical reruns, a second backward over
 * the same `saved` gives the same bits.
 * Dropout: the same generator and the same 15 sites; `row` is the PACKED row (i for a node site, i K + k for an edge site), and the flat
 * keep_in / keep_out buffer has the one-protein layout of a "protein" of T rows at this K: tmpnn_seqloss_batch_mask_numel(T, K) =
 * (12 T + 3 T K) 128 floats, the sites in order, each [rows, 128] with no tail (the one-protein entries lay an edge site out for
 * min(48, L) whatever K). With n_proteins = 1 the numbering coincides with the one-protein entry's. A protein's masks therefore DEPEND
 * ON WHERE IT SITS in the batch: the same (seed, step) gives a protein other masks at another offset.
 * status_opt (device int32, may be NULL) is zeroed on the stream and receives TMPNN_STATUS_MAXLEN when a segment's length lies outside
 * [min_len, max_len], offsets[0] != 0 or offsets[n_proteins] != T (one workgroup checks this at the head of the forward). The kernels
 * keep their clamps: a caller whose offsets break the promise gets wrong numbers and the status bit, never an access outside the
 * buffers. T <= 65536 (tmpnn_seqbatch.hip derives it): the sizers return 0 above it, for T < 2, n_proteins < 1 or > T / 2, K outside
 * [1, 48] or K > T (mask_numel: -1), and the entries return TMPNN_E_UNSUPPORTED above it. `saved` holds about 0.8 MB per residue at
 * K = 48. Error codes before any launch as tmpnn_seqloss_*. */
size_t tmpnn_seqloss_batch_saved_bytes(int64_t T, int n_proteins, int K);
size_t tmpnn_seqloss_batch_scratch_bytes(int64_t T, int n_proteins, int K);
int64_t tmpnn_seqloss_batch_mask_numel(int64_t T, int K);
int tmpnn_seqloss_batch_forward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                const int32_t *offsets, int n_proteins, int64_t T, int min_len, int max_len, int k_neighbors,
                                const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn, const float *keep_in,
                                float *keep_out, uint64_t seed, uint64_t step, float *log_probs, int32_t *E_idx_opt, int32_t *status_opt,
                                void *saved, size_t saved_bytes, tmpnn_stream_t stream);
int tmpnn_seqloss_batch_backward(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                                 const int32_t *offsets, int n_proteins, int64_t T, int min_len, int max_len, int k_neighbors,
                                 const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn, const float *keep_in,
                                 uint64_t seed, uint64_t step, const float *dlog_probs, float *grads, const void *saved,
                                 size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream);

/* ---- gradients with respect to the backbone coordinates ------------------------------------------------------------------------
 * The three split backwards with one output more: dX = dL / dX, [L,4,3] ([T,4,3] packed), fp32, directly after grads. Each entry takes
 * its parent's arguments, buffers, sizes and error order, writes grads exactly as its parent does, bit for bit, and writes ALL of dX
 * (the caller does not zero it). dX == NULL is TMPNN_E_INVALID: the parent is the entry for that case. tmpnn_finetune_backward_x needs
 * the ProteinMPNN backward: mpnn_grads = 0 is TMPNN_E_INVALID; with num_final_layers = 0 the head never reads the structure and dX is
 * all zeros. `saved` is never written: a second _x backward over it gives the same bits. No float atomics, fixed summation orders,
 * bit-identical reruns. In the packed entry a row's neighbours lie in its own segment, so dX of protein b is a function of that
 * protein's rows only. No workspace grows: the stage lives in scratch buffers that are dead after the encoder loop.
 * What is differentiated: the featurizer (model_utils.py:314-381 = protein_mpnn_utils.py:1101-1168 of the reference): the virtual Cb
 * from N, Ca, C (cross product included), the 25 atom-pair distances sqrt(|A - B|^2 + 1e-6) of every edge, their 16 RBFs, then
 * edge_embedding; one stage at the tail of the backward, after d edge_embedding is formed:
 *     dRBF [E,400] = dE0 W_edge[:, 16:416];   dD_p = sum_r dRBF[e, 16 p + r] RBF[e, 16 p + r] (-1.28 (D_p - mu_r));
 *     edge (i, k), j = E_idx[i, k], pair p = (a, b): + dD_p (A - B) / D_p to atom a of row i, - the same to atom b of row j;
 *     per residue: its own K edges in slot order, then the incoming edges in ascending edge order, then the Cb chain rule.
 * Contract: the graph E_idx is a constant (no gradient through the choice of neighbours), and D_max of _dist (model_utils.py:318-319)
 * is a constant. Pair 0 (Ca-Ca, the masked distance of _dist) therefore contributes (Ca_i - Ca_j) / D where mask_i mask_j = 1 and
 * nothing elsewhere. (The reference's autograd leaks a gradient from every masked neighbour slot of a row into that row's farthest
 * valid residue through D + (1 - mask_2D) D_max: a by-product of how masked entries are pushed behind the sort, undefined at distance
 * ties, and absent whenever a protein has more than K valid residues: there the two definitions coincide exactly.) Everything else is
 * the chain rule as written: a masked residue that IS selected as a neighbour gets the gradient of its (zero) coordinates through the
 * 24 unmasked pairs, as in the reference. Rows whose coordinates reach the loss through no edge get exactly 0. */
int tmpnn_finetune_backward_x(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                              int64_t L, const int32_t *pos, const int32_t *mut, const int32_t *wt, int64_t M, int n_final, int lightattn,
                              int n_layers, const int32_t *dims, int subtract_mut, const float *params, int64_t slab_numel, float p_mpnn,
                              float p_head, const float *keep_in, const float *head_keep_in, uint64_t seed, uint64_t step,
                              const float *dpred, float *grads, float *dX, int mpnn_grads, const void *saved, size_t saved_bytes,
                              void *scratch, size_t scratch_bytes, tmpnn_stream_t stream);
int tmpnn_seqloss_backward_x(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                             int64_t L, int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                             const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs, float *grads, float *dX,
                             const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream);
int tmpnn_seqloss_batch_backward_x(const float *X, const int32_t *S, const float *mask, const int32_t *residue_idx,
                                   const int32_t *chain_enc, const int32_t *offsets, int n_proteins, int64_t T, int min_len, int max_len,
                                   int k_neighbors, const int32_t *ranks, const float *params, int64_t slab_numel, float p_mpnn,
                                   const float *keep_in, uint64_t seed, uint64_t step, const float *dlog_probs, float *grads, float *dX,
                                   const void *saved, size_t saved_bytes, void *scratch, size_t scratch_bytes, tmpnn_stream_t stream);

/* ---- the fused path ------------------------------------------------------------------------------
 * Everything TransferModel.forward does on the device for a ragged batch of N proteins
 * (transfer_model.py:75-121 + protein_mpnn_utils.py:1222-1277), one call, 18 launches on `stream` (14 when every workgroup has at most one residue tile).
 * Outputs (each may be NULL; ddg needs a handle with the head tensors): ddg [T,21]; hidden_opt [3,T,128] = decoder states 1..3
 * (the reference returns them reversed, :1277); log_probs_opt [T,21]; E_idx_opt [T,48] global rows.
 * status_opt (device int32, may be NULL) is zeroed on the stream and then receives TMPNN_STATUS_* bits. */
int tmpnn_ssm_forward(const tmpnn_weights_t *w, const float *X, const int32_t *S, const float *mask,
                      const int32_t *residue_idx, const int32_t *chain_enc, const int32_t *offsets,
                      int n_proteins, int64_t T, int max_len, int K, float *ddg, float *hidden_opt,
                      float *log_probs_opt, int32_t *E_idx_opt, int32_t *status_opt, void *workspace,
                      size_t workspace_bytes, tmpnn_stream_t stream);

/* ---- many sequence variants over one backbone --------------------------------------------------------
 * The k-NN graph, the edge features and the three encoder layers never read the sequence (it enters at decoder layer 0,
 * protein_mpnn_utils.py:1268). tmpnn_encode runs that part of tmpnn_ssm_forward once for a ragged batch — the same launches,
 * small-launch forms included, so the encoder state has the fused forward's bits — and leaves in the caller's ctx buffer
 * (tmpnn_encode_bytes(T) bytes, 256-byte aligned, opaque) what the decoder reads: E_idx [T,48], the final h_E [T,48,128], the
 * encoder's h_V [T,128] and decoder layer 0's node projection without its sequence term [T,256]. status_opt is zeroed on the
 * stream and receives TMPNN_STATUS_MAXLEN / TMPNN_STATUS_RANGE (a non-finite encoder state). The ctx belongs to the handle's
 * precision: decode it with a handle of the same precision. */
size_t tmpnn_encode_bytes(int64_t T);
size_t tmpnn_encode_workspace_bytes(int64_t T);
int tmpnn_encode(const tmpnn_weights_t *w, const float *X, const float *mask, const int32_t *residue_idx,
                 const int32_t *chain_enc, const int32_t *offsets, int n_proteins, int64_t T, int max_len, int K,
                 void *ctx, size_t ctx_bytes, int32_t *status_opt, void *workspace, size_t workspace_bytes,
                 tmpnn_stream_t stream);
/* The three decoder layers, the ddG head and the log-probabilities for V full sequences over the encoded batch: S_var [V,T]
 * (variant v = one sequence over the packed residue axis), mask [T] as given to tmpnn_encode. Outputs (each may be NULL, not all):
 * ddg [V,T,21] with ddg[v,t,a] relative to the variant's OWN residue S_var[v,t], as tmpnn_ssm_forward defines it for S;
 * hidden_opt [V,3,T,128]; log_probs_opt [V,T,21]. The decoder message pass fetches a residue's h_E tile and multiplies it by
 * W1's edge block once per chunk of variants, not once per variant. A variant's result has the same bits whatever V is and
 * whichever slot it takes (callers may chunk V freely); with an fp32 handle it is tmpnn_ssm_forward's result for that sequence bit
 * for bit, with the split precisions it is held to the same tolerances but sums in another order. V * T is bounded by the
 * kernels' 32-bit row arithmetic: TMPNN_E_UNSUPPORTED beyond it (decode in chunks), and tmpnn_decode_variants_workspace_bytes
 * returns 0. status_opt is zeroed on the stream and receives TMPNN_STATUS_RANGE. */
size_t tmpnn_decode_variants_workspace_bytes(int64_t T, int64_t V);
int tmpnn_decode_variants(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const int32_t *S_var, int64_t V,
                          const float *mask, int64_t T, float *ddg, float *hidden_opt, float *log_probs_opt,
                          int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);
/* The same decode under a decoding order per variant: the reference's masked decoder (protein_mpnn_utils.py:1247-1272 without the
 * overwrite of :1259) as ProteinMPNN.conditional_probs / unconditional_probs run it (:1496-1587). rank [V,T]: residue i of variant
 * v sees neighbour j's identity and decoder state when rank[v][j] < rank[v][i]; of every other neighbour it sees the encoder
 * state alone (mask_bw / mask_fw of the reference; h_E is always present, everything times mask[i]). rank is the inverse
 * permutation of the reference's decoding_order; ranks are only compared between a residue and its listed neighbours, any int32
 * is legal, equal ranks mean "not visible" (all ranks equal: unconditional_probs). Arguments, outputs, error codes, the no-op on
 * T == 0 or V == 0 and status_opt as tmpnn_decode_variants; additionally (V + 1) * T < 2^24 (32-bit offsets into the projection
 * table of V variants + the encoder state): TMPNN_E_UNSUPPORTED beyond it, and tmpnn_decode_ordered_workspace_bytes returns 0.
 * A variant's result has the same bits whatever V is and whichever slot it takes. */
size_t tmpnn_decode_ordered_workspace_bytes(int64_t T, int64_t V);
int tmpnn_decode_ordered(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const int32_t *S_var,
                         const int32_t *rank, int64_t V, const float *mask, int64_t T, float *ddg_opt,
                         float *hidden_opt, float *log_probs_opt, int32_t *status_opt,
                         void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);

/* ---- autoregressive sampling over one encoded backbone ---------------------------------------------------
 * ProteinMPNN.sample's loop (protein_mpnn_utils.py:1279-1383) for N CHAINS over the encoded batch, in ONE launch: a chain is one
 * sequence being sampled over the packed residue axis, with its own decoding order, fixed positions and uniform draws. A workgroup
 * owns up to 16 chains and runs their T steps inside the kernel; no workgroup reads what another writes. Step s of chain n decodes
 * residue t = order[n,s] with tmpnn_decode_ordered's arithmetic for a variant whose ranks are the inverse of `order` (the residues of
 * earlier steps are visible with the letters the chain chose), then
 *     probs = softmax(logits * inv_temperature + bias[t]);  with allowed: probs = probs * allowed[t] / sum(probs * allowed[t]);
 *     c_a = fp32 running sum of probs in index order; the pick is the smallest a with c_a > u[n,t] * c_20, or, if rounding leaves
 *     none, the largest a with probs_a > 0.
 * S_out[n,t] is the pick where free[n,t] * mask[t] == 1 and S_fixed[n,t] elsewhere; probs_opt[n,t,:] is probs there and exactly 0
 * elsewhere. A chain's result has the same bits whatever N is, whichever slot it takes and whichever chains run with it. The message
 * GEMMs run at the handle's precision (f16x2 | bf16x3); the 16-row node update, projections and logits are exact fp32 matrix-core
 * arithmetic for both. An fp32 handle is refused with TMPNN_E_UNSUPPORTED (use "bf16x3"). 3 * N * T < 2^24 (32-bit row arithmetic):
 * TMPNN_E_UNSUPPORTED beyond it (sample in chunks of chains) and tmpnn_sample_workspace_bytes returns 0. An order entry outside
 * [0, T) skips that step; letters are clamped to [0, 21) before any table lookup; non-finite logits OR TMPNN_STATUS_RANGE into
 * status_opt (zeroed on the stream first) and that step takes S_fixed. T == 0 or N == 0 is a no-op. */
size_t tmpnn_sample_workspace_bytes(int64_t T, int64_t N);          /* 0 = unsupported sizes */
int tmpnn_sample(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T, int64_t N,
                 const int32_t *order,      /* [N,T] a permutation of 0..T-1 per chain: order[n,s] is decoded at step s */
                 const int32_t *S_fixed,    /* [N,T] letters kept where free == 0 or mask == 0 */
                 const float *free,         /* [N,T] 1 = sample here (the reference's chain_mask * chain_M_pos) */
                 const float *u,            /* [N,T] uniforms in [0,1), indexed by RESIDUE, not by step */
                 float inv_temperature, const float *bias_opt /* [T,21] */, const float *allowed_opt /* [T,21] */,
                 int32_t *S_out /* [N,T] */, float *probs_opt /* [N,T,21] */,
                 int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);
/* ProteinMPNN.tied_sample's loop (protein_mpnn_utils.py:1385-1494) and the PSSM terms of both reference samplers (:1354-1367,
 * :1472-1481), again N chains in ONE launch; every argument tmpnn_sample has means what it means there. A chain's schedule is
 * order[n,:] (a permutation) and close[n,:] (0 / 1): a GROUP is a maximal run of steps ending at a step with close == 1,
 * close[n,T-1] must be 1, and close all ones is untied sampling. A group's members are decoded one after the other and share ONE
 * draw. Walking the members in step order (t the residue, s the step):
 *   - dead group (:1444-1450): the first member with mask[t] == 0 ends the group, t_dead = t. The members before it stay decoded,
 *     the members after it are never decoded, the group's letter is S_fixed[n,t_dead] and the probs rows of ALL members are exactly 0;
 *   - a live member is decoded as tmpnn_sample decodes it; neighbour j is visible iff its step is below s. A visible neighbour from
 *     an earlier group gives its decoder-state rows plus the sequence term of its group's letter; an earlier member of the SAME group
 *     gives its rows WITHOUT a sequence term (the reference has written h_V_stack[l+1][j], h_S[j] is still zero, :1454-1461); a
 *     member that was never decoded gives zero state at layers 1 and 2 and the encoder row at layer 0, with its letter's sequence term;
 *   - acc[0..20] += weight[n,t] * logits_t (:1464; weight = tied_beta[t] / len(group) is the caller's, NULL = 1, may be negative);
 *   - at the closing member t1 of a live group, in this order (:1468-1488; every per-residue table is read at t1 — the reference's
 *     loop variable as the member loop leaves it):
 *         probs = softmax(acc * inv_temperature + bias[t1]);
 *         pssm_mix:  probs = (1 - mix[t1]) * probs + mix[t1] * pssm_bias[t1];
 *         pssm_keep: pm = probs * keep[t1] + 0.001 * probs;  probs = pm / sum(pm);
 *         allowed:   pm = probs * allowed[t1];  probs = pm / sum(pm);
 *     tmpnn_sample's draw rule on u[n,t1]; the letter is the pick where free[n,t1] == 1, S_fixed[n,t1] elsewhere; probs is
 *     written to EVERY member's row, also where not free (:1492 has no chain_mask factor, unlike :1376);
 *   - every member receives the letter in S_out (:1489-1491), and its table rows gain the letter's sequence term.
 * With close all ones and no weight / PSSM tables this is tmpnn_sample, except that unmasked fixed positions get their probs row.
 * Non-finite logits or totals OR TMPNN_STATUS_RANGE and the group takes S_fixed[n,t1]. Sizes, bounds (3 * N * T < 2^24), the fp32
 * refusal ("bf16x3"), the no-op on T == 0 or N == 0 and chain independence as tmpnn_sample; pssm_bias_opt is required iff
 * pssm_mix_opt is given (TMPNN_E_INVALID otherwise). */
size_t tmpnn_sample_tied_workspace_bytes(int64_t T, int64_t N);     /* 0 = unsupported sizes */
int tmpnn_sample_tied(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T, int64_t N,
                      const int32_t *order, const int32_t *close /* [N,T] 1 = the step is the last member of its group */,
                      const int32_t *S_fixed, const float *free, const float *u /* [N,T] by residue; read at closing members */,
                      float inv_temperature, const float *weight_opt /* [N,T] by residue */, const float *bias_opt /* [T,21] */,
                      const float *allowed_opt /* [T,21] */, const float *pssm_mix_opt /* [T] pssm_multi * pssm_coef */,
                      const float *pssm_bias_opt /* [T,21] */, const float *pssm_keep_opt /* [T,21] pssm_log_odds_mask */,
                      int32_t *S_out /* [N,T] */, float *probs_opt /* [N,T,21] */,
                      int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);
/* The two samplers for EVERY PROTEIN of a packed batch over its own steps, in ONE launch: many backbones, a few chains each. The ctx
 * is tmpnn_encode's for P proteins (offsets [P+1], on the device) and every [N,T] / [T,21] / [T] array keeps its meaning and its
 * full-batch shape; chain n's schedule for protein b is order[n, t0:t1] with t0 = offsets[b], t1 = offsets[b+1] — a permutation of
 * the packed indices t0 .. t1-1 — and the kernel's work item is (protein b, block of 16 chains), which runs the steps s in [t0, t1)
 * only: the grid is (p1 - p0) * ceil(N / 16) workgroups for the protein range [p0, p1). A neighbour is visible iff its step is below
 * s (packed s); all arithmetic of a step is tmpnn_sample's, so a (protein, chain) pair has the bits tmpnn_sample gives for that
 * protein encoded alone with the segment's order shifted to local indices, whatever P, N, the range, the slot and sched_opt are.
 * sched_opt [p1 - p0] (device) is the launch order as protein indices (longest first keeps the tail short), NULL = index order; an
 * entry outside [p0, p1) makes its workgroups do nothing. The scratch is sized by the RANGE: row0 = offsets[p0] and
 * rows = offsets[p1] - offsets[p0] as host integers (0 <= row0, row0 + rows <= T); the bound 3 * N * rows < 2^24 holds per launch
 * (TMPNN_E_UNSUPPORTED beyond it, the workspace size is then 0). A step whose residue lies outside its protein or outside
 * [row0, row0 + rows) is skipped, so a wrong pair cannot overrun the workspace. S_out / probs_opt are written for the rows of
 * [p0, p1) only. Tied form: groups live inside one protein; close[n, t1-1] must be 1 for every protein (the caller checks it; the
 * kernel treats a segment's last step as closing regardless). Errors, the fp32 refusal ("bf16x3"), status_opt and the no-op on
 * N == 0, rows == 0 or p0 == p1 as tmpnn_sample; additionally TMPNN_E_INVALID for p0 > p1, p1 > P or a negative size. */
size_t tmpnn_sample_each_workspace_bytes(int64_t rows, int64_t N);        /* 0 = unsupported sizes */
int tmpnn_sample_each(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T,
                      const int32_t *offsets /* device [P+1] */, int64_t P, int64_t p0, int64_t p1, int64_t row0, int64_t rows,
                      const int32_t *sched_opt /* device [p1-p0] */, int64_t N, const int32_t *order, const int32_t *S_fixed,
                      const float *free, const float *u, float inv_temperature, const float *bias_opt, const float *allowed_opt,
                      int32_t *S_out, float *probs_opt, int32_t *status_opt, void *workspace, size_t workspace_bytes,
                      tmpnn_stream_t stream);
size_t tmpnn_sample_tied_each_workspace_bytes(int64_t rows, int64_t N);   /* 0 = unsupported sizes */
int tmpnn_sample_tied_each(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T,
                           const int32_t *offsets /* device [P+1] */, int64_t P, int64_t p0, int64_t p1, int64_t row0, int64_t rows,
                           const int32_t *sched_opt /* device [p1-p0] */, int64_t N, const int32_t *order, const int32_t *close,
                           const int32_t *S_fixed, const float *free, const float *u, float inv_temperature, const float *weight_opt,
                           const float *bias_opt, const float *allowed_opt, const float *pssm_mix_opt, const float *pssm_bias_opt,
                           const float *pssm_keep_opt, int32_t *S_out, float *probs_opt, int32_t *status_opt, void *workspace,
                           size_t workspace_bytes, tmpnn_stream_t stream);

/* ---- ranked hit lists: the k most stabilising substitutions of every protein, selected on the device -----------------------------
 * What retrieve_best_mutants + a sort of the frame would give (analysis/SSM.py:32-42,153-166), without moving a [T,21] table to the
 * host. ddg [T, ld] (ld >= 20; the table of tmpnn_ssm_forward has ld = 21), S [T] (the residue's own letter; >= 20 or negative = no
 * residue or 'X'), offsets [n_proteins + 1]. A CANDIDATE of protein b is (local position p, letter a < 20) at row t = offsets[b] + p with
 * S[t] < 20, a != S[t], ddg[t, a] not NaN, a != cysteine (letter 1) unless TMPNN_HITS_INCLUDE_CYS, and ddg[t, a] <= cutoff (+inf
 * removes no candidate; a NaN cutoff is TMPNN_E_INVALID). With TMPNN_HITS_ONE_PER_POSITION every position first keeps only its best
 * candidate (the first minimum, as idxmin). The hits of b are its first min(k, #candidates) candidates in ascending (value, position,
 * letter) order; values compare as fp32 numbers with -0.0 taken as +0.0, +-inf are ordinary values. Every key is distinct: the result
 * is unique, and a protein's hits do not depend on the batch, on n_proteins or on the launch shape. No float arithmetic, no atomics:
 * reruns give identical bits.
 * Outputs: hit_ddg [n_proteins, k] = the table's own bits (a -0.0 stays -0.0), padded with NaN; hit_pos [n_proteins, k] the local
 * position, hit_aa [n_proteins, k] the letter, both padded with -1; hit_count [n_proteins]. 1 <= k <= 256 (TMPNN_E_INVALID outside);
 * every protein <= 8192 residues, the forward's own bound. The lengths live in device memory, so the host cannot check them: a longer
 * protein gets hit_count = -1 and padding only, never an access outside the buffers (offsets are clamped into [0, T]).
 * Two launches on `stream`: (protein, block of 256 residues) sorts its candidates' 64-bit keys in LDS and leaves its first k in the
 * workspace; one workgroup per protein sorts the <= 32 blocks' leaders and decodes the first k. tmpnn_hits_workspace_bytes: the
 * workspace, ((T >> 8) + n_proteins) * k keys of 8 bytes; 0 for sizes that are not served (T < 0 or > 2^31 - 1, n_proteins < 1, k
 * outside [1, 256]). n_proteins == 0 is a no-op. Errors before any launch: null pointer, k, ld < 20, negative sizes, unknown flag
 * bits, NaN cutoff -> TMPNN_E_INVALID; T > 2^31 - 1 -> TMPNN_E_UNSUPPORTED; a short workspace -> TMPNN_E_WORKSPACE. */
enum { TMPNN_HITS_INCLUDE_CYS = 1, TMPNN_HITS_ONE_PER_POSITION = 2 };
size_t tmpnn_hits_workspace_bytes(int64_t T, int n_proteins, int k);
int tmpnn_select_hits(const float *ddg, int ld, const int32_t *S, const int32_t *offsets, int n_proteins, int64_t T, int k,
                      float cutoff, int flags, float *hit_ddg, int32_t *hit_pos, int32_t *hit_aa, int32_t *hit_count,
                      void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);

/* ---- streaming hit lists over variant tables: the k smallest of base[v] + ddg[v, q, b], carried from call to call ----------------
 * For selections whose table is too large to exist, such as all double mutants of a protein ([P, 20, L, 20]): decode a chunk of
 * variants (tmpnn_decode_variants), reduce it to k keys while it is hot, pass the k keys on to the next chunk. One call takes V
 * variants of ONE protein of L rows: ddg [V, L, ld] (ld >= 20; relative to the variant's own residue), S_var [V, L], and per variant,
 * on the device, base [V] (fp32), tag [V] and skip [V] (int32; skip -1 = none). A CANDIDATE is (v, q, b) with 0 <= tag[v] <= 65535,
 * S_var[v, q] < 20 (unsigned compare: negative = no residue), b < 20, b != S_var[v, q], q != skip[v] (q > skip[v] with
 * TMPNN_VHITS_UPPER), b != cysteine (letter 1) unless TMPNN_VHITS_INCLUDE_CYS, and a value that is not NaN and <= cutoff (+inf
 * removes no candidate). The VALUE is base[v] + ddg[v, q, b]: one IEEE fp32 round-to-nearest add, the only float operation
 * (+inf + -inf is NaN: no candidate; a variant whose tag is out of range or whose base is NaN contributes nothing). Its 64-bit KEY
 * is the order-preserving image of the sum's bits (-0.0 taken as +0.0; tmpnn_select_hits's) in the high word and
 * tag << 16 | q << 5 | b in the low word, so L <= 2048; ascending keys are ascending (value, tag, position, letter), and all ones
 * means "none". For double mutants tag = p * 32 + a: 11 + 5 + 11 + 5 bits.
 * STATE: `state` [k], 64-bit keys, owned by the caller, on the device. Without TMPNN_VHITS_CONTINUE the call selects from its own
 * variants; with it the k keys in `state` (left by earlier calls with the same k, padded with all ones) take part. After the call
 * `state` holds the k smallest keys of everything seen, ascending. The caller promises distinct tags over all calls of one
 * selection: every key is then distinct, the result is unique and does not depend on how the variants were cut into calls, on the
 * order of the calls, on V or on the launch shape. No atomics: reruns give identical bits.
 * Outputs, decoded from the state by every call: hit_ddg [k] = the sum's bits recovered from the key (a -0.0 sum is reported as
 * +0.0), padded with NaN; hit_tag, hit_pos, hit_aa [k] padded with -1; hit_count [1].
 * Two launches on `stream`: min(items, 8192 / m - 1) workgroups (m = the power of two >= k, an item = a variant's block of 256
 * residues) each keep their m leaders in LDS over the items they loop over and leave k of them in the workspace; one workgroup
 * merges these with the state and decodes. V == 0 or L == 0 launches the merge only (the input pointers may then be NULL): with
 * CONTINUE the state is kept and decoded, without it the state becomes empty, the outputs padding and hit_count 0.
 * tmpnn_variant_hits_workspace_bytes: min(items, 8192 / m - 1) * k keys of 8 bytes; 0 for sizes that are not served. Errors before
 * any launch: null pointer, k outside [1, 256], ld < 20, negative sizes, unknown flag bits, NaN cutoff -> TMPNN_E_INVALID; L > 2048
 * or V * L > 2^31 - 1 -> TMPNN_E_UNSUPPORTED; a short workspace -> TMPNN_E_WORKSPACE. */
enum { TMPNN_VHITS_INCLUDE_CYS = 1, TMPNN_VHITS_UPPER = 2, TMPNN_VHITS_CONTINUE = 4 };
size_t tmpnn_variant_hits_workspace_bytes(int64_t V, int64_t L, int k);   /* 0 for sizes not served */
int tmpnn_select_variant_hits(const float *ddg, int ld, const int32_t *S_var, const float *base, const int32_t *tag,
                              const int32_t *skip, int64_t V, int64_t L, int k, float cutoff, int flags,
                              uint64_t *state, float *hit_ddg, int32_t *hit_tag, int32_t *hit_pos, int32_t *hit_aa,
                              int32_t *hit_count, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);

/* ---- per-site-pair maps over variant tables: every (row, position)'s best value and epistasis, carried from call to call ---------
 * The other reduction of a table that is too large to exist ([P, 20, L, 20] for the double mutants of a protein): not the k best of
 * all, but for every pair (state row, position q) its best value, the extremes of its epistasis, and the mean size of it. One call
 * takes V variants of ONE protein of L rows, all on the device: ddg [V, L, ld] (ld >= 20), S_var [V, L], per variant base [V] (fp32),
 * row [V], letter [V] and skip [V] (int32; skip -1 = none), the wild-type table wt [L, ld_wt] (ld_wt >= 20), and R, the number of
 * state rows. A CANDIDATE is (v, q, b) with 0 <= row[v] < R and 0 <= letter[v] < 20 (a variant outside either range contributes
 * nothing), S_var[v, q] < 20 (unsigned compare: negative = no residue), b < 20, b != S_var[v, q], q != skip[v] (q > skip[v] with
 * TMPNN_PMAP_UPPER), and b != cysteine (letter 1) unless TMPNN_PMAP_INCLUDE_CYS. For double mutants row = the index of the first
 * site p, letter = a, skip = p and base = wt[p, a].
 * STATE: five arrays of R L entries, owned by the caller, on the device, entry row * L + q. With a = letter[v]:
 *   best [R L] uint64     the smallest KEY  hits_ord(base[v] + ddg[v, q, b]) << 32 | a << 5 | b  over candidates whose sum is not NaN.
 *                         The sum is one IEEE fp32 round-to-nearest add. hits_ord(bits) is tmpnn_select_hits' order-preserving image
 *                         of fp32 bits on uint32: 0x80000000 (-0.0) is first taken as 0, then a word with the sign bit set is
 *                         inverted and any other gets the sign bit set. So the smallest key is the smallest value (-0.0 counts as
 *                         +0.0, +-inf are ordinary values), ties going to the smallest (a, b). To decode: o = key >> 32; the value's
 *                         bits are o ^ 0x80000000 if o has bit 31 set, else ~o; a = (key >> 5) & 31; b = key & 31.
 *   eps_lo [R L] uint64   the same key on e = ddg[v, q, b] - wt[q, b] (one fp32 subtract), over candidates whose e is not NaN: the
 *                         most negative epistasis of the pair.
 *   eps_hi [R L] uint64   the key with high word ~hits_ord(e): the smallest key is the LARGEST e, ties again to the smallest (a, b).
 *                         To decode, invert the high word first.
 *   eps_abs_sum [R L] fp32 and count [R L] int32. Per (v, q) an inner sum starts at +0.0 and takes |e| of the candidates with a
 *                         non-NaN e in ascending b, one fp32 add each, and each counts 1. Then, for every variant of the call
 *                         whose row lies in [0, R), in ascending v: sum = sum + inner (one fp32 add, also where inner is +0.0) and
 *                         count += its count. This order is the contract: it makes the sum's bits independent of how the variants
 *                         are cut into calls.
 * All ones in a key means "none". No multiply takes part, so nothing can be contracted; no atomics: reruns give identical bits.
 * Without TMPNN_PMAP_CONTINUE the call first sets the WHOLE state to empty (keys all ones, sum +0.0, count 0); with it the state
 * takes part, and entries of rows that no variant of the call names keep their bits. The caller promises that within one call the
 * variants of one row are contiguous (a row may go on in the next call); a row met in two separate runs of one call is undefined.
 * Two launches on `stream`: one thread per table row (v, q) leaves a record (three keys, the inner sum, the count) in the workspace
 * and, without CONTINUE, the launch empties the state; then one thread per (first variant of a run, q) folds the run's records in
 * ascending v into the state. With V == 0 or L == 0 (the input pointers may then be NULL) the call only resets the state, or keeps it
 * with CONTINUE; with R == 0 or L == 0 the state is empty, its pointers may be NULL and nothing is launched.
 * tmpnn_pair_map_workspace_bytes: V L records of 32 bytes as five arrays; 0 for sizes that are not served. Errors
 * before any launch: null pointer, ld or ld_wt < 20, negative sizes, unknown flag bits -> TMPNN_E_INVALID; L > 2048, or V * L or
 * R * L > 2^31 - 1 -> TMPNN_E_UNSUPPORTED; a short workspace -> TMPNN_E_WORKSPACE. */
enum { TMPNN_PMAP_INCLUDE_CYS = 1, TMPNN_PMAP_UPPER = 2, TMPNN_PMAP_CONTINUE = 4 };
size_t tmpnn_pair_map_workspace_bytes(int64_t V, int64_t L);              /* 0 for sizes not served */
int tmpnn_pair_map(const float *ddg, int ld, const int32_t *S_var, const float *base, const int32_t *row, const int32_t *letter,
                   const int32_t *skip, const float *wt, int ld_wt, int64_t V, int64_t L, int64_t R, int flags, uint64_t *best,
                   uint64_t *eps_lo, uint64_t *eps_hi, float *eps_abs_sum, int32_t *count, void *workspace, size_t workspace_bytes,
                   tmpnn_stream_t stream);

/* ---- one step of a beam search over n-point mutants: the k best DISTINCT children of a beam, with their sequence rows ------------
 * A search of order n is n decodes (tmpnn_decode_variants) plus n steps over one encoded backbone; no table goes to the host and no
 * sequence comes back. One call takes the V members of a beam over ONE protein of L rows, all on the device: ddg [V, L, ld] (ld >= 20;
 * relative to the member's own residue), S_var [V, L], score [V] (fp32: the member's cumulative ddG against the wild type), depth d
 * (1 <= d <= 8: the size of the children), muts [V, d - 1] (int32: the member's substitutions as q << 5 | b, ascending, distinct
 * positions; may be NULL when d = 1; a member with a negative entry is DEAD and contributes nothing), allowed_opt [L] (int32, nonzero =
 * the position may be mutated; NULL = all).
 * A CANDIDATE is (v, q, b) with member v alive and score[v] not NaN, S_var[v, q] < 20 (unsigned compare: negative = no residue),
 * b < 20, b != S_var[v, q], q not a position of muts[v], allowed[q] nonzero, b != cysteine (letter 1) unless TMPNN_BEAM_INCLUDE_CYS,
 * and a value that is not NaN and <= cutoff (+inf removes no candidate). The VALUE is score[v] + ddg[v, q, b]: one IEEE fp32
 * round-to-nearest add, the only float operation. Its 64-bit KEY is tmpnn_select_hits' order word of the sum's bits (-0.0 taken as
 * +0.0) in the high word and v << 16 | q << 5 | b in the low word, so L <= 2048 and V <= 65536.
 * The CHILD SET of a candidate is muts[v] with q << 5 | b added, sorted ascending; two candidates are duplicates when their child sets
 * are equal. RESULT: walk the candidates in ascending key order, keep a candidate when no earlier candidate has the same child set,
 * stop after k kept. Every distinct set is so represented by its smallest key: its smallest path value, ties going to the smaller
 * parent slot, then q, then b.
 * Outputs, best first: out_muts [k, d] (ascending), out_score [k] (the sum's bits recovered from the key; a -0.0 sum comes back as
 * +0.0), out_parent [k] (the member's slot), out_S [k, L] (S_var[parent] with q <- b), out_count [1]. Padding rows hold -1 in out_muts
 * and out_parent, NaN in out_score and 20 in out_S — a legal decoder letter that makes no candidates, so a padded beam can be decoded
 * and stepped again as it is (its padded rows are dead by their muts).
 * The caller PROMISES that live members are distinct sets. A child set of size d then has at most d parents in the beam, each with
 * exactly one candidate, so the first k distinct sets lie within the k d smallest keys; the entry serves k d <= 256. With members that
 * are not distinct the result is an unspecified subset: still no access outside the buffers, every returned set valid and distinct.
 * Three launches on `stream`, no atomics (reruns give identical bits): min(items, 8192 / m - 1) workgroups (m = the power of two
 * >= k d, an item = a member's block of 256 residues) keep their m leaders in LDS and leave k d keys each in the workspace; one
 * workgroup sorts them, builds the child sets, drops the duplicates and writes the first k; (row, block of 256 residues) writes out_S.
 * With V == 0 or L == 0 the input pointers may be NULL (and out_S with L == 0); the call writes padding and count 0.
 * tmpnn_beam_step_workspace_bytes: 0 for sizes that are not served. Errors before any launch: null pointer, k < 1, depth outside
 * [1, 8], ld < 20, negative sizes, unknown flag bits, NaN cutoff -> TMPNN_E_INVALID; k depth > 256, L > 2048, V > 65536 or
 * V * L > 2^31 - 1 -> TMPNN_E_UNSUPPORTED; a short workspace -> TMPNN_E_WORKSPACE. */
enum { TMPNN_BEAM_INCLUDE_CYS = 1 };
size_t tmpnn_beam_step_workspace_bytes(int64_t V, int64_t L, int k, int depth);   /* 0 for sizes not served */
int tmpnn_beam_step(const float *ddg, int ld, const int32_t *S_var, const float *score, const int32_t *muts, int depth,
                    const int32_t *allowed_opt, int64_t V, int64_t L, int k, float cutoff, int flags, int32_t *out_muts,
                    float *out_score, int32_t *out_parent, int32_t *out_S, int32_t *out_count, void *workspace,
                    size_t workspace_bytes, tmpnn_stream_t stream);
/* The same step for P PROTEINS of a packed axis of T rows in one call: row v of the [V, T] arrays holds beam slot v of EVERY protein,
 * so one tmpnn_decode_variants per round serves the whole pack. All pointers are device pointers: ddg [V, T, ld] (ld >= 20), S_var
 * [V, T], score [P, V], muts [P, V, d - 1] (words q << 5 | b with q the position WITHIN the protein; NULL allowed at d = 1; a member
 * with a negative entry is dead), allowed_opt [T] or NULL, offsets [P + 1] (int32, as for tmpnn_select_hits). For protein p with rows
 * [o_p, o_p + L_p) = [offsets[p], offsets[p + 1]) everything is tmpnn_beam_step's contract, word for word — the candidate rule, the one
 * fp32 add, the key hits_ord(sum) << 32 | v << 16 | q << 5 | b, the child sets, the walk, the padding, the caller's promise and
 * k d <= 256 — applied to ddg[:, o_p : o_p + L_p], S_var[:, o_p : o_p + L_p], score[p], muts[p] and allowed[o_p : o_p + L_p].
 * Outputs: out_muts [P, k, d], out_score [P, k], out_parent [P, k], out_count [P], and out_S [k, T]: row r holds, in protein p's
 * columns, the sequence of p's r-th child, 20 there in p's padding rows. The outputs are the next round's S_var, score and muts as they
 * stand, with V = k.
 * The offsets live in device memory, so the DEVICE checks them, in 64-bit arithmetic: 0 <= offsets[p] <= offsets[p + 1] <= T and
 * L_p <= max_len (<= 2048). Every workgroup of a protein evaluates the same predicate. A protein that fails gets out_count[p] = -1 and
 * padding in its out_muts, out_score and out_parent; no column of out_S is written for it and none of its table rows, scores or
 * substitutions is read; its neighbours are served. L_p = 0 is a good protein with count 0. No access ever leaves the buffers. Columns
 * of out_S that two proteins both claim are the caller's error: undefined values, still inside the buffers.
 * Three launches on `stream`, no atomics, no grid barrier: slots (p, w), W = min(V ceil(max_len / 256), 8192 / m - 1) per protein (m =
 * the power of two >= k d), where (p, w) loops over p's own items w, w + W, ... (an item = a member's block of 256 of p's rows), keeps m
 * leaders in LDS and leaves k d keys in the workspace; one workgroup per protein sorts them, builds the child sets, drops the
 * duplicates and writes the first k and the padding; (protein, kept row, block of 256 rows) writes out_S. Each grid is capped at 8192
 * workgroups that loop over their slots. Every output bit of a protein is independent of P, of its place in the pack, of W, of the
 * grid, and of a rerun.
 * With P == 0 nothing is launched. With V == 0 or T == 0 every input pointer may be NULL, offsets included: they are not read, every
 * protein gets count 0 and padding, and out_S (which may be NULL when T == 0) is not written.
 * tmpnn_beam_step_each_workspace_bytes: P W k d keys of 8 bytes plus P k words; 0 for sizes that are not served. Errors before any
 * launch: null pointer, k < 1, depth outside [1, 8], ld < 20, negative sizes, unknown flag bits, NaN cutoff -> TMPNN_E_INVALID;
 * k depth > 256, max_len > 2048, V > 65536 or V * T > 2^31 - 1 -> TMPNN_E_UNSUPPORTED; a short workspace -> TMPNN_E_WORKSPACE. */
size_t tmpnn_beam_step_each_workspace_bytes(int P, int64_t V, int max_len, int k, int depth);   /* 0 for sizes not served */
int tmpnn_beam_step_each(const float *ddg, int ld, const int32_t *S_var, const float *score, const int32_t *muts, int depth,
                         const int32_t *allowed_opt, const int32_t *offsets, int P, int64_t T, int64_t V, int max_len, int k,
                         float cutoff, int flags, int32_t *out_muts, float *out_score, int32_t *out_parent, int32_t *out_S,
                         int32_t *out_count, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream);

/* ---- conformer ensembles: per-mutation ddG statistics across the members of an ensemble -------------------------------------------
 * Whether a substitution is stabilising in ALL NMR models, AF2 ranks or MD frames, or in one conformer only. The members of an
 * ensemble are a ragged packed batch of tmpnn_ssm_forward (a protein's table does not depend on its batch); this entry reduces the
 * packed table across the members. All pointers are device pointers: ddg [T, ld] (ld >= 20), S [T] (the row's own letter; negative
 * or >= 20 = the row takes no part, unsigned compare), desc [E, 4] int32 = (row0, M, L, out_row0) per ensemble: M members of L rows
 * each, contiguous, member m's position q at table row row0 + m L + q, its results at output rows out_row0 + q. max_len >= every L.
 * Outputs [T_out, 20] each: mean, spread, lo, hi (fp32), lo_member, hi_member, count, below (int32); status [E] (int32).
 * The descriptors live in device memory, so the DEVICE checks them, in 64-bit arithmetic: row0, M, L, out_row0 >= 0, L <= max_len,
 * row0 + M L <= T, out_row0 + L <= T_out. An ensemble that fails gets status[e] = -1 and none of its output rows is written; a good
 * one gets status[e] = 0. No access ever leaves the buffers. Output ranges that overlap are the caller's error: undefined values,
 * still inside the buffers.
 * Per output entry (e, q, b < 20): member m PARTICIPATES when (uint32)S[row] < 20 and x = ddg[row, b] is not NaN (tested on the bits).
 *   count      the number of participants n;  below  the number of participants with x <= cutoff (+inf counts every one).
 *   mean       s starts at +0.0 and takes the participants in ASCENDING m, one fp32 round-to-nearest add each; mean = s / (float)n,
 *              correctly rounded.
 *   spread     t starts at +0.0; in ascending m: d = x - mean (one subtract), t = t + d * d (one multiply, one add, NOT contracted);
 *              spread = sqrt(t / (float)n): a correctly rounded divide, then a correctly rounded square root. The population form
 *              (ddof = 0): the spread of the ensemble as given, 0 for one member.
 *   Any NaN this arithmetic produces (inf - inf, +inf + -inf) is written as 0x7fc00000.
 *   lo, lo_member   the smallest key hits_ord(bits(x)) << 32 | m over the participants (hits_ord: tmpnn_pair_map's; -0.0 taken as
 *              +0.0, +-inf ordinary values): lo_member = that key's m, so ties go to the smallest m; lo = that member's own table
 *              bits (a -0.0 stays -0.0).
 *   hi, hi_member   the same with ~hits_ord in the high word: the largest value, ties again to the smallest m.
 *   n = 0 (M = 0 included): mean, spread, lo, hi = 0x7fc00000, the members -1, count and below 0.
 * The order of the sums is the contract: every bit is reproducible on a rerun and independent of E, of the ensemble's place in the
 * batch and of the launch shape. One launch on `stream`, one thread per output entry on a grid of (ceil(20 max_len / 256), E); no
 * workspace, no atomics. E == 0 is a no-op. Errors before any launch: null pointer (ddg and S may be NULL when T == 0, the outputs
 * when T_out == 0), ld < 20, negative sizes, NaN cutoff -> TMPNN_E_INVALID; T or T_out > 2^31 - 1, max_len > 8192 or E > 65535 ->
 * TMPNN_E_UNSUPPORTED. */
int tmpnn_ensemble_stats(const float *ddg, int ld, const int32_t *S, const int32_t *desc, int E, int64_t T, int64_t T_out,
                         int max_len, float cutoff, float *mean, float *spread, float *lo, float *hi, int32_t *lo_member,
                         int32_t *hi_member, int32_t *count, int32_t *below, int32_t *status, tmpnn_stream_t stream);
/* The same statistics THROUGH A ROW MAP, for members of unequal length that tmpnn_align_global has laid on one axis: rows [R] int32
 * (device), desc [E, 4] = (map0, M, L, out_row0): member m's position q reads table row r = rows[map0 + m L + q]. The member
 * participates when (uint32)r < T (any negative or out-of-range entry: the member is simply out at q), (uint32)S[r] < 20 and the value
 * is not NaN. Two members may name the same row; the members need not be contiguous in the table. Device checks: map0, M, L,
 * out_row0 >= 0, L <= max_len, map0 + M L <= R, out_row0 + L <= T_out. Everything else — the arithmetic and its order, the keys, the
 * NaN canonicalisation, status, the launch shape, the host-side errors (and R < 0, or rows NULL with R > 0 -> TMPNN_E_INVALID) — is
 * tmpnn_ensemble_stats': one kernel in two forms, templated on the addressing. With rows[map0 + m L + q] = row0 + m L + q the bits
 * are those of tmpnn_ensemble_stats. */
int tmpnn_ensemble_stats_rows(const float *ddg, int ld, const int32_t *S, const int32_t *rows, int64_t R, const int32_t *desc, int E,
                              int64_t T, int64_t T_out, int max_len, float cutoff, float *mean, float *spread, float *lo, float *hi,
                              int32_t *lo_member, int32_t *hi_member, int32_t *count, int32_t *below, int32_t *status,
                              tmpnn_stream_t stream);

/* ---- global alignment of letter-code sequences (the reference's pairwise2.align.globalxx, datasets.py:229-236) ---------------------
 * Lays sequences of unequal length on one axis: the members of an ensemble that differ in construct boundaries, missing termini, tags
 * or a point substitution. The rule is thermompnn_amd.datasets.global_alignment_map's, restated on int32 letter codes: identical
 * columns count 1, gaps are free. Two codes MATCH iff they are equal and (uint32)code < 20: a member's '-', 'X' (20, 21) and negative
 * codes never match anything. All pointers are device pointers: A [NA], B [NB] codes, desc [P, 6] int32 = (a0, n, b0, m, out0, add)
 * per pair: align a = A[a0 : a0 + n] (the axis) with b = B[b0 : b0 + m]. Outputs: out [NO] int32, aligned [P], status [P].
 *   score[i][j] = the LCS length of the suffixes a[i:], b[j:], filled from the bottom-right (score[n][.] = score[.][m] = 0).
 *   The trace starts at (0, 0) and, while i < n and j < m:
 *     1. a[i] matches b[j] and score[i][j] == score[i+1][j+1] + 1: a[i] is aligned to b[j]; i += 1, j += 1
 *     2. else score[i][j] == score[i+1][j]: i += 1
 *     3. else j += 1
 *   global_alignment_map's fourth branch, the mismatch column, cannot fire with this scoring: reaching it needs score[i][j] ==
 *   score[i+1][j+1] while score[i][j] > score[i+1][j], and score[i+1][j] >= score[i+1][j+1] always holds. So every mapped pair holds
 *   identical letters.
 *   out[out0 + q] = add + j when a[q] is aligned to b[j], else -1, for every q < n (with add = the member's first table row, out is
 *   directly a row map for tmpnn_ensemble_stats_rows); aligned[p] = the number of aligned columns = score[0][0]; status[p] = 0.
 * The DEVICE checks every descriptor in 64-bit arithmetic before any other access: a0, n, b0, m, out0 >= 0 (add: any value),
 * n <= max_n, m <= max_m, a0 + n <= NA, b0 + m <= NB, out0 + n <= NO. A pair that fails gets status[p] = -1 and none of its out entries
 * (nor aligned[p]) is written. n == 0 or m == 0 is a good pair with aligned = 0. out ranges that overlap are the caller's error.
 * One launch on `stream`: one workgroup of 1024 threads per pair on a persistent grid; a sweep over the anti-diagonals d = n + m - 2
 * .. 0 with three diagonals of 16-bit scores and both strings (as bytes) in LDS (3 (max_n + 2) 2 + max_n + max_m bytes: 65 548 at the
 * limit), one cell per thread; per cell a 2-bit trace decision into the workgroup's workspace slot, laid out diagonal by diagonal,
 * every diagonal from a word boundary, 16 cells folded over 16 lanes and stored as one word by one lane; then one thread walks at most
 * n + m steps. Integer work only, no atomics: results do not depend on the number of slots, on P or on the pair's place in the batch,
 * and a rerun gives the same bits.
 * tmpnn_align_workspace_bytes(max_n, max_m, P): min(P, 1024, what fits in 1 GiB, at least one) slots of the words of a max_n x max_m
 * pair with word-aligned diagonals (<= ceil(max_n max_m / 16) + max_n + max_m words), plus alignment slack; the entry uses as many
 * slots as the workspace it is given holds, so a workspace sized for P = 1 serves any P. 0 for sizes not served.
 * P == 0 is a no-op. Errors before any launch: null pointer (A, B, out may be NULL when their size is 0), negative size ->
 * TMPNN_E_INVALID; max_n or max_m > 8192 -> TMPNN_E_UNSUPPORTED; a workspace without room for one slot -> TMPNN_E_WORKSPACE. */
size_t tmpnn_align_workspace_bytes(int max_n, int max_m, int64_t P);
int tmpnn_align_global(const int32_t *A, int64_t NA, const int32_t *B, int64_t NB, const int32_t *desc, int P, int max_n, int max_m,
                       int32_t *out, int64_t NO, int32_t *aligned, int32_t *status, void *workspace, size_t workspace_bytes,
                       tmpnn_stream_t stream);

/* ---- rigid-body superposition of ensemble members: RMSD, per-column deviation, RMSF ----------------------------------------------
 * Why a ddG spread is large at a position: the backbone moves there, or it does not and the model is sensitive. And whether a member
 * is the same conformation at all. One optimal rigid-body fit of every member onto the ensemble's member fit_to, then reductions per
 * member and per axis column, from what a scan holds on the device before its forward. All pointers are device pointers.
 * Inputs: X [T, 4, 3] fp32 (only atom slot 1, C-alpha, is read), mask [T] fp32, rows [R] int32 or NULL (the identity map; R is then
 *   still the size of dev), desc [E, 6] int32 = (map0, M, L, out_row0, mem0, fit_to): M members of L axis columns each; max_len >= L.
 * Outputs: n_fit [NM] int32, rmsd [NM] fp32, xform [NM, 12] float64 (R row-major, then t: x' = R x + t takes the member into the
 *   frame of member fit_to), all three at member slot mem0 + m; dev [R] fp32 at map0 + m L + q, indexed like the map; rmsf [T_out]
 *   fp32 and col_count [T_out] int32 at out_row0 + q; status [E] int32.
 * Row r of (m, q) is rows[map0 + m L + q], or map0 + m L + q when rows is NULL. (m, q) is VALID when (uint32)r < T, mask[r] > 0 and
 *   the three C-alpha floats are finite (tested on the exponent bits). Two members may name the same rows.
 * The fit set of member m: F = {q : (m, q) and (fit_to, q) are both valid}; n_fit = |F|.
 * (R, t): the PROPER rotation (det = +1, never a reflection) and the translation that minimise sum_F |R p_m + t - p_f|^2, in float64:
 *   the centroids c_m, c_f over F; S[a][b] = sum_F (p_m - c_m)_a (p_f - c_f)_b; Horn's symmetric 4 x 4 matrix
 *     [Sxx+Syy+Szz  Syz-Szy       Szx-Sxz       Sxy-Syx     ]
 *     [             Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz     ]
 *     [                           -Sxx+Syy-Szz  Syz+Szy     ]
 *     [                                         -Sxx-Syy+Szz]
 *   solved by cyclic Jacobi (rotations (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) per sweep, until the off-diagonal squares sum to at most
 *   1e-40 of the diagonal squares, 32 sweeps at most); the eigenvector of the largest eigenvalue (ties: the first column), normalised,
 *   is the unit quaternion (w, x, y, z) of R; t = c_f - R c_m. A unit quaternion always gives a proper rotation, so a mirrored member,
 *   collinear points, two points or one need no special case: where the largest eigenvalue is not simple (such point sets; a vanishing
 *   gap to the second eigenvalue) the rotation is one of the minimisers, not a unique one. That is documented, not an error.
 *   rmsd = sqrt(sum_F |R p_m + t - p_f|^2 / n_fit), from the residuals and not from the eigenvalue (which loses everything to
 *   cancellation for near-identical members), in float64, rounded to fp32 once. Unique whenever n_fit >= 1.
 *   dev[map0 + m L + q] = |R p_m(q) + t - p_f(q)| (float64, rounded to fp32 once) for q in F when n_fit >= 3; 0x7fc00000 everywhere
 *   else in the member's L entries.
 *   m == fit_to: R = I and t = 0 exactly, rmsd = +0.0, dev = +0.0 on its valid columns whatever its n_fit (0x7fc00000 on the others).
 *   n_fit == 0 (the fit target with no valid column included): R = I, t = 0, rmsd = 0x7fc00000, dev all 0x7fc00000.
 *   n_fit 1 or 2: rmsd and xform as defined above; the member takes no part in dev or rmsf.
 * Column q: the PARTICIPANTS are the members valid at q that have n_fit >= 3 or are member fit_to. col_count = their number n;
 *   mu = sum x' / n with x' = R p + t, the sum taken in ascending m, in float64; rmsf = sqrt(sum |x' - mu|^2 / n), again in ascending
 *   m, rounded to fp32 once; n == 0 (M == 0 included): 0x7fc00000.
 * The DEVICE checks every descriptor in 64-bit arithmetic before any other access: map0, M, L, out_row0, mem0 >= 0, L <= max_len,
 *   map0 + M L <= R (and <= T when rows is NULL), out_row0 + L <= T_out, mem0 + M <= NM, 0 <= fit_to < M unless M == 0. An ensemble
 *   that fails gets status[e] = -1 and none of its outputs is written; a good one gets 0 and is served whatever its neighbours are.
 *   No access leaves the buffers. Output ranges or member slots that two good ensembles share are the caller's error.
 * Two launches on `stream`, no workspace, no atomics. Launch 1: one workgroup of 256 threads per member slot g < NM; it finds the
 *   smallest good ensemble e with mem0 <= g < mem0 + M (the host does not know M) and makes three sweeps over the member's columns
 *   (centroids; covariance; residuals), one thread solving the 4 x 4 between the second and the third. ORDER of every float64 sum:
 *   thread t of 256 takes the columns t, t + 256, ... in ascending order; a wavefront folds its 64 threads at distances 32, 16, .. 1
 *   (lane l takes lane l + distance); the four wavefront sums are added in ascending order. No contraction. Launch 2: one thread per
 *   (ensemble, column) on a grid of (ceil(max_len / 256), E); it loops over the members in ascending order and writes status. The
 *   order of every sum depends on (M, L, the data) only: every output bit, the float64 ones included, is reproducible on a rerun and
 *   independent of E, NM and the ensemble's place in the call.
 * E == 0 is a no-op. Errors before any launch: negative sizes, null pointer (X and mask may be NULL when T == 0, dev when R == 0, n_fit,
 *   rmsd, xform when NM == 0, rmsf and col_count when T_out == 0; rows may always be NULL) -> TMPNN_E_INVALID; T, T_out, R or NM >
 *   2^31 - 1, max_len > 8192 or E > 65535 -> TMPNN_E_UNSUPPORTED.
 * Limits: C-alpha only, one fit target per ensemble, no iteration to the mean structure, unweighted. */
int tmpnn_superpose(const float *X, const float *mask, const int32_t *rows, int64_t R, const int32_t *desc, int E, int64_t T, int64_t NM,
                    int64_t T_out, int max_len, int32_t *n_fit, float *rmsd, double *xform, float *dev, float *rmsf, int32_t *col_count,
                    int32_t *status, tmpnn_stream_t stream);

/* ---- bootstrap confidence intervals of the benchmark metrics (the reference's analysis/bootstrap.py) ------------------------------
 * B resamples with replacement of a table of N rows, and per resample and prediction column the five metrics of the benchmarking
 * script. No resample is sorted: the ranks inside a resample follow from one histogram over the tie groups of the original column and
 * one prefix sum, and every rank sum is an exact integer. All pointers are device pointers.
 * Inputs: values [C, N] float32, finite: row 0 the measured ddG, rows 1 .. C-1 the M = C - 1 prediction columns, 1 <= M <= 8.
 *   gid [C, N] int32: gid[c, i] = the 0-based dense rank of values[c, i] among the column's distinct values, equality being IEEE ==
 *   (-0.0 and +0.0 share a group; torch.unique(sorted=True, return_inverse=True) gives it, once per dataset).
 *   idx [B, N] int32: the N draws of each of the B resamples. N <= 2^20, B <= 2^20 per call.
 * Integer statistics of resample b and column c: cnt[g] = the number of draws d with gid[c, idx[b, d]] == g, P its inclusive prefix
 *   sum, X[g] = P[g - 1] + P[g] + 1 (twice the tie-averaged rank of group g inside the resample). For prediction column m, in int64,
 *   exactly: Sxy = sum_d X_m X_0, Sxx = sum_d X_m^2, Syy = sum_d X_0^2 (each X at the draw's own group); base = N (N + 1)^2.
 *   4 N^3 < 2^63 holds up to N = 2^20: the N limit. ranks [B, M, 3] int64 = (Sxy, Sxx, Syy).
 * metrics [B, M, 5] float64 = (r2, mse, rmse, spearman, pearson), the reference's column order:
 *   spearman = (Sxy - base) / (sqrt(Sxx - base) sqrt(Syy - base)), from the integers.
 *   With p, t the column's and the measured value at the draws, mp, mt their means (sum / N), pc = p - mp, tc = t - mt, all float64:
 *   mse = sum (p - t)^2 / N, rmse = sqrt(mse), r2 = 1 - sum (p - t)^2 / sum tc^2, pearson = sum pc tc / sqrt(sum pc^2 sum tc^2): the
 *   population forms of the host's metrics.get_metrics, centred on the resample's own means.
 *   Degeneracy is decided on the integers: Sxx == base (the column is constant inside the resample; N == 1 always is) -> spearman and
 *   pearson are NaN; Syy == base -> r2 is NaN as well. mse and rmse are always defined.
 * status [B] int32: 0 fine; -1 an idx entry of the resample is outside [0, N); -2 (when no idx entry is) a gid entry the resample
 *   meets is outside [0, N). Such a resample writes nothing else: its rows of metrics and ranks keep their bytes. Every index is
 *   compared with N before it addresses anything: no input makes the kernel read or write outside the buffers.
 * Determinism: a resample's outputs are a function of its own idx row (and values, gid) only: not of B, the row's slot, the workgroup
 *   that ran it, the form, or a rerun. The histogram uses integer atomics (no order in the result); there are no float atomics. Order
 *   of a float64 sum: thread t of 1024 takes the draws t, t + 1024, ... in ascending order; a wavefront folds its 64 threads at
 *   distances 32, 16, .. 1 (lane l takes lane l + distance); the 16 wavefront sums are added in ascending order. No contraction.
 * One launch on `stream`, one workgroup per resample on a persistent grid. The histogram and the scanned X of the measured column
 * (built once per resample) and of the current prediction column are u32 arrays in LDS for N <= 16384 (the LDS form, no workspace:
 * tmpnn_bootstrap_workspace_bytes is 0 and workspace may be NULL) or in the workspace (larger N, or TMPNN_BOOT_FORCE_WORKSPACE at any
 * N: min(B, 256) slots of 2 N words). Both forms give the same bits, the float64 outputs included.
 * B == 0 or N == 0 is a no-op. Errors before any launch: negative sizes, C outside [2, 9], unknown flag bits, null pointer ->
 * TMPNN_E_INVALID; N or B > 2^20 -> TMPNN_E_UNSUPPORTED; a short workspace -> TMPNN_E_WORKSPACE. */
enum { TMPNN_BOOT_FORCE_WORKSPACE = 1 };
size_t tmpnn_bootstrap_workspace_bytes(int C, int64_t N, int64_t B, int flags);   /* 0 for the LDS form and for sizes not served */
int tmpnn_bootstrap_metrics(const float *values, const int32_t *gid, int C, int64_t N, const int32_t *idx, int64_t B, double *metrics,
                            int64_t *ranks, int32_t *status, void *workspace, size_t workspace_bytes, int flags,
                            tmpnn_stream_t stream);

/* ---- host side: native PDB reader + packer ------------------------------------------
 * Replaces alt_parse_PDB (protein_mpnn_utils.py:183-350) + the packing of tied_featurize (:353-605) for one
 * structure: one pass over the file, all requested chains. `chains` = string of one-letter chain ids in the
 * order to concatenate them ("A", "AB", ...); NULL or "" = every chain present whose id is in the reference's default alphabet
 * (A-Z, a-z, 0-9, in that order; records of other chain ids are ignored, as the reference never reads them).
 * HOST pointers here (the only entry points that are not device-side). */
typedef struct tmpnn_pdb tmpnn_pdb_t;
int tmpnn_pdb_parse(const char *path, const char *chains, tmpnn_pdb_t **out);
/* n files on n_threads host threads; on failure every handle is released, outs[] is NULL and the message names the failing
 * files (up to eight of them). */
int tmpnn_pdb_parse_batch(const char *const *paths, const char *const *chains, int n, int n_threads,
                          tmpnn_pdb_t **outs);
/* The same with a per-file result: status [n] <- TMPNN_OK or the file's error code; a failing file leaves its handle NULL and
 * does NOT void the others (the call returns TMPNN_OK; tmpnn_last_error names the failing files) — a scan can skip or report
 * them (the reference's loop, analysis/SSM.py:105, would stop at the first bad structure). status == NULL: as above. */
int tmpnn_pdb_parse_batch_status(const char *const *paths, const char *const *chains, int n, int n_threads,
                                 tmpnn_pdb_t **outs, int32_t *status);
int64_t tmpnn_pdb_length(const tmpnn_pdb_t *p);      /* total residues L over the concatenated chains */
int tmpnn_pdb_num_chains(const tmpnn_pdb_t *p);
/* Any output may be NULL. X [L,4,3] fp32 with NaN -> 0, S [L] (ALPHABET index, gap -> 20), mask [L] (1 = all
 * four backbone atoms present), residue_idx [L] = 100 (c-1) + position, chain_enc [L] = c (1-based),
 * seq [L+1] = the parser's one-letter sequence ('-' at numbering gaps / unknown residues), NUL-terminated,
 * ca_mask [L] (1 = the CA atom is present: the mask compute_centrality uses, thermompnn_benchmarking.py:20-27). */
int tmpnn_pdb_fill(const tmpnn_pdb_t *p, float *X, int32_t *S, float *mask, int32_t *residue_idx,
                   int32_t *chain_enc, char *seq, float *ca_mask);
void tmpnn_pdb_free(tmpnn_pdb_t *p);
/* The parsed one-letter sequence (NUL-terminated, owned by the handle; same text tmpnn_pdb_fill copies out). */
const char *tmpnn_pdb_seq(const tmpnn_pdb_t *p);
/* n parsed structures -> ONE ragged batch in the caller's HOST buffers (pinned staging memory for an async H2D copy),
 * protein after protein in handle order, on n_threads host threads: offsets [n+1] (always written), then per residue the
 * arrays of tmpnn_pdb_fill (any may be NULL). capacity = residues the buffers hold; TMPNN_E_WORKSPACE if the batch is
 * longer. This is tied_featurize's packing (protein_mpnn_utils.py:353-605) for a whole chunk of a many-PDB scan. */
int tmpnn_pdb_pack_batch(tmpnn_pdb_t *const *handles, int n, int n_threads, int64_t capacity, float *X, int32_t *S,
                         float *mask, int32_t *residue_idx, int32_t *chain_enc, float *ca_mask, int32_t *offsets);

/* ---- host side: columnar result writer ------------------------------------------------
 * Replaces the cell-by-cell pandas frame + DataFrame.to_csv of analysis/SSM.py:102-176 (schema 0: ",WT Seq,Model,
 * Dataset,ddG_pred,position,wildtype,mutation,neighbors,best_AA,pdb") and analysis/custom_inference.py:64,94-111
 * (schema 1: ",Model,Dataset,ddG_pred,position,wildtype,mutation,pdb,chain"), byte for byte what pandas writes: '\n'
 * line ends, running index first, floats as repr(float(x)), empty cells for missing values (a NaN ddG included), minimal
 * quoting — pinned to files made by pandas itself (tests/golden/make_csv_golden.py).
 * HOST pointers; tables are the [T, ld] fp32 ddG tables of tmpnn_ssm_forward copied back (ld >= 20). */
typedef struct tmpnn_csv tmpnn_csv_t;
enum { TMPNN_CSV_PICK_BEST = 1,      /* one row per position carrying best_AA = argmin ddG (SSM.py:32-42,153-162); the schema-0
                                      * frame then has one more column, ",dupe_detector" = pdb + str(position) (:161), never dropped */
       TMPNN_CSV_INCLUDE_CYS = 2,    /* otherwise C is excluded from best_AA / rows mutating to C are dropped (:164-166) */
       TMPNN_CSV_NO_HEADER = 4 };    /* tmpnn_csv_open_ex: a part file of a sharded scan — no header line */
int tmpnn_csv_open(const char *path, int schema, tmpnn_csv_t **out);          /* creates the file, writes the header (of the first
                                                                               * listing written: PICK_BEST adds its column) */
/* The same with the header decided at once: flags = TMPNN_CSV_PICK_BEST (header with dupe_detector) | TMPNN_CSV_NO_HEADER. */
int tmpnn_csv_open_ex(const char *path, int schema, int flags, tmpnn_csv_t **out);
/* No file: the text goes into an anonymous mapping of `capacity` bytes (address space; pages are touched as text arrives), no
 * header line — one rank's share of a sharded scan, kept in memory until the ranks know where each protein's text belongs
 * (TMPNN_E_INVALID "No space left" when the listing outgrows the capacity). tmpnn_csv_mem -> the buffer and its fill; valid until
 * tmpnn_csv_close. */
int tmpnn_csv_open_mem(int schema, int flags, int64_t capacity, tmpnn_csv_t **out);
const char *tmpnn_csv_mem(const tmpnn_csv_t *c, int64_t *bytes_out);
/* The header line of a schema (flags: TMPNN_CSV_PICK_BEST) into buf -> its length, NUL-terminated (cap > length). */
int tmpnn_csv_header(int schema, int flags, char *buf, int cap);
/* Appends the listing of n proteins (may be called once per chunk of a scan; the running index continues). offsets [n+1]
 * index `table`; seqs[i] (length = rows of protein i; '-' positions are skipped) ; names[i] = 'pdb' cell; neighbors (may be
 * NULL) [T] -> 'neighbors' cell; `datasets` (may be NULL) per-protein 'Dataset' cells instead of `dataset`; chain: schema 1;
 * wt_cells (may be NULL) per-protein 'WT Seq' cells instead of seqs[i] — SSM.py:145-149 writes the DATASET's wild-type sequence
 * (dataset.wt_seqs[key]) there, which need not be the parsed structure's. */
int tmpnn_csv_write_ssm(tmpnn_csv_t *c, const float *table, int ld, const int32_t *offsets, int n,
                        const char *const *seqs, const char *const *wt_cells, const char *const *names, const int32_t *neighbors, const char *model,
                        const char *dataset, const char *const *datasets, const char *chain, int flags, int n_threads);
/* One rank's share of a scan that N ranks write into ONE file (the loop of SSM.py:105-176 sharded over GPUs): first_rows (may be
 * NULL) [n] = the running index of each protein's first row in the whole listing (every rank can compute them from the sequences
 * alone), bytes_out (may be NULL) [n] <- bytes of text written per protein; the ranks exchange those, and each places its
 * proteins' text at their offsets of the one output file (thermompnn_amd/dist.py: scan_files_to_csv). */
int tmpnn_csv_write_ssm_ex(tmpnn_csv_t *c, const float *table, int ld, const int32_t *offsets, int n,
                           const char *const *seqs, const char *const *wt_cells, const char *const *names, const int32_t *neighbors, const char *model,
                           const char *dataset, const char *const *datasets, const char *chain, int flags, int n_threads,
                           const int64_t *first_rows, int64_t *bytes_out);
/* Appends an explicit mutation list: triples [m,3] int64 (protein, 0-based position, amino-acid index < 20); schema 0. */
int tmpnn_csv_write_listed(tmpnn_csv_t *c, const float *table, int ld, const int32_t *offsets, int n,
                           const char *const *seqs, const char *const *names, const int32_t *neighbors, const char *model,
                           const char *dataset, const int64_t *triples, int64_t m);
int tmpnn_csv_close(tmpnn_csv_t *c, int64_t *rows_out, int64_t *bytes_out);   /* either may be NULL */
/* repr(float(v)) into buf (>= 32 bytes, NUL-terminated) -> length: the writer's number format, exposed for tests. */
int tmpnn_csv_format_double(double v, char *buf);

#ifdef __cplusplus
}
#endif
#endif /* TMPNN_H */
