// Internal host-side declarations shared by the .hip translation units of libtmpnn.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tmpnn.h"

// Pre-built f16x2 MFMA A-fragment image of one 128 x 128 weight block for the 8-wavefront kernels: 64 KB,
// [wavefront 8][k-step 4][plane 2][lane 64] x 16 B — a wavefront's fragment is four coalesced 1 KB loads per plane
// instead of 16-row gathers of fp32 that are split on the fly (tmpnn_node.hip: node_update8_split_kernel).
#define TM_WIMG_BYTES 65536
// The image rule: tmpnn_weights_create_p builds every image of an f16x2 handle where it fills the weight structs below, and
// stores its address in the struct member beside the weights it was made from; fp32 and bf16x3 handles build none and leave
// those members null. An f16x2 launcher refuses with TMPNN_E_INVALID when an image it needs is null; the f16x2 kernels assume them.
// Every struct keeps its images in one member `img` of nothing but `const char *`, so that the compiler counts them:
#define TM_IMG_COUNT(S) ((int)(sizeof(S::img) / sizeof(const char *)))

// kernel-side description of a node projection (an argument of node_proj_kernel's launcher and a member of NodeArgs):
// P [T,256]: P[t, 0:128] = Wa h_t + ba, P[t, 128:256] = Wc h_t (+ add_tab[add_idx[t]] when add_tab is set: the decoder's
// sequence term W1[:, 256:384] W_s[S_t], which rides with the neighbour's projection)
struct ProjSpec { const float *Wa; int lda; const float *ba; const float *Wc; int ldc; float *P; const float *add_tab; const int32_t *add_idx; };
// host side: the same with the images of its two blocks. The handle keeps one per consumer with P / add_* unset
// (enc_msg_proj, enc_edge_proj and dec_msg_proj of tmpnn_api.hip fill those per call).
struct NodeProj { ProjSpec spec; struct { const char *a, *c; } img; };
// Device pointers into the raw state-dict tensors of one layer, grouped by the launcher that takes them.
struct NodeW {   // node update: W3, LayerNorm 1, the feed-forward pair, LayerNorm 2
    const float *W3, *b3, *n1w, *n1b, *Win, *bin, *Wout, *bout, *n2w, *n2b;
    const char *img[9];            // W3, then (W_in rows 128 c.., W_out columns 128 c..) for c = 0..3: NodeArgs::img[0:9]
};
struct MsgW {    // message pass: the edge block of W1 (leading dimension 384 in the encoder, 512 in the decoder) and W2
    const float *W1e; int ld1; const float *W2, *b2;
    bool dec;
    struct { const char *w1, *w2, *p1, *p2; } img;   // p*: the same blocks with the K axis permuted inside every 32-deep step
                                                     // (msg8_wave_kernel: element e of lane group q <-> k = 32 c + 16 (e >> 2) + 4 q + (e & 3))
};
struct EdgeW {   // encoder edge update: the edge block of W11, W12, W13, LayerNorm 3
    const float *W11e, *W12, *b12, *W13, *b13, *n3w, *n3b;
    struct { const char *w11, *w12, *w13; } img;
};
struct EncW { NodeW node; MsgW msg; EdgeW edge; NodeProj msg_proj, edge_proj; };   // projections: W1a | W1c and W11a | W11c
struct DecW { NodeW node; MsgW msg; NodeProj msg_proj; };                          // W1a | W1d (spec.Wa is W1 itself)
struct FeatImg { const char *edge[4], *we; };   // edge_embedding.weight[:, 16:416] (four 128-column blocks, the last zero-padded), W_e
                                                // (a CA handle: edge[0:2] = the K blocks 0..127 and 128..159 of edge_ca, edge[2:4] null)
struct HeadImg { const char *unit[12]; };        // 9 blocks of the conv centre tap + 3 of both_out.1: HeadArgs::img

struct tmpnn_weights {
    int n_tensors;
    int mode;              // TM_MM_*: matrix-core path of this handle's per-edge GEMMs
    int ca;                // 1: the C-alpha-only flavour (tmpnn_weights_create_ca): edge_w is [128,167], the featurizer is tmpnn_graph_ca.hip's
    const float *t[TMPNN_N_TENSORS];
    // features
    const float *pos_w, *pos_b, *edge_w, *norm_edges_w, *norm_edges_b, *We_w, *We_b, *Ws_w;
    FeatImg feat_img;
    EncW enc[3];
    DecW dec[3];
    const float *Wout_w, *Wout_b;
    // head
    const float *conv_w, *conv_b, *mlp_w[3], *mlp_b[3], *ddg_w, *ddg_b;
    HeadImg head_img;
    // derived tables (in the caller's packed buffer)
    float *pos_table;      // [66,128]   (W_pos^T + b_pos) . W_edge[:, :16]^T
    float *seq_table[3];   // [21,128]   W_s . W1_dec[l][:, 256:384]^T
    float *conv_center;    // [384,384]  feature_convolution.weight[:, :, 4]
    float *edge_ca;        // [128,160]  CA handles: edge_w[:, 16:167] and 9 zero columns (GEMM 1 of the CA featurizer); null otherwise
};
// images of a full f16x2 handle, in the packed buffer behind the tables (a handle without the head tensors builds TM_N_HEAD_IMG fewer)
enum {
    TM_N_ENC_IMG = TM_IMG_COUNT(NodeW) + TM_IMG_COUNT(MsgW) + TM_IMG_COUNT(EdgeW) + 2 * TM_IMG_COUNT(NodeProj),
    TM_N_DEC_IMG = TM_IMG_COUNT(NodeW) + TM_IMG_COUNT(MsgW) + TM_IMG_COUNT(NodeProj),
    TM_N_HEAD_IMG = (int)(sizeof(HeadImg) / sizeof(const char *)),
    TM_N_IMG = (int)(sizeof(FeatImg) / sizeof(const char *)) + TM_N_HEAD_IMG + 3 * TM_N_ENC_IMG + 3 * TM_N_DEC_IMG
};
static_assert(TM_N_IMG == 122, "tmpnn_weights_packed_bytes() is part of the ABI: 122 images of 64 KB + the tables");

// scratch carved out of the caller's workspace for the message-passing layers
struct LayerWs {
    float *P;      // [T,256] node projections (A | C) for the message pass
    float *P2;     // [T,256] node projections for the encoder edge update
    float *Ssum;   // [T,128] sum_k mask_k * m2_k
    float *cnt;    // [T]     sum_k mask_k
    size_t bytes;  // of the workspace, up to the end of cnt
    float *ca_frames;   // [T,9] frames of a CA forward: shares P2's bytes, dead before the first node update writes P2 (layer_ws)
};

// Caller-owned buffers are carved into arrays that each start on a 256-byte boundary. A buffer's layout is ONE function that takes
// its arrays from a Carver and reports `used`: the entry runs it on the caller's buffer and compares with the caller's byte count
// before it touches an array; the buffer's *_bytes() runs it without a base (null pointers, only the count) and adds the buffer's
// slack. So a size cannot drift from its carve.
static inline size_t tm_align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Carver {
    char *base = nullptr;        // nullptr: measure
    size_t used = 0;
    Carver() {}
    // the caller's buffer as it is, or (align_base) from its first 256-byte boundary on, the bytes skipped charged to `used`
    Carver(void *buf, bool align_base) : base((char *)buf), used(align_base ? tm_align256((uintptr_t)buf) - (uintptr_t)buf : 0) {}
    template <class T> T *take(size_t n) {
        T *const r = base ? (T *)(base + used) : nullptr;
        used += tm_align256(n * sizeof(T));
        return r;
    }
};

int tm_set_error(int code, const char *fmt, ...);
int tm_check_launch(const char *what);
void tm_prof_begin(const char *name, hipStream_t st);   // no-ops unless tmpnn_profile_enable(1)
void tm_prof_end(hipStream_t st);

// tmpnn_graph.hip
// Optional extra of the fused forward: the k-NN kernel (one wavefront per residue) also writes the residue's all-zero initial
// node state hV0[t, 0:128] and its message projection P[t] = [ba | 0] (what node_proj of a zero state gives, exactly) —
// two launches (a memset and a fill) fewer per forward.
// fused forward: the k-NN kernel writes the zero state + first projection and ZEROES the caller's status word (workgroup 0; it
// then must not OR into that word itself — rows of an over-long protein are flagged by the last kernel, HeadArgs::maxlen_probe)
struct KnnInit { float *hV0; float *P; const float *ba; int32_t *status_zero; };
int launch_knn(const float *X, const float *mask, const int32_t *offsets, int N, int64_t T, int max_len, int K,
               int32_t *E_idx, float *D_nb, int32_t *status, hipStream_t st, KnnInit init = KnnInit{nullptr, nullptr, nullptr, nullptr});
int launch_centrality(const float *X, const float *mask, const int32_t *offsets, int N, int64_t T, float radius,
                      int32_t *out, hipStream_t st);
// small launches: the k-NN rows computed inside the featurizer launch (E_idx / D_nb are then OUTPUTS of it)
struct KnnFuse { const float *mask; const int32_t *offsets; int N, max_len, K; int32_t *E_idx; float *D_nb; KnnInit init; };
bool featurize_fusable(int mode, int64_t T);
int launch_featurize(const tmpnn_weights *w, const float *X, const int32_t *ridx, const int32_t *cenc,
                     const int32_t *E_idx, const float *D_nb, int64_t T, float *h_E, float *E_opt, hipStream_t st,
                     const KnnFuse *knn = nullptr);
// tmpnn_graph_ca.hip: the C-alpha-only flavour — frames O [T,9] once per residue, then the edge kernel that gathers them
int launch_prep_ca(tmpnn_weights *w, hipStream_t st);       // pos_table (167-column weight) + edge_ca
int launch_ca_frames(const float *X, const int32_t *offsets, int N, int64_t T, float *O, hipStream_t st);
int launch_featurize_ca(const tmpnn_weights *w, const float *X, const float *O, const int32_t *offsets, int N, const int32_t *ridx,
                        const int32_t *cenc, const int32_t *E_idx, const float *D_nb, int64_t T, float *h_E, float *E_opt, hipStream_t st);
int launch_gather_rows(const float *nodes, const void *idx, int idx64, int64_t n_rows, int64_t rows_per_batch,
                       int64_t nodes_per_batch, int C, float *out, hipStream_t st);
int launch_gather_edges(const float *edges, const int64_t *idx, int B, int N, int K, int C, float *out, hipStream_t st);

// tmpnn_layers.hip
// Every launcher below takes the precision (`mode`, TM_MM_*: the handle's) and the weight struct with its images as arguments.
int launch_msg(int mode, const MsgW &m, const float *P, const float *hE, const int32_t *E_idx, const float *mask, int64_t T,
               float *Ssum, float *cnt, hipStream_t st);
// kernel-side argument block of node_update (tmpnn_layers.hip: fp32 MFMA; tmpnn_node.hip: f16x2)
struct NodeArgs {
    const float *W3, *b3, *n1w, *n1b, *Win, *bin, *Wout, *bout, *n2w, *n2b;
    const float *h_in, *Ssum, *cnt, *mask;
    float *h_out;
    int T;
    ProjSpec proj[2];       // proj[k].P == nullptr -> not requested
    const char *img[13];    // fragment images of the 13 GEMM units (W3, W_in/W_out chunk pairs, projections) or all null
};
struct HeadArgs;
// head != nullptr (small launches, no projections requested): the ddG head of the same rows MAY run in the same launch (node_head_fused_kernel);
// *head_ran says whether it did — the caller launches the head itself otherwise
int launch_node_update_split(const NodeArgs &a, int64_t T, hipStream_t st, const HeadArgs *head = nullptr, bool *head_ran = nullptr);
bool node_head_fusable(int mode, int64_t T);
int launch_node_proj(const float *h, const NodeProj &np, int64_t T, hipStream_t st);
int launch_node_update(int mode, const NodeW &n, const float *h_in, const float *Ssum, const float *cnt, const float *mask, int64_t T,
                       float *h_out, const NodeProj *p0, const NodeProj *p1, hipStream_t st, const HeadArgs *head = nullptr,
                       bool *head_ran = nullptr);
int launch_enc_edge(int mode, const EdgeW &e, const float *P, float *hE, const int32_t *E_idx, int64_t T, hipStream_t st);

// tmpnn_head.hip
int launch_head(const tmpnn_weights *w, const float *hA, const float *hB, const int32_t *S, int64_t T, float *ddg,
                float *z_opt, int32_t *status, hipStream_t st, const int32_t *maxlen_probe = nullptr);
int tm_head_args(HeadArgs &a, const tmpnn_weights *w, const float *hA, const float *hB, const int32_t *S, int64_t T, float *ddg,
                 float *z_opt, int32_t *status, const int32_t *maxlen_probe);
int launch_log_probs(const tmpnn_weights *w, const float *h, int64_t T, float *out, int32_t *status, hipStream_t st,
                     const int32_t *maxlen_probe = nullptr);
int launch_seq_embed(const tmpnn_weights *w, const int32_t *S, int64_t T, float *hS, hipStream_t st);
int launch_head_generic(const float *const *hidden, int n_final, const float *Ws, const int32_t *S, int64_t T, const float *conv_w,
                        const float *conv_b, int n_layers, const float *const *mlp_w, const float *const *mlp_b, const int32_t *dims,
                        const float *ddg_w, const float *ddg_b, float *ddg, float *z_opt, float *buf0, float *buf1, int32_t *status,
                        hipStream_t st);
// tmpnn_train.hip: the launches of tmpnn_head_train_step (arguments validated by the caller); dfeat [M, D0] (may be null) receives
// d loss / d feature row and needs rows[i] == i. tmpnn_finetune.hip back-propagates it into ProteinMPNN.
int tm_head_train_core(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt,
                       const float *target, int64_t M, int lightattn, int n_layers, const int32_t *dims, int subtract_mut,
                       const float *params, float *grads, float p_drop, const float *keep_in, float *keep_out, uint64_t seed,
                       uint64_t step, float *loss, float *pred_opt, void *workspace, hipStream_t st, float *dfeat,
                       const float *dpred);
int tm_head_forward(const float *feat, int64_t n_feat, const int32_t *rows, const int32_t *mut, const int32_t *wt, int64_t M,
                    int lightattn, int n_layers, const int32_t *dims, int subtract_mut, const float *params, float p_drop,
                    const float *keep_in, float *keep_out, uint64_t seed, uint64_t step, float *pred, void *workspace, hipStream_t st);
int launch_range_check(const float *x, int64_t n, int32_t *status, hipStream_t st, const int32_t *maxlen_probe = nullptr,
                       int64_t T = 0);   // ORs TMPNN_STATUS_RANGE if any x is inf / NaN (+ the MAXLEN probe of the fused forward)
int launch_prep_tables(tmpnn_weights *w, hipStream_t st);

int launch_clock_probe(int blocks, int iters, unsigned long long *out, float *sink, hipStream_t st);
int launch_clock_monitor(int iters, unsigned long long *out, hipStream_t st);
// tmpnn_edge.hip, tmpnn_msg.hip (mode = TM_MM_F16X2 | TM_MM_BF16X3)
int launch_enc_edge_split(int mode, const EdgeW &e, const float *P, float *hE, const int32_t *E_idx, int64_t T, hipStream_t st);
int launch_msg_split(int mode, const MsgW &m, const float *P, const float *hE, const int32_t *E_idx, const float *mask, int64_t T,
                     float *Ssum, float *cnt, hipStream_t st);
// tmpnn_split.hip
int launch_gemm_probe(int mode, const float *X, const float *W, float *Y, int64_t T, int reps, hipStream_t st);
// tmpnn_edge_msg.hip, small launches (one tile per workgroup, f16x2): edge update of layer l + message pass of the next layer as
// one launch (bit-identical)
bool edge_msg_fusable(int mode, int64_t T);
int launch_edge_msg_fused(const EdgeW &e, const float *P_edge, float *hE, const int32_t *E_idx, const MsgW &m, const float *P_msg,
                          const float *mask, int64_t T, float *Ssum, float *cnt, hipStream_t st);
// tmpnn_variants.hip: V sequence variants over one encoded backbone, rows r = v T + t (tmpnn_decode_variants)
int launch_variant_expand(const float *hV, const float *P0, const float *mask, const float *tab, const int32_t *S_var, int64_t T,
                          int64_t V, float *hV_rep, float *P, float *mask_rep, int32_t *status, hipStream_t st);
int launch_variant_msg(int mode, const MsgW &m, const float *P, const float *hE, const int32_t *E_idx, const float *mask, int64_t T,
                       int64_t V, float *Ssum, float *cnt, hipStream_t st, const void *vis = nullptr, int32_t *remap = nullptr);
// order-masked decode (tmpnn_decode_ordered): visibility words [V T] x 8 bytes from rank [V,T]; P0 -> slot V of the table (layer 0)
int launch_variant_vis(const int32_t *rank, const int32_t *E_idx, int64_t T, int64_t V, void *vis, hipStream_t st);
int launch_variant_penc0(const float *P0, int64_t T, float *Penc, hipStream_t st);
int launch_variant_hidden(const float *const *h, int64_t T, int64_t V, float *out, hipStream_t st);
// tmpnn_sample.hip: N chains sampled autoregressively over one encoded backbone, 16 chains per workgroup, the T steps inside the launch
// (tmpnn_sample). Penc[l] [T,256]: projections of the encoder state; rank [N,T] (pre-filled with a large value) and tab [N,3,T,128]: scratch
// the tied form's extra arrays (tmpnn_sample_tied): close [N,T]; weight [N,T] by residue or null; the PSSM tables or null
struct SampleTied { const int32_t *close; const float *weight, *pssm_mix, *pssm_bias, *pssm_keep; };
// the per-protein form (tmpnn_sample_each): proteins [p0, p1) of offsets [P+1], each over its own steps; Penc / rank / tab then hold
// the rows [row0, row0 + rows) only; sched [p1 - p0] or null: the launch order as protein indices
struct SampleEach { const int32_t *offsets, *sched; int64_t p0, p1, row0, rows; };
int launch_sample_chains(const tmpnn_weights *w, const float *hE, const int32_t *E_idx, const float *hV, const float *P0,
                         const float *const *Penc, const float *mask, int64_t T, int64_t N, const int32_t *order, const int32_t *S_fixed,
                         const float *free_, const float *u, float inv_temp, const float *bias, const float *allowed, int32_t *S_out,
                         float *probs, int32_t *status, float *tab, int32_t *rank, const SampleTied *tied, const SampleEach *each,
                         hipStream_t st);
int launch_selftest(int32_t *status, hipStream_t st);
int tm_num_cus();
// Kernel-form switches (TMPNN_KNN_REG, TMPNN_NODE_DEEP, TMPNN_FUSE_SMALL ...) and the per-phase timers (TMPNN_*_PROF, which
// hipMalloc a scratch buffer, copy it back with a blocking hipMemcpy and print) exist ONLY in the debug variant of the library
//   python -m thermompnn_amd.build --variant debug -DTMPNN_DEBUG_BUILD      (-> libtmpnn_debug.so; select with TMPNN_LIB)
// The shipped libtmpnn.so picks every kernel form from the launch size and the handle's precision alone: its launchers never
// read the environment, never allocate device memory and never synchronise (the contract of include/tmpnn.h).
#ifdef TMPNN_DEBUG_BUILD
#include <stdlib.h>
#define TM_DBG_FLAG(name, dflt) ([] { const char *e_ = getenv(name); return e_ ? e_[0] != '0' : (bool)(dflt); }())
#define TM_DBG_INT(name, dflt) ([] { const char *e_ = getenv(name); return e_ ? atoi(e_) : (int)(dflt); }())
#else
#define TM_DBG_FLAG(name, dflt) ((bool)(dflt))
#define TM_DBG_INT(name, dflt) ((int)(dflt))
#endif
// matrix-core path of the per-edge GEMMs (tmpnn_split.h): a property of the weight handle (tmpnn_weights_create_p);
// TMPNN_PRECISION = f16x2 (default) | bf16x3 | fp32 only picks the default of handles created without one.
enum { TM_MM_FP32 = 0, TM_MM_BF16X3 = 1, TM_MM_F16X2 = 2 };
int launch_prep_wimg(const float *W, int ld, char *dst, hipStream_t st, int n_rows = 128, int k_valid = 128, int k_wrap = 0, bool perm = false);       // tmpnn_split.hip
// Non-finite tests under -fno-honor-nans. The kernels are built with relaxed NaN semantics, so hipcc may fold a NaN test
// on the RESULT of floating-point arithmetic (measured: both the sum test and the exponent-bit test on a computed value
// were compiled away; only the inf half survives). Tests are therefore made on raw bits LOADED FROM MEMORY, before any
// arithmetic touches them: tm_nonfinite_bits on integer loads of the same addresses.
__device__ __forceinline__ bool tm_nonfinite_bits(unsigned b) { return (b & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool tm_nonfinite(float x) { return tm_nonfinite_bits(__float_as_uint(x)); }   // inf only is guaranteed
// |x| >= 65504 (the largest fp16), inf and NaN included: a value the f16x2 split cannot carry. On raw bits, like the above.
__device__ __forceinline__ bool tm_f16_range_bits(unsigned b) { return (b & 0x7fffffffu) >= 0x477fe000u; }
// The same test on a COMPUTED value: the value is laundered through an empty asm first, so that hipcc (-fno-honor-nans) cannot
// reason "the result of fp arithmetic is never NaN" and fold the NaN half of the integer comparison away.
__device__ __forceinline__ bool tm_f16_range_computed(float x) {
    asm volatile("" : "+v"(x));
    return tm_f16_range_bits(__float_as_uint(x));
}
