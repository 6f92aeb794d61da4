// C-ABI of libtmpnn.so (declared in include/tmpnn.h): argument checking, the weight handle, workspace
// carving and the launch sequence of the fused forward. No device allocation, no stream sync.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <new>
#include <string>
#include <vector>

#include "tmpnn_internal.h"
#include "tmpnn_head_body.h"
#include "../../include/tmpnn_debug.h"

// ---- errors ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int tm_set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int tm_check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tm_set_error(TMPNN_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return TMPNN_OK;
}

// ---- optional per-kernel timing with HIP events on the launch stream (bench.py's roofline leg) --------
struct ProfRec { const char *name; hipEvent_t start, stop; };
static bool g_prof_on = false;
static bool g_prof_open = false;               // the launch between the last begin/end is being recorded
static std::string g_prof_only;                // tmpnn_profile_select: the one kernel to record ("" = all)
static std::vector<ProfRec> g_prof;            // recorded launches since the last enable/fetch
static std::vector<hipEvent_t> g_event_pool;   // recycled events

static hipEvent_t prof_event() {
    if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
void tm_prof_begin(const char *name, hipStream_t st) {
    g_prof_open = false;
    if (!g_prof_on || (!g_prof_only.empty() && g_prof_only != name)) return;
    ProfRec r{name, prof_event(), prof_event()};
    if (!r.start || !r.stop) return;
    (void)hipEventRecord(r.start, st);
    g_prof.push_back(r);
    g_prof_open = true;
}
void tm_prof_end(hipStream_t st) {
    if (!g_prof_open) return;
    (void)hipEventRecord(g_prof.back().stop, st);
    g_prof_open = false;
}

extern "C" int tmpnn_profile_select(const char *name) {
    g_prof_only = name ? name : "";
    return TMPNN_OK;
}

extern "C" int tmpnn_profile_enable(int on) {
    for (auto &r : g_prof) { g_event_pool.push_back(r.start); g_event_pool.push_back(r.stop); }
    g_prof.clear();
    g_prof_on = on != 0;
    return TMPNN_OK;
}

extern "C" int tmpnn_profile_fetch(const char **names, double *total_ms, int64_t *launches, int capacity) {
    if (capacity < 0 || (capacity > 0 && (!names || !total_ms || !launches)))
        return tm_set_error(TMPNN_E_INVALID, "profile_fetch: bad arguments");
    std::vector<const char *> order;
    std::map<std::string, std::pair<double, int64_t>> agg;
    for (auto &r : g_prof) {
        if (hipEventSynchronize(r.stop) != hipSuccess) return tm_set_error(TMPNN_E_LAUNCH, "profile_fetch: event sync failed");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.start, r.stop) != hipSuccess) return tm_set_error(TMPNN_E_LAUNCH, "profile_fetch: elapsed failed");
        auto it = agg.find(r.name);
        if (it == agg.end()) { order.push_back(r.name); agg[r.name] = {ms, 1}; }
        else { it->second.first += ms; it->second.second += 1; }
    }
    int n = 0;
    for (const char *nm : order) {
        if (n >= capacity) break;
        names[n] = nm; total_ms[n] = agg[nm].first; launches[n] = agg[nm].second;
        ++n;
    }
    for (auto &r : g_prof) { g_event_pool.push_back(r.start); g_event_pool.push_back(r.stop); }
    g_prof.clear();
    return n;
}
int tm_num_cus() {           // of the CURRENT device (cached per device: one process may drive several GPUs)
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cache[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

// Matrix-core path of the per-edge GEMMs (featurizer, message and edge-update kernels), see tmpnn_split.h:
//   "f16x2" (default) three-term fp16 split products, "bf16x3" six-term bf16 split products (both on the 16-bit matrix
//   cores with fp32 accumulation, fp32-class accuracy), "fp32" = v_mfma_f32_16x16x4_f32. All pass the same parity tests.
static int parse_mode(const char *e) {      // -1 = unknown
    if (e == nullptr || e[0] == 0 || strcmp(e, "f16x2") == 0) return (int)TM_MM_F16X2;
    if (strcmp(e, "bf16x3") == 0) return (int)TM_MM_BF16X3;
    if (strcmp(e, "fp32") == 0) return (int)TM_MM_FP32;
    return -1;
}
static const char *mode_name(int m) { return m == TM_MM_F16X2 ? "f16x2" : m == TM_MM_BF16X3 ? "bf16x3" : "fp32"; }
static int default_mode() {                  // TMPNN_PRECISION, read once; an unknown value is reported by weights_create
    static const int v = parse_mode(getenv("TMPNN_PRECISION"));
    return v;
}
// the process default (a handle's own precision is tmpnn_weights_precision); an unknown TMPNN_PRECISION reads as f16x2 here
extern "C" const char *tmpnn_matmul_mode(void) { return mode_name(default_mode() < 0 ? (int)TM_MM_F16X2 : default_mode()); }
extern "C" const char *tmpnn_weights_precision(const tmpnn_weights_t *w) { return w ? mode_name(w->mode) : nullptr; }

extern "C" int tmpnn_status_error(int32_t status) {
    if (status == 0) return TMPNN_OK;
    if (status & TMPNN_STATUS_MAXLEN)
        return tm_set_error(TMPNN_E_INVALID, "a protein is longer than the max_len passed to the call (its neighbour rows were left empty)");
    if (status & TMPNN_STATUS_RANGE)
        return tm_set_error(TMPNN_E_RANGE, "non-finite ddG / log-probability: an operand left the fp16 range of the f16x2 "
                                           "matrix-core path (|x| >= 65504); use precision \"bf16x3\" (full fp32 range)");
    if (status & TMPNN_STATUS_SELFTEST)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "device self-test failed: this libtmpnn.so was built with flags under which the f16x2 "
                                                 "GELU does not propagate NaN (fp16 overflow would go undetected) or the code-object "
                                                 "ABI differs from v5 (persistent tile loops would stride wrongly); rebuild with "
                                                 "python -m thermompnn_amd.build");
    return tm_set_error(TMPNN_E_INVALID, "unknown status bits 0x%x", (unsigned)status);
}

extern "C" int tmpnn_selftest(int32_t *status, tmpnn_stream_t stream) {
    if (!status) return tm_set_error(TMPNN_E_INVALID, "selftest: null status word");
    return launch_selftest(status, (hipStream_t)stream);
}

extern "C" int tmpnn_version(void) { return TMPNN_VERSION; }
extern "C" const char *tmpnn_last_error(void) { return g_err; }

// ---- tensor table ---------------------------------------------------------------------------------
struct TensorSpec { std::string name; int64_t numel; };

static const std::vector<TensorSpec> &tensor_table() {
    static std::vector<TensorSpec> t;
    if (!t.empty()) return t;
    auto add = [&](const std::string &n, int64_t e) { t.push_back({n, e}); };
    const int H = TMPNN_HID;
    add("features.embeddings.linear.weight", 16 * 66);
    add("features.embeddings.linear.bias", 16);
    add("features.edge_embedding.weight", H * 416);
    add("features.norm_edges.weight", H);
    add("features.norm_edges.bias", H);
    add("W_e.weight", H * H);
    add("W_e.bias", H);
    add("W_s.weight", TMPNN_VOCAB * H);
    auto layer = [&](const std::string &p, int num_in, bool edge) {
        const char *norms[3] = {"norm1", "norm2", "norm3"};
        for (int i = 0; i < (edge ? 3 : 2); ++i) { add(p + "." + norms[i] + ".weight", H); add(p + "." + norms[i] + ".bias", H); }
        add(p + ".W1.weight", (int64_t)H * (H + num_in)); add(p + ".W1.bias", H);
        add(p + ".W2.weight", H * H); add(p + ".W2.bias", H);
        add(p + ".W3.weight", H * H); add(p + ".W3.bias", H);
        if (edge) {
            add(p + ".W11.weight", (int64_t)H * (H + num_in)); add(p + ".W11.bias", H);
            add(p + ".W12.weight", H * H); add(p + ".W12.bias", H);
            add(p + ".W13.weight", H * H); add(p + ".W13.bias", H);
        }
        add(p + ".dense.W_in.weight", 4 * H * H); add(p + ".dense.W_in.bias", 4 * H);
        add(p + ".dense.W_out.weight", 4 * H * H); add(p + ".dense.W_out.bias", H);
    };
    for (int i = 0; i < 3; ++i) layer("encoder_layers." + std::to_string(i), 2 * H, true);
    for (int i = 0; i < 3; ++i) layer("decoder_layers." + std::to_string(i), 3 * H, false);
    add("W_out.weight", TMPNN_VOCAB * H);
    add("W_out.bias", TMPNN_VOCAB);
    // TransferModel head
    add("light_attention.feature_convolution.weight", 384 * 384 * 9);
    add("light_attention.feature_convolution.bias", 384);
    add("light_attention.attention_convolution.weight", 384 * 384 * 9);
    add("light_attention.attention_convolution.bias", 384);
    add("both_out.1.weight", 64 * 384); add("both_out.1.bias", 64);
    add("both_out.3.weight", 32 * 64); add("both_out.3.bias", 32);
    add("both_out.5.weight", TMPNN_VOCAB * 32); add("both_out.5.bias", TMPNN_VOCAB);
    add("ddg_out.weight", 1); add("ddg_out.bias", 1);
    return t;
}

extern "C" int tmpnn_num_tensors(void) { return (int)tensor_table().size(); }
extern "C" const char *tmpnn_tensor_name(int i) {
    const auto &t = tensor_table();
    return (i < 0 || i >= (int)t.size()) ? nullptr : t[i].name.c_str();
}
extern "C" int64_t tmpnn_tensor_numel(int i) {
    const auto &t = tensor_table();
    return (i < 0 || i >= (int)t.size()) ? -1 : t[i].numel;
}

static const size_t POS_TABLE_FLOATS = 66 * TMPNN_HID, SEQ_TABLE_FLOATS = TMPNN_VOCAB * TMPNN_HID,
                    CONV_CENTER_FLOATS = 384 * 384;
// A CA handle (tmpnn_weights_create_ca): no head, so no centre tap and no head images; edge_ca [128,160] behind the tables; two
// featurizer images (the K blocks of edge_ca) instead of four.
static const size_t EDGE_CA_FLOATS = 128 * 160;
enum { TM_N_IMG_CA = TM_N_IMG - TM_N_HEAD_IMG - 2 };
static size_t packed_bytes_for(int mode, bool ca = false) {    // the f16 fragment images exist for f16x2 handles only (nothing else reads them)
    if (ca) return (POS_TABLE_FLOATS + 3 * SEQ_TABLE_FLOATS + EDGE_CA_FLOATS) * sizeof(float) + (mode == TM_MM_F16X2 ? (size_t)TM_N_IMG_CA * TM_WIMG_BYTES : 0);
    return (POS_TABLE_FLOATS + 3 * SEQ_TABLE_FLOATS + CONV_CENTER_FLOATS) * sizeof(float) +
           (mode == TM_MM_F16X2 ? (size_t)TM_N_IMG * TM_WIMG_BYTES : 0);
}
extern "C" size_t tmpnn_weights_packed_bytes(void) { return packed_bytes_for(TM_MM_F16X2); }   // upper bound over the precisions
extern "C" size_t tmpnn_weights_packed_bytes_p(const char *precision) {
    const int mode = precision ? parse_mode(precision) : default_mode();
    return mode < 0 ? 0 : packed_bytes_for(mode);
}

extern "C" size_t tmpnn_weights_ca_packed_bytes_p(const char *precision) {
    const int mode = precision ? parse_mode(precision) : default_mode();
    return mode < 0 ? 0 : packed_bytes_for(mode, true);
}
extern "C" int64_t tmpnn_tensor_numel_ca(int i) {     // the 118 ProteinMPNN tensors; entry 2 is edge_embedding.weight [128,167]
    if (i < 0 || i >= TMPNN_N_MPNN_TENSORS) return -1;
    return i == 2 ? (int64_t)TMPNN_HID * 167 : tensor_table()[i].numel;
}
extern "C" int tmpnn_weights_is_ca(const tmpnn_weights_t *w) { return w ? w->ca : 0; }

extern "C" int tmpnn_weights_create(tmpnn_weights_t **out, const float *const *tensors, int n_tensors, void *packed,
                                    size_t packed_bytes, tmpnn_stream_t stream) {
    return tmpnn_weights_create_p(out, tensors, n_tensors, packed, packed_bytes, nullptr, stream);
}

static int weights_create(bool ca, tmpnn_weights_t **out, const float *const *tensors, int n_tensors, void *packed, size_t packed_bytes,
                          const char *precision, tmpnn_stream_t stream);
extern "C" int tmpnn_weights_create_p(tmpnn_weights_t **out, const float *const *tensors, int n_tensors, void *packed,
                                      size_t packed_bytes, const char *precision, tmpnn_stream_t stream) {
    return weights_create(false, out, tensors, n_tensors, packed, packed_bytes, precision, stream);
}
extern "C" int tmpnn_weights_create_ca(tmpnn_weights_t **out, const float *const *tensors, int n_tensors, void *packed,
                                       size_t packed_bytes, const char *precision, tmpnn_stream_t stream) {
    return weights_create(true, out, tensors, n_tensors, packed, packed_bytes, precision, stream);
}

// ca: the C-alpha-only flavour — the same 118 tensors with edge_embedding.weight [128,167]; ThermoMPNN has no CA flavour, so no head
static int weights_create(bool ca, tmpnn_weights_t **out, const float *const *tensors, int n_tensors, void *packed, size_t packed_bytes,
                          const char *precision, tmpnn_stream_t stream) {
    const int mode = precision ? parse_mode(precision) : default_mode();
    if (mode < 0)                  // first: a caller that sized `packed` with tmpnn_weights_packed_bytes_p() got 0 for this name
        return tm_set_error(TMPNN_E_INVALID, "weights_create: unknown precision '%s' (f16x2 | bf16x3 | fp32)",
                            precision ? precision : getenv("TMPNN_PRECISION"));
    if (!out || !tensors || !packed) return tm_set_error(TMPNN_E_INVALID, "weights_create: null argument");
    if (tensor_table().size() != TMPNN_N_TENSORS) return tm_set_error(TMPNN_E_INVALID, "internal tensor table size");
    if (ca && n_tensors != TMPNN_N_MPNN_TENSORS)
        return tm_set_error(TMPNN_E_INVALID, "weights_create_ca: n_tensors must be %d (a CA model has no ddG head), got %d",
                            TMPNN_N_MPNN_TENSORS, n_tensors);
    if (n_tensors != TMPNN_N_MPNN_TENSORS && n_tensors != TMPNN_N_TENSORS)
        return tm_set_error(TMPNN_E_INVALID, "weights_create: n_tensors must be %d or %d, got %d", TMPNN_N_MPNN_TENSORS,
                            TMPNN_N_TENSORS, n_tensors);
    if (packed_bytes < packed_bytes_for(mode, ca))
        return tm_set_error(TMPNN_E_WORKSPACE, "weights_create: packed buffer %zu < %zu bytes", packed_bytes,
                            packed_bytes_for(mode, ca));
    if (((uintptr_t)packed & 15) != 0) return tm_set_error(TMPNN_E_INVALID, "weights_create: packed buffer must be 16-byte aligned");
    for (int i = 0; i < n_tensors; ++i)
        if (!tensors[i] || ((uintptr_t)tensors[i] & 15) != 0)
            return tm_set_error(TMPNN_E_INVALID, "weights_create: tensor %d (%s) is null or not 16-byte aligned", i,
                                tmpnn_tensor_name(i));
    tmpnn_weights *w = new (std::nothrow) tmpnn_weights();
    if (!w) return tm_set_error(TMPNN_E_INVALID, "weights_create: host allocation failed");
    memset(w, 0, sizeof(*w));
    w->n_tensors = n_tensors;
    w->mode = mode;
    w->ca = ca ? 1 : 0;
    std::map<std::string, const float *> by_name;
    for (int i = 0; i < n_tensors; ++i) { w->t[i] = tensors[i]; by_name[tensor_table()[i].name] = tensors[i]; }
    auto get = [&](const std::string &n) -> const float * {
        auto it = by_name.find(n);
        return it == by_name.end() ? nullptr : it->second;
    };
    w->pos_w = get("features.embeddings.linear.weight");
    w->pos_b = get("features.embeddings.linear.bias");
    w->edge_w = get("features.edge_embedding.weight");
    w->norm_edges_w = get("features.norm_edges.weight");
    w->norm_edges_b = get("features.norm_edges.bias");
    w->We_w = get("W_e.weight");
    w->We_b = get("W_e.bias");
    w->Ws_w = get("W_s.weight");
    auto node = [&](const std::string &p) {
        return NodeW{get(p + "W3.weight"), get(p + "W3.bias"), get(p + "norm1.weight"), get(p + "norm1.bias"),
                     get(p + "dense.W_in.weight"), get(p + "dense.W_in.bias"), get(p + "dense.W_out.weight"), get(p + "dense.W_out.bias"),
                     get(p + "norm2.weight"), get(p + "norm2.bias"), {}};
    };
    // W [128, ld]: the h_i block is columns [0:128), the h_j block starts at column c_off
    auto proj = [](const float *W, int ld, int c_off, const float *b) {
        return NodeProj{ProjSpec{W, ld, b, W + c_off, ld, nullptr, nullptr, nullptr}, {}};
    };
    for (int l = 0; l < 3; ++l) {
        // encoder, W1 and W11 columns: [0:128) h_i | [128:256) e_ij | [256:384) h_j
        const std::string p = "encoder_layers." + std::to_string(l) + ".";
        const float *W1 = get(p + "W1.weight"), *W11 = get(p + "W11.weight");
        EncW &e = w->enc[l];
        e.node = node(p);
        e.msg = MsgW{W1 + 128, 384, get(p + "W2.weight"), get(p + "W2.bias"), false, {}};
        e.edge = EdgeW{W11 + 128, get(p + "W12.weight"), get(p + "W12.bias"), get(p + "W13.weight"), get(p + "W13.bias"),
                       get(p + "norm3.weight"), get(p + "norm3.bias"), {}};
        e.msg_proj = proj(W1, 384, 256, get(p + "W1.bias"));
        e.edge_proj = proj(W11, 384, 256, get(p + "W11.bias"));
        // decoder, W1 columns: [0:128) h_i | [128:256) e_ij | [256:384) W_s[S_j] (folded into seq_table, added to the h_j term) | [384:512) h_j
        const std::string d = "decoder_layers." + std::to_string(l) + ".";
        const float *D1 = get(d + "W1.weight");
        DecW &c = w->dec[l];
        c.node = node(d);
        c.msg = MsgW{D1 + 128, 512, get(d + "W2.weight"), get(d + "W2.bias"), true, {}};
        c.msg_proj = proj(D1, 512, 384, get(d + "W1.bias"));
    }
    w->Wout_w = get("W_out.weight");
    w->Wout_b = get("W_out.bias");
    if (n_tensors == TMPNN_N_TENSORS) {
        w->conv_w = get("light_attention.feature_convolution.weight");
        w->conv_b = get("light_attention.feature_convolution.bias");
        const char *idx[3] = {"1", "3", "5"};
        for (int i = 0; i < 3; ++i) {
            w->mlp_w[i] = get(std::string("both_out.") + idx[i] + ".weight");
            w->mlp_b[i] = get(std::string("both_out.") + idx[i] + ".bias");
        }
        w->ddg_w = get("ddg_out.weight");
        w->ddg_b = get("ddg_out.bias");
    }
    float *p = (float *)packed;
    w->pos_table = p; p += POS_TABLE_FLOATS;
    for (int l = 0; l < 3; ++l) { w->seq_table[l] = p; p += SEQ_TABLE_FLOATS; }
    if (ca) { w->edge_ca = p; p += EDGE_CA_FLOATS; }
    else { w->conv_center = p; p += CONV_CENTER_FLOATS; }
    int rc = launch_prep_tables(w, (hipStream_t)stream);
    if (rc == TMPNN_OK && ca) rc = launch_prep_ca(w, (hipStream_t)stream);
    if (mode == TM_MM_F16X2) {   // fragment images of every 128 x 128 block the f16x2 kernels multiply by (the image rule, tmpnn_internal.h)
        char *img = (char *)p, *const img_end = img + (size_t)(ca ? TM_N_IMG_CA : TM_N_IMG) * TM_WIMG_BYTES;       // (inside `packed`: checked above)
        auto image = [&](const float *base, int ld, int n_rows = 128, int k_valid = 128, int k_wrap = 0, bool perm = false) -> const char * {
            if (rc != TMPNN_OK || img == img_end) return nullptr;
            const char *at = img;
            rc = launch_prep_wimg(base, ld, img, (hipStream_t)stream, n_rows, k_valid, k_wrap, perm);
            img += TM_WIMG_BYTES;
            return at;
        };
        auto node_images = [&](NodeW &n) {
            n.img[0] = image(n.W3, 128);
            for (int c = 0; c < 4; ++c) { n.img[1 + 2 * c] = image(n.Win + (size_t)128 * c * 128, 128); n.img[2 + 2 * c] = image(n.Wout + 128 * c, 512); }
        };
        auto proj_images = [&](NodeProj &np) { np.img = {image(np.spec.Wa, np.spec.lda), image(np.spec.Wc, np.spec.ldc)}; };
        auto msg_images = [&](MsgW &m) { m.img.w1 = image(m.W1e, m.ld1); m.img.w2 = image(m.W2, 128); };
        auto msg_images_kperm = [&](MsgW &m) { m.img.p1 = image(m.W1e, m.ld1, 128, 128, 0, true); m.img.p2 = image(m.W2, 128, 128, 128, 0, true); };
        if (ca) {   // the K blocks 0..127 and 128..159 of edge_ca (derived just above, on the same stream)
            for (int b = 0; b < 2; ++b) w->feat_img.edge[b] = image(w->edge_ca + 128 * b, 160, 128, b == 0 ? 128 : 32);
        } else {
            // RBF columns 16..415 (K padded to 416 + 96), then — K positions 400..415 — the 16 positional columns 0..15 of the same rows
            for (int b = 0; b < 4; ++b) w->feat_img.edge[b] = image(w->edge_w + 16 + 128 * b, 416, 128, b < 3 ? 128 : 16, b < 3 ? 0 : 16);
        }
        w->feat_img.we = image(w->We_w, 128);
        if (n_tensors == TMPNN_N_TENSORS) {          // ddG head: centre tap (derived just above, on the same stream) + both_out.1
            for (int u = 0; u < 9; ++u) w->head_img.unit[u] = image(w->conv_center + (size_t)128 * (u / 3) * 384 + 128 * (u % 3), 384);
            for (int u = 0; u < 3; ++u) w->head_img.unit[9 + u] = image(w->mlp_w[0] + 128 * u, 384, 64);
        }
        for (int l = 0; l < 3; ++l) {
            EncW &e = w->enc[l];
            node_images(e.node); proj_images(e.msg_proj); proj_images(e.edge_proj); msg_images(e.msg);
            e.edge.img = {image(e.edge.W11e, 384), image(e.edge.W12, 128), image(e.edge.W13, 128)};
            DecW &d = w->dec[l];
            node_images(d.node); proj_images(d.msg_proj); msg_images(d.msg);
        }
        for (int l = 0; l < 3; ++l) { msg_images_kperm(w->enc[l].msg); msg_images_kperm(w->dec[l].msg); }   // (behind the others: the order of the packed buffer is kept)
        // every image member above is filled exactly once: the count the structs declare is the count built
        const int n_built = (int)((img - (char *)p) / TM_WIMG_BYTES), n_want = ca ? TM_N_IMG_CA : TM_N_IMG - (n_tensors == TMPNN_N_TENSORS ? 0 : TM_N_HEAD_IMG);
        if (rc == TMPNN_OK && n_built != n_want) rc = tm_set_error(TMPNN_E_INVALID, "weights_create: built %d fragment images, expected %d", n_built, n_want);
    }
    if (rc != TMPNN_OK) { delete w; return rc; }
    *out = w;
    return TMPNN_OK;
}

extern "C" void tmpnn_weights_destroy(tmpnn_weights_t *w) { delete w; }

// ---- helpers --------------------------------------------------------------------------------------
#define REQUIRE(cond, ...) do { if (!(cond)) return tm_set_error(TMPNN_E_INVALID, __VA_ARGS__); } while (0)
#define TRY(expr) do { int rc_ = (expr); if (rc_ != TMPNN_OK) return rc_; } while (0)

static const int64_t T_MAX = ((int64_t)1 << 31) / (TMPNN_KS * 4) - 1;   // int32 tile arithmetic inside kernels

// ---- layouts of the caller-owned buffers: one function each, run by the entry on the buffer and by *_bytes() without a base -------
// A layout struct's members are carved in the order they are declared (a braced list is evaluated left to right); `bytes` comes last.
// *_bytes() adds 256 bytes of slack per alignment of the caller's base (tmpnn_workspace_bytes has carried two since the layer part
// was split off).
static LayerWs layer_ws(Carver &c, int64_t T) {             // (by reference: the forward's and the encoder's layouts go on behind it)
    const size_t n = (size_t)T;
    LayerWs ws{c.take<float>(n * 256), c.take<float>(n * 256), c.take<float>(n * TMPNN_HID), c.take<float>(n), c.used, nullptr};
    // The frames of a CA forward, O [T,9], share P2's bytes (9 of its 256 floats per row): the edge-update projection is first written
    // by node update 0, which every encoder runs behind the featurizer, the frames' only reader. Carved HERE so that the overlap is
    // part of the layout: the sizers return what they return for a full-backbone handle.
    static_assert(9 <= 256, "the frames must fit the projection they share bytes with");
    ws.ca_frames = ws.P2;
    return ws;
}
struct FwdWs { LayerWs l; int32_t *E_idx; float *D_nb, *hE, *hV[4]; size_t bytes; };       // tmpnn_ssm_forward
static FwdWs fwd_ws(Carver c, int64_t T) {
    const size_t n = (size_t)T, nh = n * TMPNN_HID;
    return FwdWs{layer_ws(c, T), c.take<int32_t>(n * TMPNN_KS), c.take<float>(n * TMPNN_KS), c.take<float>(n * TMPNN_KS * TMPNN_HID),
                 {c.take<float>(nh), c.take<float>(nh), c.take<float>(nh), c.take<float>(nh)}, c.used};
}
struct EncWs { LayerWs l; float *D_nb; size_t bytes; };                                     // tmpnn_encode
static EncWs enc_ws(Carver c, int64_t T) { return EncWs{layer_ws(c, T), c.take<float>((size_t)T * TMPNN_KS), c.used}; }

extern "C" size_t tmpnn_layer_workspace_bytes(int64_t T) { Carver c; return T < 0 ? 0 : layer_ws(c, T).bytes + 256; }
extern "C" size_t tmpnn_workspace_bytes(int64_t T) { return T < 0 ? 0 : fwd_ws(Carver(), T).bytes + 512; }

// The entries that take whatever the carve fits (layers, ssm_forward, encode) carve from the aligned base and check the layer part here.
static int layer_ws_fits(void *workspace, size_t bytes, const LayerWs &ws, int64_t T) {
    if (!workspace || Carver(workspace, true).used > bytes) return tm_set_error(TMPNN_E_WORKSPACE, "workspace missing or too small");
    if (ws.bytes > bytes) return tm_set_error(TMPNN_E_WORKSPACE, "workspace too small for T=%lld", (long long)T);
    return TMPNN_OK;
}
static int carve_layer_ws(void *workspace, size_t bytes, int64_t T, LayerWs *ws) {
    Carver c(workspace, true);
    *ws = layer_ws(c, T);
    return layer_ws_fits(workspace, bytes, *ws, T);
}

// Which node projection the NEXT consumer of h_V needs (fused into node_update): encoder layer l+1's message
// pass, or decoder layer 0's after the last encoder layer; decoder layer l+1's after decoder layer l. The handle holds the
// weights and images of each; the destination (and the decoder's sequence term) is the call's.
static NodeProj proj_into(NodeProj np, float *P) { np.spec.P = P; return np; }
static NodeProj enc_msg_proj(const tmpnn_weights *w, int l, float *P) { return proj_into(w->enc[l].msg_proj, P); }
static NodeProj enc_edge_proj(const tmpnn_weights *w, int l, float *P) { return proj_into(w->enc[l].edge_proj, P); }
static NodeProj dec_msg_proj(const tmpnn_weights *w, int l, float *P, const int32_t *S) {   // S == nullptr: without the sequence term
    NodeProj np = proj_into(w->dec[l].msg_proj, P);
    if (S) { np.spec.add_tab = w->seq_table[l]; np.spec.add_idx = S; }
    return np;
}

// One encoder layer (EncLayer :819-838): message pass, node update, edge update with the NEW node states.
// have_P:   ws.P already holds this layer's message projection (written by the previous node update);
// have_msg: ws.Ssum / ws.cnt already hold this layer's message sums (the previous layer's edge update ran them in its launch);
// next:     the node update also writes this projection of the new state (besides the edge update's, into ws.P2);
// then:     small launches — the message pass that follows (over ws.P, which `next` must fill) runs inside the edge update's launch.
static int run_enc_layer(const tmpnn_weights *w, int l, float *hV, float *hE, const int32_t *E_idx, const float *mask,
                         int64_t T, const LayerWs &ws, bool have_P, bool have_msg, const NodeProj *next, const MsgW *then,
                         hipStream_t st) {
    const EncW &e = w->enc[l];
    if (!have_P) {
        const NodeProj mp = enc_msg_proj(w, l, ws.P);
        TRY(launch_node_proj(hV, mp, T, st));
    }
    if (!have_msg) TRY(launch_msg(w->mode, e.msg, ws.P, hE, E_idx, mask, T, ws.Ssum, ws.cnt, st));
    const NodeProj ep = enc_edge_proj(w, l, ws.P2);
    TRY(launch_node_update(w->mode, e.node, hV, ws.Ssum, ws.cnt, mask, T, hV, &ep, next, st));
    if (then) return launch_edge_msg_fused(e.edge, ws.P2, hE, E_idx, *then, ws.P, mask, T, ws.Ssum, ws.cnt, st);
    return launch_enc_edge(w->mode, e.edge, ws.P2, hE, E_idx, T, st);
}

// One decoder layer; have_P, have_msg and next as above. head: the ddG head of the same rows may ride in the node update's launch
// (launch_node_update; the caller asked node_head_fusable).
static int run_dec_layer(const tmpnn_weights *w, int l, const float *hV_in, float *hV_out, const float *hE,
                         const int32_t *E_idx, const int32_t *S, const float *mask, int64_t T, const LayerWs &ws,
                         bool have_P, bool have_msg, const NodeProj *next, hipStream_t st, const HeadArgs *head = nullptr,
                         bool *head_ran = nullptr) {
    const DecW &d = w->dec[l];
    if (!have_P) {
        const NodeProj mp = dec_msg_proj(w, l, ws.P, S);
        TRY(launch_node_proj(hV_in, mp, T, st));
    }
    if (!have_msg) TRY(launch_msg(w->mode, d.msg, ws.P, hE, E_idx, mask, T, ws.Ssum, ws.cnt, st));
    return launch_node_update(w->mode, d.node, hV_in, ws.Ssum, ws.cnt, mask, T, hV_out, next, nullptr, st, head, head_ran);
}

// k-NN graph, edge features and the three encoder layers of a ragged batch: the part of a forward that never reads the sequence.
// The k-NN kernel writes the zero node state (:1228) and its message projection [b1 | 0] as it goes and zeroes the status word (no
// memset launch: hipMemsetAsync of 4 bytes is a 5.4 us fill kernel in front of a 180 us single-protein forward); node_update of every
// layer writes the projection the next message pass needs into ws.P — 18 launches per forward (28 when every projection and the zero
// state are launches of their own). The last node update writes decoder layer 0's projection into P_dec0:
//   S != nullptr (tmpnn_ssm_forward): with the sequence term, and small launches run the last edge update and decoder message pass 0
//                as one launch (*dec_msg0_done; P_dec0 must be ws.P);
//   S == nullptr (tmpnn_encode): without it, and the last edge update runs alone — same kernels, same bits in h_E and h_V.
static int run_encoder(const tmpnn_weights *w, const float *X, const float *mask, const int32_t *residue_idx, const int32_t *chain_enc,
                       const int32_t *offsets, int n_proteins, int64_t T, int max_len, int K, const LayerWs &ws, int32_t *E_idx,
                       float *D_nb, float *hE, float *hV, const int32_t *S, float *P_dec0, int32_t *status_opt, bool *dec_msg0_done,
                       hipStream_t st) {
    static const bool fuse_small = TM_DBG_FLAG("TMPNN_FUSE_SMALL", true);     // (A/B switch in the debug library only)
    const KnnInit kinit{hV, ws.P, w->enc[0].msg_proj.spec.ba, status_opt};
    if (w->ca) {
        // A CA handle: k-NN (the same kernel: _dist reads the C-alpha atoms in both flavours), the frame pre-pass, the CA edge kernel —
        // at every launch size (the k-NN-inside-the-featurizer form is full-backbone only). The frames O [T,9]: ws.ca_frames (layer_ws).
        TRY(launch_knn(X, mask, offsets, n_proteins, T, max_len, K, E_idx, D_nb, nullptr, st, kinit));
        TRY(launch_ca_frames(X, offsets, n_proteins, T, ws.ca_frames, st));
        TRY(launch_featurize_ca(w, X, ws.ca_frames, offsets, n_proteins, residue_idx, chain_enc, E_idx, D_nb, T, hE, nullptr, st));
    } else if (fuse_small && max_len <= 256 && featurize_fusable(w->mode, T)) {             // one tile per workgroup: k-NN inside the featurizer launch
        const KnnFuse kf{mask, offsets, n_proteins, max_len, K, E_idx, D_nb, kinit};
        TRY(launch_featurize(w, X, residue_idx, chain_enc, E_idx, D_nb, T, hE, nullptr, st, &kf));
    } else {
        TRY(launch_knn(X, mask, offsets, n_proteins, T, max_len, K, E_idx, D_nb, nullptr, st, kinit));
        TRY(launch_featurize(w, X, residue_idx, chain_enc, E_idx, D_nb, T, hE, nullptr, st));
    }
    // One tile per workgroup (a single protein, a few short ones): the edge update of encoder layer l and the message pass of
    // the layer after it are ONE launch (edge_msg_fused_kernel: no grid-wide dependency between them; 16 launches instead
    // of 19, bit-identical results). Launch order: msg0, node0, [edge0 + msg1], node1, [edge1 + msg2], node2,
    // [edge2 + dec msg0], dnode0, dmsg1, dnode1, dmsg2, dnode2. Larger launches: msg, node, edge per layer.
    const bool fused = fuse_small && edge_msg_fusable(w->mode, T);
    *dec_msg0_done = fused && S;
    for (int l = 0; l < 3; ++l) {
        const NodeProj next = l < 2 ? enc_msg_proj(w, l + 1, ws.P) : dec_msg_proj(w, 0, P_dec0, S);
        const MsgW *then = !fused ? nullptr : l < 2 ? &w->enc[l + 1].msg : S ? &w->dec[0].msg : nullptr;
        TRY(run_enc_layer(w, l, hV, hE, E_idx, mask, T, ws, true, fused && l > 0, &next, then, st));
    }
    return TMPNN_OK;
}

// ---- entry points ---------------------------------------------------------------------------------
extern "C" int tmpnn_knn_topk(const float *X, const float *mask, const int32_t *offsets, int n_proteins, int64_t T,
                              int max_len, int K, int32_t *E_idx, float *D_nb, int32_t *status_opt, tmpnn_stream_t stream) {
    REQUIRE(X && mask && offsets && E_idx && D_nb, "knn_topk: null pointer");
    REQUIRE(n_proteins >= 0 && T >= 0 && T <= T_MAX, "knn_topk: bad sizes (N=%d, T=%lld)", n_proteins, (long long)T);
    REQUIRE(K >= 1 && K <= TMPNN_KS, "knn_topk: K=%d outside [1, %d]", K, TMPNN_KS);
    if (T == 0 || n_proteins == 0) return TMPNN_OK;
    REQUIRE(max_len >= 1, "knn_topk: max_len must be >= 1");
    if (max_len > 8192) return tm_set_error(TMPNN_E_UNSUPPORTED, "knn_topk: max_len %d > 8192", max_len);
    return launch_knn(X, mask, offsets, n_proteins, T, max_len, K, E_idx, D_nb, status_opt, (hipStream_t)stream);
}

extern "C" int tmpnn_centrality(const float *X, const float *mask, const int32_t *offsets, int n_proteins, int64_t T,
                                float radius, int32_t *out, tmpnn_stream_t stream) {
    REQUIRE(n_proteins >= 0 && T >= 0 && T <= T_MAX && radius > 0.f, "centrality: bad argument");
    if (T == 0 || n_proteins == 0) return TMPNN_OK;
    REQUIRE(X && mask && offsets && out, "centrality: null pointer");
    return launch_centrality(X, mask, offsets, n_proteins, T, radius, out, (hipStream_t)stream);
}

extern "C" int tmpnn_edge_featurize(const tmpnn_weights_t *w, const float *X, const int32_t *residue_idx,
                                    const int32_t *chain_enc, const int32_t *E_idx, const float *D_nb, int64_t T,
                                    float *h_E, float *E_opt, tmpnn_stream_t stream) {
    REQUIRE(w && X && residue_idx && chain_enc && E_idx && D_nb && h_E, "edge_featurize: null pointer");
    REQUIRE(T >= 0 && T <= T_MAX, "edge_featurize: bad T");
    REQUIRE(!w->ca, "edge_featurize: a CA handle needs the proteins' offsets and the frames: tmpnn_ca_frames + tmpnn_edge_featurize_ca");
    if (T == 0) return TMPNN_OK;
    return launch_featurize(w, X, residue_idx, chain_enc, E_idx, D_nb, T, h_E, E_opt, (hipStream_t)stream);
}

extern "C" int tmpnn_ca_frames(const float *X, const int32_t *offsets, int n_proteins, int64_t T, float *O, tmpnn_stream_t stream) {
    REQUIRE(n_proteins >= 0 && T >= 0 && T <= T_MAX, "ca_frames: bad sizes (N=%d, T=%lld)", n_proteins, (long long)T);
    if (T == 0 || n_proteins == 0) return TMPNN_OK;
    REQUIRE(X && offsets && O, "ca_frames: null pointer");
    return launch_ca_frames(X, offsets, n_proteins, T, O, (hipStream_t)stream);
}

extern "C" int tmpnn_edge_featurize_ca(const tmpnn_weights_t *w, const float *X, const int32_t *residue_idx, const int32_t *chain_enc,
                                       const int32_t *offsets, int n_proteins, const int32_t *E_idx, const float *D_nb, const float *O,
                                       int64_t T, float *h_E, float *E_opt, tmpnn_stream_t stream) {
    REQUIRE(w && X && residue_idx && chain_enc && offsets && E_idx && D_nb && O && h_E, "edge_featurize_ca: null pointer");
    REQUIRE(w->ca, "edge_featurize_ca: the handle is not a CA handle (tmpnn_weights_create_ca)");
    REQUIRE(n_proteins >= 0 && T >= 0 && T <= T_MAX, "edge_featurize_ca: bad sizes");
    if (T == 0 || n_proteins == 0) return TMPNN_OK;
    return launch_featurize_ca(w, X, O, offsets, n_proteins, residue_idx, chain_enc, E_idx, D_nb, T, h_E, E_opt, (hipStream_t)stream);
}

extern "C" int tmpnn_gather_nodes(const float *nodes, const int64_t *neighbor_idx, int B, int N, int K, int C, float *out,
                                  tmpnn_stream_t stream) {
    REQUIRE(B >= 0 && N >= 0 && K >= 0 && C >= 1, "gather_nodes: bad shape");
    if ((int64_t)B * N * K == 0) return TMPNN_OK;
    REQUIRE(nodes && neighbor_idx && out, "gather_nodes: null pointer");
    return launch_gather_rows(nodes, neighbor_idx, 1, (int64_t)B * N * K, (int64_t)N * K, N, C, out, (hipStream_t)stream);
}

extern "C" int tmpnn_gather_rows_i32(const float *nodes, const int32_t *idx, int64_t n_rows, int C, float *out,
                                     tmpnn_stream_t stream) {
    REQUIRE(n_rows >= 0 && C >= 1, "gather_rows_i32: bad shape");
    if (n_rows == 0) return TMPNN_OK;
    REQUIRE(nodes && idx && out, "gather_rows_i32: null pointer");
    return launch_gather_rows(nodes, idx, 0, n_rows, 0, 0, C, out, (hipStream_t)stream);
}

extern "C" int tmpnn_gather_edges(const float *edges, const int64_t *neighbor_idx, int B, int N, int K, int C, float *out,
                                  tmpnn_stream_t stream) {
    REQUIRE(B >= 0 && N >= 0 && K >= 0 && C >= 1, "gather_edges: bad shape");
    if ((int64_t)B * N * K == 0) return TMPNN_OK;
    REQUIRE(edges && neighbor_idx && out, "gather_edges: null pointer");
    return launch_gather_edges(edges, neighbor_idx, B, N, K, C, out, (hipStream_t)stream);
}

extern "C" int tmpnn_enc_layer(const tmpnn_weights_t *w, int layer, float *h_V, float *h_E, const int32_t *E_idx,
                               const float *mask, int64_t T, void *workspace, size_t workspace_bytes,
                               tmpnn_stream_t stream) {
    REQUIRE(w && h_V && h_E && E_idx && mask, "enc_layer: null pointer");
    REQUIRE(layer >= 0 && layer < 3, "enc_layer: layer %d outside [0,3)", layer);
    REQUIRE(T >= 0 && T <= T_MAX, "enc_layer: bad T");
    if (T == 0) return TMPNN_OK;
    LayerWs ws;
    TRY(carve_layer_ws(workspace, workspace_bytes, T, &ws));
    return run_enc_layer(w, layer, h_V, h_E, E_idx, mask, T, ws, false, false, nullptr, nullptr, (hipStream_t)stream);
}

// measurement hook (tools/gemm_probe.py): one [48x128] x [128x128]^T GEMM per tile, mode 0 = fp32 MFMA, 1 = bf16x3 six-term, 2 = f16x2 three-term
extern "C" int tmpnn_gemm_probe(int mode, const float *X, const float *W, float *Y, int64_t T, int reps, tmpnn_stream_t stream) {
    REQUIRE(X && W && Y && T > 0 && reps > 0 && mode >= 0 && mode <= 2, "gemm_probe: bad argument");
    return launch_gemm_probe(mode, X, W, Y, T, reps, (hipStream_t)stream);
}

// measurement hook: effective shader clock under a saturated fp32-MFMA load; out[2b] = shader cycles, out[2b+1] = 100 MHz ticks
extern "C" int tmpnn_clock_probe(int blocks, int iters, uint64_t *out, float *sink, tmpnn_stream_t stream) {
    REQUIRE(blocks > 0 && iters > 0 && out && sink, "clock_probe: bad argument");
    return launch_clock_probe(blocks, iters, (unsigned long long *)out, sink, (hipStream_t)stream);
}

// measurement hook: the clock the chip keeps under whatever runs beside it (one sleeping wavefront on `stream`): out[0] = shader cycles,
// out[1] = 100 MHz ticks over iters x s_sleep 127 (~8 100 cycles each)
extern "C" int tmpnn_clock_monitor(int iters, uint64_t *out, tmpnn_stream_t stream) {
    REQUIRE(iters > 0 && out, "clock_monitor: bad argument");
    return launch_clock_monitor(iters, (unsigned long long *)out, (hipStream_t)stream);
}

// measurement hook: n dependent launches of a kernel that does (almost) nothing — the box's own price of a kernel boundary, to set
// beside the end-to-start gaps of the real 19-launch forward (tools/gap_probe.py). dirty_floats > 0: every launch also writes that
// many floats of `buf` (dirty lines for the boundary's write-back); lds_bytes: dynamic LDS per workgroup (residency as the real kernels).
__global__ void launch_probe_kernel(float *buf, int dirty_floats, int k) {
    extern __shared__ float probe_lds[];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < dirty_floats; i += gridDim.x * blockDim.x) buf[i] = (float)k;
    if (dirty_floats < 0) probe_lds[threadIdx.x] = 0.f;
}
extern "C" int tmpnn_launch_probe(int n, int grid, int block, int lds_bytes, float *buf, int dirty_floats, tmpnn_stream_t stream) {
    REQUIRE(n > 0 && grid > 0 && block > 0 && block <= 1024 && lds_bytes >= 0 && lds_bytes <= 160 * 1024, "launch_probe: bad argument");
    REQUIRE(dirty_floats <= 0 || buf, "launch_probe: dirty_floats without a buffer");
    if (lds_bytes > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(launch_probe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (int k = 0; k < n; ++k) launch_probe_kernel<<<grid, block, lds_bytes, (hipStream_t)stream>>>(buf, dirty_floats, k);
    return tm_check_launch("launch_probe");
}

extern "C" int tmpnn_dec_layer(const tmpnn_weights_t *w, int layer, const float *h_V_in, float *h_V_out, const float *h_E,
                               const int32_t *E_idx, const int32_t *S, const float *mask, int64_t T, void *workspace,
                               size_t workspace_bytes, tmpnn_stream_t stream) {
    REQUIRE(w && h_V_in && h_V_out && h_E && E_idx && S && mask, "dec_layer: null pointer");
    REQUIRE(layer >= 0 && layer < 3, "dec_layer: layer %d outside [0,3)", layer);
    REQUIRE(T >= 0 && T <= T_MAX, "dec_layer: bad T");
    if (T == 0) return TMPNN_OK;
    LayerWs ws;
    TRY(carve_layer_ws(workspace, workspace_bytes, T, &ws));
    return run_dec_layer(w, layer, h_V_in, h_V_out, h_E, E_idx, S, mask, T, ws, false, false, nullptr, (hipStream_t)stream);
}

extern "C" int tmpnn_seq_embed(const tmpnn_weights_t *w, const int32_t *S, int64_t T, float *h_S, tmpnn_stream_t stream) {
    REQUIRE(w && S && h_S && T >= 0, "seq_embed: bad argument");
    if (T == 0) return TMPNN_OK;
    return launch_seq_embed(w, S, T, h_S, (hipStream_t)stream);
}

extern "C" int tmpnn_log_probs(const tmpnn_weights_t *w, const float *h_V, int64_t T, float *log_probs,
                               int32_t *status_opt, tmpnn_stream_t stream) {
    REQUIRE(w && h_V && log_probs && T >= 0 && T <= T_MAX, "log_probs: bad argument");
    if (T == 0) return TMPNN_OK;
    return launch_log_probs(w, h_V, T, log_probs, status_opt, (hipStream_t)stream);
}

extern "C" int tmpnn_ddg_head(const tmpnn_weights_t *w, const float *hV_last, const float *hV_prev, const int32_t *S,
                              int64_t T, float *ddg, float *z_opt, int32_t *status_opt, tmpnn_stream_t stream) {
    REQUIRE(w && hV_last && hV_prev && S && ddg && T >= 0 && T <= T_MAX, "ddg_head: bad argument");
    REQUIRE(w->n_tensors == TMPNN_N_TENSORS, "ddg_head: weight handle was created without the TransferModel head tensors");
    if (T == 0) return TMPNN_OK;
    return launch_head(w, hV_last, hV_prev, S, T, ddg, z_opt, status_opt, (hipStream_t)stream);
}

// ---- generic head ----------------------------------------------------------------------------------
static int head_generic_dims_ok(int n_final, int n_layers, const int32_t *dims) {
    if (n_final < 0 || n_final > 3 || n_layers < 1 || n_layers > 8 || !dims) return 0;
    if (dims[0] != TMPNN_HID * n_final + TMPNN_HID || dims[n_layers] != TMPNN_VOCAB) return 0;
    for (int l = 1; l < n_layers; ++l)
        if (dims[l] < 1 || dims[l] > 4096) return 0;
    return 1;
}

struct HeadWs { float *buf0, *buf1; size_t bytes; };          // two [T, widest layer] activations, ping-pong
static HeadWs head_ws(Carver c, int64_t T, int n_layers, const int32_t *dims) {
    int widest = dims[0];
    for (int l = 1; l <= n_layers; ++l) widest = dims[l] > widest ? dims[l] : widest;
    return HeadWs{c.take<float>((size_t)T * widest), c.take<float>((size_t)T * widest), c.used};
}
extern "C" size_t tmpnn_head_generic_workspace_bytes(int64_t T, int n_final, int n_layers, const int32_t *dims) {
    if (T < 0 || !head_generic_dims_ok(n_final, n_layers, dims)) return 0;
    return head_ws(Carver(), T, n_layers, dims).bytes;        // no slack: the entry uses the caller's base as it is
}

extern "C" int tmpnn_ddg_head_generic(const float *const *hidden, int n_final, const float *Ws, const int32_t *S, int64_t T,
                                      const float *conv_w, const float *conv_b, int n_layers, const float *const *mlp_w,
                                      const float *const *mlp_b, const int32_t *dims, const float *ddg_w, const float *ddg_b,
                                      float *ddg, float *z_opt, void *workspace, size_t workspace_bytes, int32_t *status_opt,
                                      tmpnn_stream_t stream) {
    REQUIRE(head_generic_dims_ok(n_final, n_layers, dims),
            "ddg_head_generic: dims must run from 128 * num_final_layers + 128 to 21 over 1..8 layers (num_final_layers 0..3)");
    REQUIRE(Ws && S && mlp_w && mlp_b && ddg_w && ddg_b && ddg && (n_final == 0 || hidden), "ddg_head_generic: null pointer");
    for (int i = 0; i < n_final; ++i) REQUIRE(hidden[i], "ddg_head_generic: hidden[%d] is null", i);
    for (int l = 0; l < n_layers; ++l) REQUIRE(mlp_w[l] && mlp_b[l], "ddg_head_generic: layer %d has a null weight / bias", l);
    REQUIRE((conv_w == nullptr) == (conv_b == nullptr), "ddg_head_generic: conv weight and bias go together");
    REQUIRE(T >= 0 && T <= T_MAX, "ddg_head_generic: bad T");
    if (T == 0) return TMPNN_OK;
    const size_t need = tmpnn_head_generic_workspace_bytes(T, n_final, n_layers, dims);
    if (!workspace || workspace_bytes < need)
        return tm_set_error(TMPNN_E_WORKSPACE, "ddg_head_generic: workspace %zu < %zu bytes", workspace_bytes, need);
    const HeadWs h = head_ws(Carver(workspace, false), T, n_layers, dims);
    return launch_head_generic(hidden, n_final, Ws, S, T, conv_w, conv_b, n_layers, mlp_w, mlp_b, dims, ddg_w, ddg_b, ddg, z_opt,
                               h.buf0, h.buf1, status_opt, (hipStream_t)stream);
}

extern "C" int tmpnn_ssm_forward(const tmpnn_weights_t *w, const float *X, const int32_t *S, const float *mask,
                                 const int32_t *residue_idx, const int32_t *chain_enc, const int32_t *offsets,
                                 int n_proteins, int64_t T, int max_len, int K, float *ddg, float *hidden_opt,
                                 float *log_probs_opt, int32_t *E_idx_opt, int32_t *status_opt, void *workspace,
                                 size_t workspace_bytes, tmpnn_stream_t stream) {
    REQUIRE(w, "ssm_forward: null weight handle");
    REQUIRE(n_proteins >= 0 && T >= 0 && T <= T_MAX, "ssm_forward: bad sizes");
    REQUIRE(K >= 1 && K <= TMPNN_KS, "ssm_forward: K=%d outside [1, %d]", K, TMPNN_KS);
    REQUIRE(!ddg || !w->ca, "ssm_forward: ddg requested with a CA handle (ThermoMPNN has no CA flavour)");
    REQUIRE(!ddg || w->n_tensors == TMPNN_N_TENSORS, "ssm_forward: ddg requested but the handle has no head tensors");
    if (T == 0 || n_proteins == 0) return TMPNN_OK;   // an empty batch is a no-op (pointers may be null)
    REQUIRE(X && S && mask && residue_idx && chain_enc && offsets, "ssm_forward: null input pointer");
    REQUIRE(ddg || hidden_opt || log_probs_opt, "ssm_forward: no output requested");
    REQUIRE(max_len >= 1, "ssm_forward: max_len must be >= 1 (the longest protein of the batch)");
    if (max_len > 8192) return tm_set_error(TMPNN_E_UNSUPPORTED, "ssm_forward: max_len %d > 8192", max_len);
    hipStream_t st = (hipStream_t)stream;
    // (status_opt: the k-NN kernel zeroes the word, and the LAST kernel flags what the k-NN kernel found, see KnnInit / HeadArgs)

    FwdWs f = fwd_ws(Carver(workspace, true), T);
    TRY(layer_ws_fits(workspace, workspace_bytes, f.l, T));
    if (f.bytes > workspace_bytes)
        return tm_set_error(TMPNN_E_WORKSPACE, "ssm_forward: workspace %zu < %zu bytes", workspace_bytes, tmpnn_workspace_bytes(T));
    if (E_idx_opt) f.E_idx = E_idx_opt;
    if (hidden_opt) for (int l = 0; l < 3; ++l) f.hV[1 + l] = hidden_opt + (size_t)l * T * TMPNN_HID;
    const LayerWs &ws = f.l;
    int32_t *const E_idx = f.E_idx;
    float *const *hV = f.hV;

    bool dec_msg0_done = false;      // small launches: decoder message pass 0 ran inside the last edge update's launch
    bool head_done = false;          // the ddG head ran inside the last node update's launch
    TRY(run_encoder(w, X, mask, residue_idx, chain_enc, offsets, n_proteins, T, max_len, K, ws, E_idx, f.D_nb, f.hE, hV[0], S, ws.P,
                    status_opt, &dec_msg0_done, st));
    for (int l = 0; l < 3; ++l) {
        const NodeProj next = dec_msg_proj(w, l < 2 ? l + 1 : 2, ws.P, S);
        // last layer of a small launch: its node update and the ddG head of the same 16 residues are ONE launch (node_head_fused_kernel, bit-identical)
        HeadArgs ha;
        const bool with_head = dec_msg0_done && l == 2 && ddg && node_head_fusable(w->mode, T);
        if (with_head) TRY(tm_head_args(ha, w, hV[3], hV[2], S, T, ddg, nullptr, status_opt, E_idx));
        TRY(run_dec_layer(w, l, hV[l], hV[l + 1], f.hE, E_idx, S, mask, T, ws, true, dec_msg0_done && l == 0, l < 2 ? &next : nullptr, st,
                          with_head ? &ha : nullptr, with_head ? &head_done : nullptr));
    }
    if (ddg && !head_done) TRY(launch_head(w, hV[3], hV[2], S, T, ddg, nullptr, status_opt, st, E_idx));
    if (log_probs_opt) TRY(launch_log_probs(w, hV[3], T, log_probs_opt, status_opt, st, ddg ? nullptr : E_idx));
    // hidden states only: neither of the kernels above has looked at the last decoder state (a poisoned value anywhere upstream
    // has reached it through its neighbours by now)
    if (!ddg && !log_probs_opt && hidden_opt) TRY(launch_range_check(hV[3], T * TMPNN_HID, status_opt, st, E_idx, T));
    return TMPNN_OK;
}

// ---- many sequence variants over one encoded backbone ------------------------------------------------
// The encoded backbone in the caller's ctx buffer: what the decoder reads and no sequence changes.
struct EncCtx { int32_t *E_idx; float *hE, *hV, *P0; size_t bytes; };      // [T,48], [T,48,128], [T,128], [T,256] (decoder layer 0's projection, no sequence term)

static EncCtx enc_ctx(Carver c, int64_t T) {               // (this order is the ctx's format: EncodedBackbone reads E_idx at offset 0)
    const size_t n = (size_t)T;
    return EncCtx{c.take<int32_t>(n * TMPNN_KS), c.take<float>(n * TMPNN_KS * TMPNN_HID), c.take<float>(n * TMPNN_HID), c.take<float>(n * 256),
                  c.used};
}
extern "C" size_t tmpnn_encode_bytes(int64_t T) { return T < 0 ? 0 : enc_ctx(Carver(), T).bytes; }     // no slack: a ctx is aligned
extern "C" size_t tmpnn_encode_workspace_bytes(int64_t T) { return T < 0 ? 0 : enc_ws(Carver(), T).bytes + 256; }

static int carve_ctx(const char *what, void *ctx, size_t ctx_bytes, int64_t T, EncCtx *c) {
    if (!ctx || ((uintptr_t)ctx & 255) != 0) return tm_set_error(TMPNN_E_INVALID, "%s: ctx is null or not 256-byte aligned", what);
    if (ctx_bytes < tmpnn_encode_bytes(T))
        return tm_set_error(TMPNN_E_WORKSPACE, "%s: ctx %zu < %zu bytes", what, ctx_bytes, tmpnn_encode_bytes(T));
    *c = enc_ctx(Carver(ctx, false), T);
    return TMPNN_OK;
}

extern "C" int tmpnn_encode(const tmpnn_weights_t *w, const float *X, const float *mask, const int32_t *residue_idx,
                            const int32_t *chain_enc, const int32_t *offsets, int n_proteins, int64_t T, int max_len, int K,
                            void *ctx, size_t ctx_bytes, int32_t *status_opt, void *workspace, size_t workspace_bytes,
                            tmpnn_stream_t stream) {
    REQUIRE(w, "encode: null weight handle");
    REQUIRE(n_proteins >= 0 && T >= 0 && T <= T_MAX, "encode: bad sizes");
    REQUIRE(K >= 1 && K <= TMPNN_KS, "encode: K=%d outside [1, %d]", K, TMPNN_KS);
    if (T == 0 || n_proteins == 0) return TMPNN_OK;
    REQUIRE(X && mask && residue_idx && chain_enc && offsets, "encode: null input pointer");
    REQUIRE(max_len >= 1, "encode: max_len must be >= 1 (the longest protein of the batch)");
    if (max_len > 8192) return tm_set_error(TMPNN_E_UNSUPPORTED, "encode: max_len %d > 8192", max_len);
    EncCtx c;
    TRY(carve_ctx("encode", ctx, ctx_bytes, T, &c));
    const EncWs e = enc_ws(Carver(workspace, true), T);
    TRY(layer_ws_fits(workspace, workspace_bytes, e.l, T));
    if (e.bytes > workspace_bytes)
        return tm_set_error(TMPNN_E_WORKSPACE, "encode: workspace %zu < %zu bytes", workspace_bytes, tmpnn_encode_workspace_bytes(T));
    hipStream_t st = (hipStream_t)stream;
    bool unused = false;
    TRY(run_encoder(w, X, mask, residue_idx, chain_enc, offsets, n_proteins, T, max_len, K, e.l, c.E_idx, e.D_nb, c.hE, c.hV, nullptr,
                    c.P0, status_opt, &unused, st));
    // the encoder state is this call's output: a value that left the f16x2 range upstream has reached it, and rows of an over-long
    // protein have an empty neighbour list (the MAXLEN probe of the fused forward's last kernel)
    return launch_range_check(c.hV, T * TMPNN_HID, status_opt, st, c.E_idx, T);
}

// ---- order-masked decoding over one encoded backbone --------------------------------------------------
// (V + 1) T rows of 256 floats are addressed with 32-bit offsets inside the order-masked message kernel
static const int64_t ORD_ROWS_MAX = ((int64_t)1 << 24) - 1;

// Rows r = v T + t. Ordered: P is [V + 1, T, 256] (slot V = Penc_l), and the visibility words and the fp32 form's remapped list exist.
struct DecWs { float *P, *Ssum, *cnt, *mask_rep, *hV[4]; uint64_t *vis; int32_t *remap; size_t bytes; };
static DecWs dec_ws(Carver c, int64_t T, int64_t V, bool ordered) {
    const size_t R = (size_t)T * (size_t)V, rh = R * TMPNN_HID;
    return DecWs{c.take<float>((R + (ordered ? (size_t)T : 0)) * 256), c.take<float>(rh), c.take<float>(R), c.take<float>(R),
                 {c.take<float>(rh), c.take<float>(rh), c.take<float>(rh), c.take<float>(rh)},
                 ordered ? c.take<uint64_t>(R) : nullptr, ordered ? c.take<int32_t>((size_t)T * TMPNN_KS) : nullptr, c.used};
}
static size_t dec_ws_bytes(int64_t T, int64_t V, bool ordered) { return dec_ws(Carver(), T, V, ordered).bytes + 256; }
extern "C" size_t tmpnn_decode_variants_workspace_bytes(int64_t T, int64_t V) {
    if (T < 0 || V < 0 || (V > 0 && T > T_MAX / V)) return 0;
    return dec_ws_bytes(T, V, false);
}
extern "C" size_t tmpnn_decode_ordered_workspace_bytes(int64_t T, int64_t V) {
    if (T < 0 || V < 0 || (V > 0 && (T > T_MAX / V || T > ORD_ROWS_MAX / (V + 1)))) return 0;
    return dec_ws_bytes(T, V, true);
}

// The body of tmpnn_decode_variants (ordered == false, rank unused) and tmpnn_decode_ordered (`what` names the entry in messages).
// Rows r = v T + t. The row-wise kernels (node update + the next layer's projection, head, log-probabilities) run over all V T rows
// as they run over a ragged batch; the message pass shares the backbone's h_E tile between the variants of a workgroup. Ordered: the
// message pass of every layer picks each neighbour's row by rank — the variant's own projection (this layer's state + sequence term)
// for a neighbour decoded earlier, Penc_l (the encoder state's projection, no sequence) for the others.
static int decode_rows(const char *what, bool ordered, const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const int32_t *S_var,
                       const int32_t *rank, int64_t V, const float *mask, int64_t T, float *ddg, float *hidden_opt, float *log_probs_opt,
                       int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    REQUIRE(w, "%s: null weight handle", what);
    REQUIRE(T >= 0 && T <= T_MAX && V >= 0, "%s: bad sizes (T=%lld, V=%lld)", what, (long long)T, (long long)V);
    REQUIRE(!ddg || w->n_tensors == TMPNN_N_TENSORS, "%s: ddg requested but the handle has no head tensors", what);
    if (T == 0 || V == 0) return TMPNN_OK;            // nothing to decode (pointers may be null)
    if (T > T_MAX / V)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: V * T = %lld * %lld rows exceed %lld (decode the variants in chunks)", what,
                            (long long)V, (long long)T, (long long)T_MAX);
    if (ordered && T > ORD_ROWS_MAX / (V + 1))
        return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: (V + 1) * T = %lld * %lld rows exceed %lld (decode the variants in chunks)", what,
                            (long long)(V + 1), (long long)T, (long long)ORD_ROWS_MAX);
    REQUIRE(S_var && mask && (rank || !ordered), "%s: null input pointer", what);
    REQUIRE(ddg || hidden_opt || log_probs_opt, "%s: no output requested", what);
    EncCtx c;
    TRY(carve_ctx(what, const_cast<void *>(ctx), ctx_bytes, T, &c));
    const int64_t R = V * T;
    const size_t need = dec_ws_bytes(T, V, ordered);
    if (!workspace || workspace_bytes < need)
        return tm_set_error(TMPNN_E_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    const DecWs d = dec_ws(Carver(workspace, true), T, V, ordered);
    hipStream_t st = (hipStream_t)stream;
    float *const P = d.P, *const Ssum = d.Ssum, *const cnt = d.cnt, *const mask_rep = d.mask_rep, *const *hV = d.hV;
    float *Penc = P + (size_t)R * 256;
    TRY(launch_variant_expand(c.hV, c.P0, mask, w->seq_table[0], S_var, T, V, hV[0], P, mask_rep, status_opt, st));
    if (ordered) {
        TRY(launch_variant_penc0(c.P0, T, Penc, st));               // Penc_0 = P0 (its neighbour half is W1c_0 h_V_enc)
        TRY(launch_variant_vis(rank, c.E_idx, T, V, d.vis, st));
    }
    for (int l = 0; l < 3; ++l) {
        TRY(launch_variant_msg(w->mode, w->dec[l].msg, P, c.hE, c.E_idx, mask, T, V, Ssum, cnt, st, d.vis, d.remap));
        const NodeProj next = dec_msg_proj(w, l < 2 ? l + 1 : 2, P, S_var);
        TRY(launch_node_update(w->mode, w->dec[l].node, hV[l], Ssum, cnt, mask_rep, R, hV[l + 1], l < 2 ? &next : nullptr, nullptr, st));
        if (ordered && l < 2) {                       // T rows, not V T: the next layer's projection of the ENCODER state
            const NodeProj pe = dec_msg_proj(w, l + 1, Penc, nullptr);
            TRY(launch_node_proj(c.hV, pe, T, st));
        }
    }
    if (ddg) TRY(launch_head(w, hV[3], hV[2], S_var, R, ddg, nullptr, status_opt, st));
    if (log_probs_opt) TRY(launch_log_probs(w, hV[3], R, log_probs_opt, status_opt, st));
    if (!ddg && !log_probs_opt) TRY(launch_range_check(hV[3], R * TMPNN_HID, status_opt, st));
    if (hidden_opt) TRY(launch_variant_hidden(hV + 1, T, V, hidden_opt, st));
    return TMPNN_OK;
}

extern "C" int tmpnn_decode_variants(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const int32_t *S_var, int64_t V,
                                     const float *mask, int64_t T, float *ddg, float *hidden_opt, float *log_probs_opt,
                                     int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    return decode_rows("decode_variants", false, w, ctx, ctx_bytes, S_var, nullptr, V, mask, T, ddg, hidden_opt, log_probs_opt, status_opt,
                       workspace, workspace_bytes, stream);
}

extern "C" int tmpnn_decode_ordered(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const int32_t *S_var,
                                    const int32_t *rank, int64_t V, const float *mask, int64_t T, float *ddg, float *hidden_opt,
                                    float *log_probs_opt, int32_t *status_opt, void *workspace, size_t workspace_bytes,
                                    tmpnn_stream_t stream) {
    return decode_rows("decode_ordered", true, w, ctx, ctx_bytes, S_var, rank, V, mask, T, ddg, hidden_opt, log_probs_opt, status_opt,
                       workspace, workspace_bytes, stream);
}

// ---- autoregressive sampling over one encoded backbone -------------------------------------------------
// 3 N T table rows of 128 floats are addressed inside the chain kernel; bounded like ORD_ROWS_MAX bounds the ordered decode's table
static const int64_t SAMPLE_ROWS_MAX = ((int64_t)1 << 24) - 1;

struct SampleWs { float *Penc1, *Penc2, *tab; int32_t *rank; size_t bytes; };     // [T,256] x 2, [N,3,T,128], [N,T]
static SampleWs sample_ws(Carver c, int64_t T, int64_t N) {
    const size_t n = (size_t)T, R = n * (size_t)N;
    return SampleWs{c.take<float>(n * 256), c.take<float>(n * 256), c.take<float>(3 * R * TMPNN_HID), c.take<int32_t>(R), c.used};
}
extern "C" size_t tmpnn_sample_workspace_bytes(int64_t T, int64_t N) {
    if (T < 0 || N < 0 || T > T_MAX || (N > 0 && T > SAMPLE_ROWS_MAX / 3 / N)) return 0;
    return sample_ws(Carver(), T, N).bytes + 256;
}

// The body of tmpnn_sample (tied == null), tmpnn_sample_tied and their per-protein forms (`what` names the entry in messages): the
// same checks, workspace layout and encoder-state projections; the tied form's arrays travel to the chain kernel's second form.
// each != null (with P proteins): proteins [p0, p1) over the rows [row0, row0 + rows) of the batch — R below is the number of rows
// the scratch holds (T, or `rows`), and sample_ws is the one layout of all four entries.
static int sample_rows(const char *what, const SampleTied *tied, const SampleEach *each, int64_t P, const tmpnn_weights_t *w, const void *ctx,
                       size_t ctx_bytes, const float *mask, int64_t T, int64_t N, const int32_t *order, const int32_t *S_fixed,
                       const float *free_, const float *u, float inv_temperature, const float *bias_opt, const float *allowed_opt,
                       int32_t *S_out, float *probs_opt, int32_t *status_opt, void *workspace, size_t workspace_bytes,
                       tmpnn_stream_t stream) {
    REQUIRE(w, "%s: null weight handle", what);
    REQUIRE(T >= 0 && T <= T_MAX && N >= 0, "%s: bad sizes (T=%lld, N=%lld)", what, (long long)T, (long long)N);
    if (each) {
        REQUIRE(P >= 0 && each->p0 >= 0 && each->p0 <= each->p1 && each->p1 <= P, "%s: bad protein range (p0=%lld, p1=%lld, P=%lld)", what,
                (long long)each->p0, (long long)each->p1, (long long)P);
        REQUIRE(each->rows >= 0 && each->row0 >= 0 && each->rows <= T - each->row0, "%s: bad row range (row0=%lld, rows=%lld, T=%lld)", what,
                (long long)each->row0, (long long)each->rows, (long long)T);
    }
    const int64_t R = each ? each->rows : T, row0 = each ? each->row0 : 0;
    if (R == 0 || N == 0 || (each && each->p0 == each->p1)) return TMPNN_OK;      // nothing to sample (pointers may be null)
    if (R > SAMPLE_ROWS_MAX / 3 / N)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: 3 * N * %s = 3 * %lld * %lld rows exceed %lld (sample the chains in chunks)", what,
                            each ? "rows" : "T", (long long)N, (long long)R, (long long)SAMPLE_ROWS_MAX);
    if (each && (each->p1 - each->p0) > (int64_t)0x7fffffff / ((N + 15) / 16))
        return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: %lld proteins times %lld chain blocks exceed one grid (sample the proteins in chunks)",
                            what, (long long)(each->p1 - each->p0), (long long)((N + 15) / 16));
    REQUIRE(mask && order && S_fixed && free_ && u && S_out && (!tied || tied->close) && (!each || each->offsets), "%s: null input pointer",
            what);
    REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.0e38f, "%s: inv_temperature must be positive and finite", what);
    REQUIRE(!tied || (tied->pssm_mix != nullptr) == (tied->pssm_bias != nullptr), "%s: pssm_bias goes with pssm_mix (give both or neither)", what);
    EncCtx c;
    TRY(carve_ctx(what, const_cast<void *>(ctx), ctx_bytes, T, &c));
    const size_t need = tmpnn_sample_workspace_bytes(R, N);
    if (!workspace || workspace_bytes < need)
        return tm_set_error(TMPNN_E_WORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
    const SampleWs s = sample_ws(Carver(workspace, true), R, N);
    // (the handle is read only now: every check above works on the arguments alone)
    if (w->mode == TM_MM_FP32)
        return tm_set_error(TMPNN_E_UNSUPPORTED, "%s: the chain kernel has no fp32 form; create the handle with precision \"bf16x3\" (or \"f16x2\")", what);
    hipStream_t st = (hipStream_t)stream;
    if (status_opt && hipMemsetAsync(status_opt, 0, 4, st) != hipSuccess) return tm_check_launch("sample: status memset");
    // residue -> step, scattered from `order` by the chain kernel's prologue; "not decoded" everywhere else
    if (hipMemsetAsync(s.rank, 0x7f, (size_t)N * R * 4, st) != hipSuccess) return tm_check_launch("sample: rank memset");
    const float *hV = c.hV + (size_t)row0 * TMPNN_HID;
    {   // the later layers' projections of the ENCODER state (layer 0's is the ctx's P0), as the ordered decode makes them
        const NodeProj p1 = dec_msg_proj(w, 1, s.Penc1, nullptr), p2 = dec_msg_proj(w, 2, s.Penc2, nullptr);
        TRY(launch_node_proj(hV, p1, R, st));
        TRY(launch_node_proj(hV, p2, R, st));
    }
    const float *Penc[3] = {c.P0 + (size_t)row0 * 256, s.Penc1, s.Penc2};
    return launch_sample_chains(w, c.hE, c.E_idx, c.hV, c.P0, Penc, mask, T, N, order, S_fixed, free_, u, inv_temperature, bias_opt,
                                allowed_opt, S_out, probs_opt, status_opt, s.tab, s.rank, tied, each, st);
}

extern "C" int tmpnn_sample(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T, int64_t N,
                            const int32_t *order, const int32_t *S_fixed, const float *free_, const float *u, float inv_temperature,
                            const float *bias_opt, const float *allowed_opt, int32_t *S_out, float *probs_opt, int32_t *status_opt,
                            void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    return sample_rows("sample", nullptr, nullptr, 0, w, ctx, ctx_bytes, mask, T, N, order, S_fixed, free_, u, inv_temperature, bias_opt,
                       allowed_opt, S_out, probs_opt, status_opt, workspace, workspace_bytes, stream);
}

// The tied form has tmpnn_sample's workspace (one layout, sample_ws): a chain's group state lives in the chain kernel's LDS.
extern "C" size_t tmpnn_sample_tied_workspace_bytes(int64_t T, int64_t N) { return tmpnn_sample_workspace_bytes(T, N); }

extern "C" int tmpnn_sample_tied(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T, int64_t N,
                                 const int32_t *order, const int32_t *close, const int32_t *S_fixed, const float *free_, const float *u,
                                 float inv_temperature, const float *weight_opt, const float *bias_opt, const float *allowed_opt,
                                 const float *pssm_mix_opt, const float *pssm_bias_opt, const float *pssm_keep_opt, int32_t *S_out,
                                 float *probs_opt, int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    const SampleTied tied{close, weight_opt, pssm_mix_opt, pssm_bias_opt, pssm_keep_opt};
    return sample_rows("sample_tied", &tied, nullptr, 0, w, ctx, ctx_bytes, mask, T, N, order, S_fixed, free_, u, inv_temperature, bias_opt,
                       allowed_opt, S_out, probs_opt, status_opt, workspace, workspace_bytes, stream);
}

// ---- the same for every protein of a packed batch over its own steps ----------------------------------------------------------
// sample_ws again, with the range's rows where the whole-axis entries have T: the scratch is sized by the protein range.
extern "C" size_t tmpnn_sample_each_workspace_bytes(int64_t rows, int64_t N) { return tmpnn_sample_workspace_bytes(rows, N); }
extern "C" size_t tmpnn_sample_tied_each_workspace_bytes(int64_t rows, int64_t N) { return tmpnn_sample_workspace_bytes(rows, N); }

extern "C" int tmpnn_sample_each(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T,
                                 const int32_t *offsets, int64_t P, int64_t p0, int64_t p1, int64_t row0, int64_t rows,
                                 const int32_t *sched_opt, int64_t N, const int32_t *order, const int32_t *S_fixed, const float *free_,
                                 const float *u, float inv_temperature, const float *bias_opt, const float *allowed_opt, int32_t *S_out,
                                 float *probs_opt, int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    const SampleEach each{offsets, sched_opt, p0, p1, row0, rows};
    return sample_rows("sample_each", nullptr, &each, P, w, ctx, ctx_bytes, mask, T, N, order, S_fixed, free_, u, inv_temperature, bias_opt,
                       allowed_opt, S_out, probs_opt, status_opt, workspace, workspace_bytes, stream);
}

extern "C" int tmpnn_sample_tied_each(const tmpnn_weights_t *w, const void *ctx, size_t ctx_bytes, const float *mask, int64_t T,
                                      const int32_t *offsets, int64_t P, int64_t p0, int64_t p1, int64_t row0, int64_t rows,
                                      const int32_t *sched_opt, int64_t N, const int32_t *order, const int32_t *close,
                                      const int32_t *S_fixed, const float *free_, const float *u, float inv_temperature,
                                      const float *weight_opt, const float *bias_opt, const float *allowed_opt, const float *pssm_mix_opt,
                                      const float *pssm_bias_opt, const float *pssm_keep_opt, int32_t *S_out, float *probs_opt,
                                      int32_t *status_opt, void *workspace, size_t workspace_bytes, tmpnn_stream_t stream) {
    const SampleTied tied{close, weight_opt, pssm_mix_opt, pssm_bias_opt, pssm_keep_opt};
    const SampleEach each{offsets, sched_opt, p0, p1, row0, rows};
    return sample_rows("sample_tied_each", &tied, &each, P, w, ctx, ctx_bytes, mask, T, N, order, S_fixed, free_, u, inv_temperature,
                       bias_opt, allowed_opt, S_out, probs_opt, status_opt, workspace, workspace_bytes, stream);
}
