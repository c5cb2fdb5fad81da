// C ABI of liballophant_amx (see include/allophant_amx.h): model construction from a reference state_dict, inventory
// composition, and the forward pass orchestration (kernel sequence on one HIP stream).
#include "../../include/allophant_amx.h"
#include "../../include/allophant_amx_allophones.h"
#include "../../include/allophant_amx_beam.h"
#include "../../include/allophant_amx_beam_lm.h"
#include "../../include/allophant_amx_align.h"
#include "../../include/allophant_amx_align_graph.h"
#include "../../include/allophant_amx_score.h"
#include "../../include/allophant_amx_search.h"
#include "../../include/allophant_amx_variants.h"
#include "../../include/allophant_amx_restrict.h"
#include "../../include/allophant_amx_long.h"
#include "../../include/allophant_amx_resample.h"
#include "../../include/allophant_amx_edit.h"
#include "amx_common.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <cstdlib>
#include <string>
#include <vector>

using namespace amx;

namespace {

thread_local std::string g_create_error;

struct Layer {
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    void *wqkv, *wo, *w1, *w2;
    float *bqkv, *bo, *b1, *b2;
    float r_qkv = 1.f, r_o = 1.f, r_1 = 1.f, r_2 = 1.f;  // 1 / (power of two the packed planes were multiplied by)
    // pre-LN layers: the LayerNorm in front of QKV / FFN1 is folded into those products (GemmParams.row_coef): wqkv / w1 hold
    // gamma (.) W, bqkv / b1 hold d = W beta + b, and c = W gamma (row sums of the folded weights) is what the mean term multiplies
    float *c_qkv = nullptr, *c_1 = nullptr;
    // attention adapter (amx_config.adapter_attn_dim = A > 0, pre-LN layers; launch_adapter): W1 diag(gamma) [A, D] and
    // b1 + W1 beta [A] -- the adapter's LayerNorm folded in --, W2 transposed [A, D], b2 [D]; fp32
    float *ad_w1 = nullptr, *ad_b1 = nullptr, *ad_w2t = nullptr, *ad_b2 = nullptr;
};

// One GEMM (or GEMM pair for the composition head) of the hierarchical projection
struct HeadStep {
    std::vector<int> classes;   // classes computed by this step (stacked rows of W), evaluation order
    bool direct_output;         // A operand = final LayerNorm planes (single "OUTPUT" dependency)
    std::vector<ConcatPart> parts;  // otherwise: concatenation recipe (src pointers filled per forward)
    std::vector<int> part_dep;      // per part: class index (>=0) or output code (<0)
    int K, Kpad;                // input width
    void* W;                    // planes [rows, Kpad]
    float* bias;                // [rows]
    int rows;                   // sum of out_features
    bool composed;              // rows == embedding_size, followed by the composition product
    ConcatPart* parts_dev;
    std::vector<ConcatPart> parts_uploaded;  // what parts_dev currently holds (re-uploaded only when it changes)
    // time layer (ProjectingMultiheadAttention, acoustic_model.py:237-268): W / bias are its input_projection and the
    // step continues LayerNorm(+positions) -> in_proj -> key-masked attention over time -> out_proj
    int time_heads = 0;         // 0: plain linear classifier
    int Cpad = 0;               // rows rounded up to 8 (K of the in_proj / out_proj products)
    float *tl_g = nullptr, *tl_b = nullptr, *tl_bin = nullptr, *tl_bout = nullptr, *tl_pe = nullptr;
    void *tl_win = nullptr, *tl_wout = nullptr;
    float r_w = 1.f, r_tin = 1.f, r_tout = 1.f;  // reciprocal pack scales of W, tl_win, tl_wout
};

}  // namespace

struct amx_handle_s {
    int device = 0;
    amx_config cfg{};
    std::vector<amx_class_desc> classes;
    std::vector<int> order;
    int prec = AMX_PREC_F16X3, NT = 2;
    // two-plane modes: GEMM operands as interleaved planes (amx_common.h pidx(): hi and lo of 32 K elements share a 128-byte
    // line, which is what the ping-pong GEMM's whole-line operand DMA needs).  Needs 32-element row blocks: conv_dim and ffn
    // multiples of 32 (every wav2vec 2.0 shape); other shapes keep separate planes and run on the generic tile kernels.
    bool il = true;
    std::string err;
    std::vector<void*> allocs;
    int64_t weight_bytes = 0, ws_bytes = 0;

    // weights
    float *c0_w = nullptr, *c0_b = nullptr;
    Conv0Route c0{};             // the kernels of conv layer 0 (conv0_route, amx_common.h): fixed at amx_create
    double* c0_stats = nullptr;  // its CONV0_STATS_TABLE: fp64 mean / covariance of the rows [w_c, b_c]
    float c0_wscale = 1.f;       // matrix pipe: power of two its fp16 weight planes are built under
    // the variant of the wav2vec 2.0 encoder (amx_config ABI 4)
    bool gn = false;         // feat_extract_norm == "group": GroupNorm over time behind conv layer 0, no norm behind layers 1..
    bool stable = true;      // do_stable_layer_norm: pre-LN layers + final LayerNorm; false: post-LN layers
    bool masked = true;      // the model is called with the attention mask of the lengths; false: attention_mask=None
    int adapter = 0;         // width of the attention adapter behind every pre-LN layer (0: none; always 0 for post-LN layers)
    float* conv_b[AMX_MAX_CONV] = {};
    float* conv_g[AMX_MAX_CONV] = {};
    float* conv_be[AMX_MAX_CONV] = {};
    void* conv_w[AMX_MAX_CONV] = {};
    void* conv_w_tm[AMX_MAX_CONV] = {};  // the same weights in tap-minor K order (GemmParams.a_taps), for the row-complete kernel
    int conv_tm_slice = 0;               // channels per slice of that order (0: no such copy)
    // Range of the 16-bit planes: every weight tensor is packed times a power of two that puts its largest element into
    // [4096, 8192) (exact, so results do not change) and the product's epilogue multiplies by the reciprocal kept here.  An
    // fp16 lo plane only carries its 11 bits while it is a normal number (|w| >= 0.25) and the hi plane underflows below
    // 6e-5: with unscaled planes the accuracy of the split modes would depend on the magnitude of the checkpoint's weights.
    float conv_r[AMX_MAX_CONV] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    float fp_r = 1.f, pos_r = 1.f;
    std::vector<float> emb_host;  // composition embedding table (host copy: scale of a composed inventory matrix)
    int* nonfinite = nullptr;     // device counter of valid frames with non-finite logits in the last forward pass
    float *fp_g = nullptr, *fp_b = nullptr, *fp_bias = nullptr;
    void* fp_w = nullptr;
    void* pos_w = nullptr;
    float* pos_b = nullptr;
    std::vector<Layer> layers;
    float *fln_g = nullptr, *fln_b = nullptr;
    float *unit_g = nullptr, *zero_b = nullptr;  // [hidden] ones / zeros
    std::vector<HeadStep> steps;
    float* emb = nullptr;  // composition embedding table [rows, E]
    int emb_rows = 0;
    int composed_class = -1;
    std::vector<bool> need_hidden;

    // inventories: every distinct `target_feature_indices` matrix seen gets its own composed phoneme matrix and its own
    // device output tables, so switching between them (the per-language loop of run.py:742-753) neither recomputes nor
    // overwrites anything a forward pass still in flight may be reading.  Models without a composition layer own one
    // implicit entry (P1 = 0).
    struct Inventory {
        std::vector<int64_t> key;  // phones, features, tfi..., offsets...
        int P1 = 0;                // phones + blank
        float r_composed = 1.f;    // reciprocal pack scale of composed_w
        void* composed_w = nullptr;
        float* composed_f32 = nullptr;
        int64_t* idx_dev = nullptr;
        OutDesc *out_unique_dev = nullptr, *out_all_dev = nullptr;
        uint64_t last_use = 0;
        uint64_t generation = 0;   // unique per install: a cached layout of an evicted entry never matches its successor
    };
    static constexpr int INV_CAP = 16;
    std::vector<Inventory> inventories;
    int inv = -1;  // current entry (cur_inv), -1 = composition model without an inventory yet
    uint64_t inv_clock = 0;

    // logits layout
    std::vector<int> col, width;  // per class
    int ld_logits = 0;
    std::vector<amx_output_desc> outputs;  // relative to N, T of the last layout computation
    std::vector<OutDesc> out_unique, out_all;
    int layout_inv = -2;  // inventory slot the host-side layout was computed for ...
    uint64_t layout_gen = 0, inv_gen = 0;  // ... and the install generation of that slot: slots are reused after eviction
    int layout_N = -1;
    int64_t layout_T = -1;

    // workspace
    struct WS {
        void* p = nullptr;
        size_t bytes = 0;
    };
    std::map<std::string, WS> ws;
    // pinned host staging of the per-utterance lengths: a small ring of slots, each guarded by an event recorded behind
    // its H2D copies, so that a call never waits for the previous forward pass (the host keeps running ahead of the GPU)
    static constexpr int PIN_SLOTS = 4;
    int64_t* h_lengths_pinned[PIN_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int* h_frames_pinned[PIN_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int* h_rowoff_pinned[PIN_SLOTS] = {nullptr, nullptr, nullptr, nullptr};  // packed-row offsets of the utterances (N + 1)
    int* h_tiles_pinned[PIN_SLOTS] = {nullptr, nullptr, nullptr, nullptr};  // tile lists of the conv layers of a ragged batch
    size_t tiles_cap[PIN_SLOTS] = {0, 0, 0, 0};                                // capacity of each, in ints
    hipEvent_t pin_event[PIN_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    bool pin_busy[PIN_SLOTS] = {false, false, false, false};
    int pin_next = 0;
    int pinned_cap = 0;
    // per-kernel-class HIP event timing (AMX_FLAG_TIMING)
    struct Span { int cls; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
    bool timing = false;
    hipStream_t timing_stream = nullptr;
    // HIP graphs of whole forward passes (region "enqueue" of amx_forward: every memset, kernel and device copy of a pass;
    // the small pinned H2D uploads stay eager in front of it).  A pass is captured when the same key -- buffers, geometry,
    // lengths, flags, inventory, workspace generation -- recurs among the last few passes, and replayed while it recurs: one
    // hipGraphLaunch instead of ~185 launches.  Cached LRU; dropped when a workspace buffer moves.
    struct GraphEntry {
        std::vector<int64_t> key;
        hipGraphExec_t exec = nullptr;
        hipGraph_t graph = nullptr;  // the template stays alive as long as its instance (destroyed together)
        uint64_t last_use = 0;
        hipStream_t last_stream = nullptr;  // where it was launched last: waited for before the instance is destroyed
    };
    static constexpr int GRAPH_CAP = 32;  // (a length-sorted corpus on a grid of batch geometries cycles through two dozen of them)
    std::vector<GraphEntry> graphs;
    std::vector<std::vector<int64_t>> graph_seen;  // keys of the last few eager passes (a caller that alternates between two
                                                   // output buffers -- an overlapped gather holds one -- repeats with period 2)
    static constexpr int GRAPH_SEEN = 8;
    hipStream_t capture_stream = nullptr;  // capture never runs on the caller's stream (which may be the null stream)
    bool graph_broken = false;             // a capture failed once: stay eager
    uint64_t ws_gen = 0, graph_clock = 0;
    int64_t graph_captures = 0, graph_replays = 0;
    // range report (AMX_ERANGE) without a host synchronisation: every pass copies its non-finite frame count into a pinned
    // slot behind itself; the NEXT amx_forward / amx_synchronize reads the slots whose event has completed
    struct RangeSlot {
        int* host = nullptr;
        hipEvent_t ev = nullptr;
        bool pending = false, cont = false;
        uint64_t pass_id = 0;  // which amx_forward of this handle the reading belongs to (amx_pass_info: AMX_PASS_INFO_ID)
    };
    static constexpr int RANGE_SLOTS = 8;
    RangeSlot range[RANGE_SLOTS];
    int range_next = 0;
    int64_t range_carry = 0;  // count of a slot that had to be reused before any call had read it
    std::string range_carry_ids;  // ... and the passes it belonged to
    uint64_t pass_counter = 0;    // passes issued so far (the id of the last one)
    // the slices of one over-long batch (AMX_FLAG_CONTINUE) share ONE running device counter: the reading of a slice includes its
    // predecessors'.  What the last poll saw of a chain whose later slices were not ready yet, so that the next poll counts the
    // difference only (round-5 advisor finding: a chain read across two polls used to be counted twice)
    int range_chain_seen = 0;
    bool range_chain_open = false;
    // last forward geometry
    int last_N = 0;
    bool last_fold = false;  // amx_pass_info: the last pass ran its encoder layers with the LayerNorm fold ...
    int last_packed = 0, last_graph = 0;  // ... on packed rows (1; 2: from the feature projection on); eager / recorded / replayed
    int last_attention = -1;              // ... with this form of the attention kernels (AttnForm; -1: an encoder without layers)
    int64_t last_rows = 0;
    bool qkv_dirty = false;
    // columns [dh, dhp) of the Q / K / V rows (head dimensions other than 64 and 128) may hold something else than zeros, anywhere in
    // the allocations: only amx_debug_scribble makes it so -- no pass writes them -- and the next pass zeroes the buffers whole
    bool qkv_pad_dirty = false;
    int64_t last_L = 0, last_T = 0;
    bool last_keep = false;
    // the last forward pass ran its heads on the packed rows of a ragged batch (packed_early): hidden states kept for
    // OUTPUT_i classifiers, the final hidden state and the logits hold sum(frames) rows, utterance n at last_rowoff[n]
    bool last_packed_rows = false;
    std::vector<int> last_rowoff, last_frames;
    // allophone layer (amx_set_allophones): per (language, q) column the unmasked entries (p, W[l, p, q]) of the reference's
    // matrices and the accumulator start (finfo.min if the column has a masked entry, else -inf); one device allocation
    int al_lang = 0, al_P1 = 0, al_Q1 = 0;
    void* al_buf = nullptr;
    size_t al_bytes = 0;
    int *al_col_ptr = nullptr, *al_ent_p = nullptr;
    float *al_ent_w = nullptr, *al_init = nullptr;
};

namespace {

#define HIPCHK(h, expr)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                           \
            return AMX_EHIP;                                                                        \
        }                                                                                           \
    } while (0)

int fail(amx_handle h, int code, const std::string& msg) {
    if (h) h->err = msg;
    g_create_error = msg;
    return code;
}

void* dev_alloc(amx_handle h, size_t bytes, bool weight = true) {
    void* p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    h->allocs.push_back(p);
    if (weight) h->weight_bytes += (int64_t)bytes;
    return p;
}

int ws_get(amx_handle h, const char* name, size_t bytes, void** out, bool zero_on_grow = false) {
    auto& w = h->ws[name];
    if (w.bytes < bytes) {
        if (w.p) {
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, hipFree(w.p));
            h->ws_bytes -= (int64_t)w.bytes;
            w.p = nullptr;
            w.bytes = 0;
        }
        // grow geometrically: a corpus of ragged batches would otherwise reallocate (and synchronise) every few calls
        size_t want = bytes + bytes / 4 + 256;
        if (hipMalloc(&w.p, want) != hipSuccess) return fail(h, AMX_ENOMEM, std::string("workspace allocation failed: ") + name);
        w.bytes = want;
        h->ws_bytes += (int64_t)want;
        ++h->ws_gen;  // a buffer moved: every captured graph holds stale pointers
        if (zero_on_grow) HIPCHK(h, hipMemset(w.p, 0, want));
    }
    *out = w.p;
    return AMX_OK;
}

int round_up(int x, int m) { return (x + m - 1) / m * m; }

// brackets one kernel launch with HIP events on the launch stream when timing is enabled
struct Timed {
    amx_handle h;
    hipEvent_t b = nullptr;
    Timed(amx_handle h_, int cls) : h(h_) {
        if (!h->timing) return;
        hipEvent_t a = nullptr;
        auto get = [&](hipEvent_t& e) {
            if (!h->event_pool.empty()) { e = h->event_pool.back(); h->event_pool.pop_back(); }
            else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        };
        get(a); get(b);
        if (!a || !b) { b = nullptr; return; }
        (void)hipEventRecord(a, h->timing_stream);
        h->spans.push_back({cls, a, b});
    }
    ~Timed() { if (b) (void)hipEventRecord(b, h->timing_stream); }
};
inline int gemm_class(int prec, const GemmParams& g) { return gemm_uses_pp(prec, g) ? AMX_KC_GEMM_PP : AMX_KC_GEMM_TILE; }

struct TensorMap {
    std::map<std::string, const amx_tensor*> m;
    const amx_tensor* get(const std::string& k) const {
        auto it = m.find(k);
        return it == m.end() ? nullptr : it->second;
    }
};

const std::string AM = "_acoustic_model._model.";
const std::string PROJ = "_projection._layers.";

// evaluation order of the classifier graph = order in which AttributeGraph.sort() yields nodes
// (reference attribute_graph.py:124-199): depth-first post-order, roots in index order, edges in listed order.
int evaluation_order(const std::vector<amx_class_desc>& cls, std::vector<int>& order, std::string& err) {
    int n = (int)cls.size();
    std::vector<int> state(n, 0);
    order.clear();
    for (int root = 0; root < n; ++root) {
        if (state[root]) continue;
        std::vector<std::pair<int, int>> stack;
        stack.push_back({root, 0});
        state[root] = 1;
        while (!stack.empty()) {
            auto [node, edge] = stack.back();
            stack.pop_back();
            std::vector<int> deps;
            for (int i = 0; i < cls[node].n_deps; ++i)
                if (cls[node].deps[i] >= 0) deps.push_back(cls[node].deps[i]);
            if (edge < (int)deps.size()) {
                stack.push_back({node, edge + 1});
                int t = deps[edge];
                if (t >= n) { err = "dependency index out of range"; return AMX_EINVAL; }
                if (state[t] == 1) { err = std::string("Dependency cycle detected at ") + cls[t].name; return AMX_EINVAL; }
                if (state[t] == 0) { state[t] = 1; stack.push_back({t, 0}); }
            } else {
                state[node] = 2;
                order.push_back(node);
            }
        }
    }
    return AMX_OK;
}

}  // namespace

static void free_inventory(amx_handle_s::Inventory& e);
static void drop_graphs(amx_handle h);
static int install_inventory(amx_handle h, std::vector<int64_t>&& key, const std::vector<int64_t>& idx, int P1, int features,
                             hipStream_t s);

// =================================================================================================================
// creation
// =================================================================================================================
#define TRY(x) do { if (int rc_ = (x)) return rc_; } while (0)

static int upload_f32(amx_handle h, const TensorMap& tm, const std::string& key, int64_t numel, float** out) {
    const amx_tensor* t = tm.get(key);
    if (!t) return fail(h, AMX_EINVAL, "missing tensor in state_dict: " + key);
    if (t->numel != numel)
        return fail(h, AMX_EINVAL, "tensor " + key + " has " + std::to_string(t->numel) + " elements, expected " + std::to_string(numel));
    float* d = (float*)dev_alloc(h, (size_t)numel * 4);
    if (!d) return fail(h, AMX_ENOMEM, "device allocation failed for " + key);
    HIPCHK(h, hipMemcpy(d, t->data, (size_t)numel * 4, hipMemcpyHostToDevice));
    *out = d;
    return AMX_OK;
}

// a weight buffer amx_create could not allocate or fill
static int alloc_failed(amx_handle h) { return fail(h, AMX_ENOMEM, "device allocation failed"); }

// a weight buffer of `bytes` holding a copy of host `src` (zeros when null)
template <class T>
static int dev_upload(amx_handle h, T** out, const void* src, size_t bytes) {
    *out = (T*)dev_alloc(h, bytes);
    if (!*out || (src ? hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice) : hipMemset(*out, 0, bytes)) != hipSuccess)
        return alloc_failed(h);
    return AMX_OK;
}

// uploads a [rows, cols] fp32 host matrix and packs it as planes at row offset `row0` of dst [*, ldd]
static int pack_linear_host(amx_handle h, const float* data, int rows, int cols, float scale, void* dst, int64_t plane, int64_t ldd,
                            int row0, int cols_pad, float* staging) {
    HIPCHK(h, hipMemcpy(staging, data, (size_t)rows * cols * 4, hipMemcpyHostToDevice));
    launch_pack_matrix(h->prec, staging, rows, cols, cols, 1, scale, (char*)dst + (size_t)row0 * ldd * 2 * (plane == PLANE_IL ? 2 : 1), plane, ldd,
                       cols_pad, 0);
    HIPCHK(h, hipDeviceSynchronize());
    return AMX_OK;
}

// the same for a tensor of the state_dict
static int pack_linear(amx_handle h, const TensorMap& tm, const std::string& key, int rows, int cols, float scale, void* dst,
                       int64_t plane, int64_t ldd, int row0, int cols_pad, float* staging) {
    const amx_tensor* t = tm.get(key);
    if (!t) return fail(h, AMX_EINVAL, "missing tensor in state_dict: " + key);
    if (t->numel != (int64_t)rows * cols)
        return fail(h, AMX_EINVAL, "tensor " + key + " has " + std::to_string(t->numel) + " elements, expected " +
                                       std::to_string((int64_t)rows * cols));
    return pack_linear_host(h, t->data, rows, cols, scale, dst, plane, ldd, row0, cols_pad, staging);
}

// LayerNorm(gamma, beta) folded into the Linear(W [rows, cols], b) behind it:  LN(x) W^T + b = rstd ((x - p) . (gamma (.) W)^T)
// - rstd (mu - p) c + d  with  c = W gamma,  d = W beta + b  (fp64 sums; `pre` multiplies everything: the attention's query scale).
// folded: gamma (.) W * pre in fp32 (one rounding at 2^-24, below the 2^-22 of the planes); c from those values, as the product sees them
static void fold_layer_norm(const float* W, const float* b, const float* gamma, const float* beta, int rows, int cols, float pre,
                            float* folded, float* c, float* d) {
    for (int r = 0; r < rows; ++r) {
        double cs = 0.0, ds = 0.0;
        const float* w = W + (size_t)r * cols;
        float* f = folded + (size_t)r * cols;
        for (int k = 0; k < cols; ++k) {
            f[k] = w[k] * gamma[k] * pre;
            cs += (double)f[k];
            ds += (double)w[k] * (double)beta[k];
        }
        c[r] = (float)cs;
        d[r] = (float)((ds + (double)b[r]) * (double)pre);
    }
}

// power of two that puts the largest |w * pre| of the listed tensors into [4096, 8192); 1 for empty / zero / non-finite data
static float pow2_for(float m) {
    if (!(m > 0.f) || !std::isfinite(m)) return 1.f;
    return std::ldexp(1.f, 12 - std::ilogb(m));
}
static float pack_scale(std::initializer_list<std::pair<const amx_tensor*, float>> tensors) {
    float m = 0.f;
    for (auto& tp : tensors) {
        if (!tp.first) continue;
        const float* d = tp.first->data;
        float mt = 0.f;
        for (int64_t i = 0; i < tp.first->numel; ++i) mt = std::max(mt, std::fabs(d[i]));
        m = std::max(m, mt * std::fabs(tp.second));
    }
    return pow2_for(m);
}

// plane distance of a GEMM operand / row-stride granule of its padded K: interleaved (PLANE_IL, 32) or separate planes
// (a separate plane is never exactly PLANE_IL elements away: tiny matrices get a distance of 64, and every plane buffer is
// allocated with PLANE_SLACK bytes to spare for it)
constexpr size_t PLANE_SLACK = 256;
static int64_t pln(amx_handle h, int64_t separate) { return h->il ? PLANE_IL : std::max<int64_t>(separate, 64); }
static int kalign(amx_handle h) { return h->il ? 32 : 8; }

static void* alloc_planes(amx_handle h, int64_t elems_per_plane) {
    return dev_alloc(h, (size_t)elems_per_plane * 2 * h->NT + PLANE_SLACK);
}

// ---- amx_create, section by section (each returns an AMX_* code with the message set; amx_create destroys the handle) ----

// (interleaved planes: see amx_handle_s::il)
static bool planes_interleaved(const amx_config* cfg) {
    return prec_planes(cfg->precision) > 1 && cfg->conv_dim % 32 == 0 && cfg->ffn % 32 == 0 && cfg->hidden % 32 == 0;
}

static int check_config(const amx_config* cfg, int n_classes, const Conv0Route& c0) {
    if (cfg->abi_version != AMX_ABI_VERSION) return fail(nullptr, AMX_EINVAL, "ABI version mismatch");
    if (cfg->n_conv < 2 || cfg->n_conv > AMX_MAX_CONV) return fail(nullptr, AMX_EINVAL, "n_conv out of range");
    if (cfg->heads < 1 || cfg->hidden % cfg->heads != 0 || (cfg->hidden / cfg->heads) % 8 || cfg->hidden / cfg->heads > 128)
        return fail(nullptr, AMX_EINVAL, "head_dim (hidden / heads) must be a multiple of 8 and at most 128");
    if (cfg->hidden > 2048 || cfg->hidden % 8 || cfg->conv_dim % 8)
        return fail(nullptr, AMX_EINVAL, "hidden must be a multiple of 8 and <= 2048, conv_dim a multiple of 8");
    if (cfg->conv_kernel[0] > 16) return fail(nullptr, AMX_EINVAL, "first conv kernel must be <= 16");
    for (int i = 0; i < cfg->n_conv; ++i)
        if (cfg->conv_kernel[i] < 1 || cfg->conv_stride[i] < 1) return fail(nullptr, AMX_EINVAL, "conv kernels and strides must be positive");
    if (c0.refusal) return fail(nullptr, AMX_EINVAL, c0.refusal);  // a conv_dim or first stride no first-layer kernel serves
    if (cfg->hidden % cfg->pos_groups != 0 || (cfg->hidden / cfg->pos_groups) % 8 || cfg->hidden / cfg->pos_groups > 128)
        return fail(nullptr, AMX_EINVAL, "hidden / pos_groups must be a multiple of 8 and <= 128");
    if (cfg->ffn % 8) return fail(nullptr, AMX_EINVAL, "ffn must be a multiple of 8");
    if (cfg->precision < 0 || cfg->precision > 3) return fail(nullptr, AMX_EINVAL, "unknown precision");
    if (cfg->feat_extract_norm != AMX_NORM_LAYER && cfg->feat_extract_norm != AMX_NORM_GROUP)
        return fail(nullptr, AMX_EINVAL, "`feat_extract_norm` has to be one of ['group', 'layer']");
    if (cfg->embedding_size % 8) return fail(nullptr, AMX_EINVAL, "embedding_size must be a multiple of 8");
    if (cfg->adapter_attn_dim < 0 || cfg->adapter_attn_dim > ADAPTER_MAX_DIM)
        return fail(nullptr, AMX_EINVAL, "adapter_attn_dim must be 0 (no attention adapters) or 1 .. " + std::to_string(ADAPTER_MAX_DIM));
    if (n_classes < 1) return fail(nullptr, AMX_EINVAL, "Each model needs at least one classifier");
    return AMX_OK;
}

// the classifier graph (mirrors the ValueErrors of acoustic_model.py:353-466) and its evaluation order
static int check_classes(amx_handle h) {
    const int n_classes = (int)h->classes.size();
    bool uses_output = false;
    for (int i = 0; i < n_classes; ++i) {
        const auto& c = h->classes[i];
        for (int j = 0; j < i; ++j)
            if (!strncmp(c.name, h->classes[j].name, AMX_NAME_LEN)) return fail(h, AMX_EINVAL, "Dependencies contain duplicate keys");
        if (!strncmp(c.name, "OUTPUT", 6)) return fail(h, AMX_EINVAL, "'OUTPUT' is a reserved keyword");
        if (c.n_deps < 1 || c.n_deps > AMX_MAX_DEPS) return fail(h, AMX_EINVAL, "Each class projection requires a dependency");
        if (c.out_features < 1) return fail(h, AMX_EINVAL, "classifier without outputs");
        if (c.time_heads < 0 || (c.time_heads > 0 && c.out_features % c.time_heads))
            return fail(h, AMX_EINVAL, "embed_dim must be divisible by num_heads");  // nn.MultiheadAttention's assertion
        if (c.time_heads > 0 && c.time_positional && (c.out_features & 1))
            return fail(h, AMX_EINVAL, "sinusoidal position embeddings need an even number of classifier outputs");
        for (int d = 0; d < c.n_deps; ++d) {
            if (c.deps[d] < 0) {
                uses_output = true;
                if (c.deps[d] < -1 && -2 - c.deps[d] > h->cfg.layers) return fail(h, AMX_EINVAL, "OUTPUT_i exceeds the number of encoder layers");
            } else if (c.deps[d] >= n_classes) {
                return fail(h, AMX_EINVAL, "unknown dependency");
            }
        }
    }
    if (!uses_output) return fail(h, AMX_EINVAL, "At least one of the input layers requires 'OUTPUT' as a dependency");
    return evaluation_order(h->classes, h->order, h->err);
}

// the conv layers of the feature extractor, and the LayerNorm statistics table of conv layer 0 on the matrix pipe
static int create_feature_extractor(amx_handle h, const TensorMap& tm, float* staging) {
    const amx_config& cfg = h->cfg;
    const int C = cfg.conv_dim;
    const std::string p0 = AM + "feature_extractor.conv_layers.0.";
    TRY(upload_f32(h, tm, p0 + "conv.weight", (int64_t)C * cfg.conv_kernel[0], &h->c0_w));
    int c_in = 1;
    for (int i = 0; i < cfg.n_conv; ++i) {
        const std::string p = AM + "feature_extractor.conv_layers." + std::to_string(i) + ".";
        const int k = cfg.conv_kernel[i];
        if (cfg.conv_bias) {
            TRY(upload_f32(h, tm, p + "conv.bias", C, &h->conv_b[i]));
        } else {
            // config.conv_bias = False (wav2vec2-base / -large): nn.Conv1d(bias=False) -- a zero bias for the kernels
            TRY(dev_upload(h, &h->conv_b[i], nullptr, (size_t)C * 4));
        }
        // "layer": LayerNorm(C) behind every conv layer; "group": GroupNorm(C, C) behind layer 0 only -- the same key names
        // (`layer_norm.{weight,bias}`, transformers Wav2Vec2GroupNormConvLayer / Wav2Vec2NoLayerNormConvLayer)
        if (!h->gn || i == 0) {
            TRY(upload_f32(h, tm, p + "layer_norm.weight", C, &h->conv_g[i]));
            TRY(upload_f32(h, tm, p + "layer_norm.bias", C, &h->conv_be[i]));
        }
        if (i > 0) {
            const amx_tensor* t = tm.get(p + "conv.weight");
            if (!t || t->numel != (int64_t)C * c_in * k) return fail(h, AMX_EINVAL, "missing or mis-shaped tensor " + p + "conv.weight");
            int64_t plane = (int64_t)C * c_in * k;
            h->conv_w[i] = alloc_planes(h, plane);
            if (!h->conv_w[i]) return alloc_failed(h);
            if (hipMemcpy(staging, t->data, (size_t)t->numel * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(h, AMX_EHIP, "H2D failed");
            const float ps = pack_scale({{t, 1.f}});
            h->conv_r[i] = 1.f / ps;
            launch_pack_conv_w(h->prec, staging, C, c_in, k, ps, h->conv_w[i], pln(h, plane), 0);
            // layers the row-complete kernel may take (LayerNorm variant, conv_dim 512, k > 1 taps): a tap-minor copy too
            const int tm_slice = h->NT == 2 ? 32 : 64;
            if (!h->gn && i < cfg.n_conv - 1 && k > 1 && C == 512 && c_in % tm_slice == 0) {
                h->conv_w_tm[i] = alloc_planes(h, plane);
                if (!h->conv_w_tm[i]) return alloc_failed(h);
                launch_pack_conv_w(h->prec, staging, C, c_in, k, ps, h->conv_w_tm[i], pln(h, plane), 0, tm_slice);
                h->conv_tm_slice = tm_slice;
            }
            if (hipDeviceSynchronize() != hipSuccess) return fail(h, AMX_EHIP, "pack_conv_w failed");
        }
        c_in = C;
    }
    const amx_tensor* wt = tm.get(p0 + "conv.weight");
    if (h->c0.mfma) h->c0_wscale = pack_scale({{wt, 1.f}});
    if (h->c0.stats != CONV0_STATS_TABLE) return AMX_OK;
    // conv layer 0 on the matrix pipe (LayerNorm variant, k = 10, C = 512): the LayerNorm statistics of a frame are a linear
    // and a quadratic form of its 10 samples -- mean_c(w_c . x + b_c) = m . [x; 1], var_c = [x; 1]^T G [x; 1] with m / G the mean
    // / covariance of the rows [w_c, b_c] over the channels -- tabulated here in fp64
    const amx_tensor* bt = cfg.conv_bias ? tm.get(p0 + "conv.bias") : nullptr;
    const int k0 = cfg.conv_kernel[0], dim = k0 + 1;
    std::vector<double> table((size_t)dim + (size_t)dim * dim, 0.0), row(dim);
    for (int ch = 0; ch < C; ++ch)
        for (int j = 0; j < dim; ++j) table[j] += (j < k0 ? (double)wt->data[(size_t)ch * k0 + j] : (bt ? (double)bt->data[ch] : 0.0)) / C;
    for (int ch = 0; ch < C; ++ch) {
        for (int j = 0; j < dim; ++j) row[j] = (j < k0 ? (double)wt->data[(size_t)ch * k0 + j] : (bt ? (double)bt->data[ch] : 0.0)) - table[j];
        for (int a = 0; a < dim; ++a)
            for (int b2 = 0; b2 < dim; ++b2) table[(size_t)dim + (size_t)a * dim + b2] += row[a] * row[b2] / C;
    }
    return dev_upload(h, &h->c0_stats, table.data(), table.size() * 8);
}

// the feature projection and the positional conv (weight-norm folded)
static int create_projection(amx_handle h, const TensorMap& tm, float* staging) {
    const amx_config& cfg = h->cfg;
    const int C = cfg.conv_dim, D = cfg.hidden;
    {
        std::string p = AM + "feature_projection.";
        TRY(upload_f32(h, tm, p + "layer_norm.weight", C, &h->fp_g));
        TRY(upload_f32(h, tm, p + "layer_norm.bias", C, &h->fp_b));
        TRY(upload_f32(h, tm, p + "projection.bias", D, &h->fp_bias));
        h->fp_w = alloc_planes(h, (int64_t)D * C);
        if (!h->fp_w) return alloc_failed(h);
        const float ps = pack_scale({{tm.get(p + "projection.weight"), 1.f}});
        h->fp_r = 1.f / ps;
        TRY(pack_linear(h, tm, p + "projection.weight", D, C, ps, h->fp_w, pln(h, (int64_t)D * C), C, 0, C, staging));
    }
    std::string p = AM + "encoder.pos_conv_embed.conv.";
    const int cg = D / cfg.pos_groups, k = cfg.pos_kernel;
    const amx_tensor* g = tm.get(p + "parametrizations.weight.original0");
    const amx_tensor* v = tm.get(p + "parametrizations.weight.original1");
    if (!g) g = tm.get(p + "weight_g");
    if (!v) v = tm.get(p + "weight_v");
    if (!g || !v || g->numel != k || v->numel != (int64_t)D * cg * k) return fail(h, AMX_EINVAL, "missing or mis-shaped positional conv weights");
    TRY(upload_f32(h, tm, p + "bias", D, &h->pos_b));
    float* gd = (float*)dev_alloc(h, (size_t)k * 4 * 2);
    if (!gd) return alloc_failed(h);
    if (hipMemcpy(gd, g->data, (size_t)k * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(staging, v->data, (size_t)v->numel * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(h, AMX_EHIP, "H2D failed");
    int64_t plane = (int64_t)D * cg * k;
    h->pos_w = alloc_planes(h, plane);
    if (!h->pos_w) return alloc_failed(h);
    float ps = 1.f;
    {   // largest folded weight |v * g[tap] / ||v[:, :, tap]|||, on the host (the device folds them while packing)
        std::vector<double> sq(k, 0.0);
        std::vector<float> mx(k, 0.f);
        const int64_t rows = (int64_t)D * cg;
        for (int64_t r = 0; r < rows; ++r)
            for (int tap = 0; tap < k; ++tap) {
                const float x = v->data[r * k + tap];
                sq[tap] += (double)x * x;
                mx[tap] = std::max(mx[tap], std::fabs(x));
            }
        float m = 0.f;
        for (int tap = 0; tap < k; ++tap)
            if (sq[tap] > 0.0) m = std::max(m, (float)(mx[tap] * std::fabs(g->data[tap]) / std::sqrt(sq[tap])));
        ps = pow2_for(m);
    }
    h->pos_r = 1.f / ps;
    launch_pack_posconv_w(h->prec, gd, staging, D, cg, k, ps, gd + k, h->pos_w, plane, 0);
    if (hipDeviceSynchronize() != hipSuccess) return fail(h, AMX_EHIP, "pack_posconv_w failed");
    return AMX_OK;
}

// The attention adapter of layer l (Wav2Vec2AttnAdapterLayer: norm, linear_1, ReLU, linear_2).  Its LayerNorm is folded into
// linear_1 like the layer's other norms (fold_layer_norm), linear_2 is stored transposed: both matrices are then [A, D], read by
// column block.  A model without adapters (or a post-LN one, which upstream builds without them) must not carry their tensors:
// they are refused, never dropped.
static int create_adapter(amx_handle h, const TensorMap& tm, int l) {
    const int D = h->cfg.hidden, A = h->adapter;
    const std::string p = AM + "encoder.layers." + std::to_string(l) + ".adapter_layer.";
    if (A == 0) {
        auto it = tm.m.lower_bound(p);
        if (it != tm.m.end() && it->first.compare(0, p.size(), p) == 0)
            return fail(h, AMX_EINVAL, "tensor " + it->first + " belongs to an attention adapter, but " +
                                           (h->cfg.adapter_attn_dim ? "post-LN encoder layers (do_stable_layer_norm = false) have none"
                                                                    : "adapter_attn_dim is 0"));
        return AMX_OK;
    }
    const amx_tensor* t[6];
    const char* names[6] = {"norm.weight", "norm.bias", "linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias"};
    const int64_t numel[6] = {D, D, (int64_t)A * D, A, (int64_t)D * A, D};
    for (int i = 0; i < 6; ++i) {
        t[i] = tm.get(p + names[i]);
        if (!t[i]) return fail(h, AMX_EINVAL, "missing tensor in state_dict: " + p + names[i] + " (adapter_attn_dim = " + std::to_string(A) + ")");
        if (t[i]->numel != numel[i])
            return fail(h, AMX_EINVAL, "tensor " + p + names[i] + " has " + std::to_string(t[i]->numel) + " elements, expected " +
                                           std::to_string(numel[i]) + " (adapter_attn_dim = " + std::to_string(A) + ")");
    }
    std::vector<float> w1((size_t)A * D), c(A), b1(A), w2t((size_t)A * D);
    fold_layer_norm(t[2]->data, t[3]->data, t[0]->data, t[1]->data, A, D, 1.f, w1.data(), c.data(), b1.data());
    for (int d = 0; d < D; ++d)
        for (int a = 0; a < A; ++a) w2t[(size_t)a * D + d] = t[4]->data[(size_t)d * A + a];
    Layer& ly = h->layers[l];
    TRY(dev_upload(h, &ly.ad_w1, w1.data(), w1.size() * 4));
    TRY(dev_upload(h, &ly.ad_b1, b1.data(), b1.size() * 4));
    TRY(dev_upload(h, &ly.ad_w2t, w2t.data(), w2t.size() * 4));
    return upload_f32(h, tm, p + "linear_2.bias", D, &ly.ad_b2);
}

// encoder layer l: Q / K / V as one product, the out-projection, the FFN
static int create_layer(amx_handle h, const TensorMap& tm, int l, float* staging) {
    const int D = h->cfg.hidden, F = h->cfg.ffn;
    // folded into W_q / b_q: dh^-0.5 and log2(e) -- the attention softmax runs in base 2 (v_exp_f32)
    const float qscale = 1.44269504088896340736f / sqrtf((float)(D / h->cfg.heads));
    Layer& ly = h->layers[l];
    const std::string p = AM + "encoder.layers." + std::to_string(l) + ".";
    TRY(upload_f32(h, tm, p + "layer_norm.weight", D, &ly.ln1_g));
    TRY(upload_f32(h, tm, p + "layer_norm.bias", D, &ly.ln1_b));
    TRY(upload_f32(h, tm, p + "final_layer_norm.weight", D, &ly.ln2_g));
    TRY(upload_f32(h, tm, p + "final_layer_norm.bias", D, &ly.ln2_b));
    ly.wqkv = alloc_planes(h, (int64_t)3 * D * D);
    ly.wo = alloc_planes(h, (int64_t)D * D);
    ly.w1 = alloc_planes(h, (int64_t)F * D);
    ly.w2 = alloc_planes(h, (int64_t)D * F);
    ly.bqkv = (float*)dev_alloc(h, (size_t)3 * D * 4);
    if (!ly.wqkv || !ly.wo || !ly.w1 || !ly.w2 || !ly.bqkv) return alloc_failed(h);
    // a Linear [rows, cols] as it is: weight planes under their own power of two, fp32 bias
    auto linear = [&](const std::string& name, int rows, int cols, void* w, float& r, float** b) {
        const float ps = pack_scale({{tm.get(p + name + ".weight"), 1.f}});
        r = 1.f / ps;
        TRY(pack_linear(h, tm, p + name + ".weight", rows, cols, ps, w, pln(h, (int64_t)rows * cols), cols, 0, cols, staging));
        return upload_f32(h, tm, p + name + ".bias", rows, b);
    };
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    if (h->stable) {
        // pre-LN layer: `layer_norm` folded into Q / K / V, `final_layer_norm` into FFN1 (see fold_layer_norm)
        const amx_tensor *g1 = tm.get(p + "layer_norm.weight"), *be1 = tm.get(p + "layer_norm.bias");
        const amx_tensor *g2 = tm.get(p + "final_layer_norm.weight"), *be2 = tm.get(p + "final_layer_norm.bias");
        std::vector<float> folded((size_t)std::max(3 * D, F) * D), cvec(std::max(3 * D, F)), dvec(std::max(3 * D, F));
        for (int j = 0; j < 3; ++j) {
            const amx_tensor* w = tm.get(p + "attention." + names[j] + ".weight");
            const amx_tensor* b = tm.get(p + "attention." + names[j] + ".bias");
            if (!w || w->numel != (int64_t)D * D || !b || b->numel != D) return fail(h, AMX_EINVAL, "missing or mis-shaped tensor " + p + "attention." + names[j]);
            fold_layer_norm(w->data, b->data, g1->data, be1->data, D, D, j == 0 ? qscale : 1.f, folded.data() + (size_t)j * D * D,
                            cvec.data() + j * D, dvec.data() + j * D);
        }
        amx_tensor ft{};
        ft.data = folded.data(); ft.numel = (int64_t)3 * D * D;
        const float ps_qkv = pack_scale({{&ft, 1.f}});
        ly.r_qkv = 1.f / ps_qkv;
        TRY(pack_linear_host(h, folded.data(), 3 * D, D, ps_qkv, ly.wqkv, pln(h, (int64_t)3 * D * D), D, 0, D, staging));
        TRY(dev_upload(h, &ly.c_qkv, cvec.data(), (size_t)3 * D * 4));
        if (hipMemcpy(ly.bqkv, dvec.data(), (size_t)3 * D * 4, hipMemcpyHostToDevice) != hipSuccess) return alloc_failed(h);
        const amx_tensor* w1 = tm.get(p + "feed_forward.intermediate_dense.weight");
        const amx_tensor* b1 = tm.get(p + "feed_forward.intermediate_dense.bias");
        if (!w1 || w1->numel != (int64_t)F * D || !b1 || b1->numel != F) return fail(h, AMX_EINVAL, "missing or mis-shaped tensor " + p + "feed_forward.intermediate_dense");
        fold_layer_norm(w1->data, b1->data, g2->data, be2->data, F, D, 1.f, folded.data(), cvec.data(), dvec.data());
        ft.numel = (int64_t)F * D;
        const float ps_1 = pack_scale({{&ft, 1.f}});
        ly.r_1 = 1.f / ps_1;
        TRY(pack_linear_host(h, folded.data(), F, D, ps_1, ly.w1, pln(h, (int64_t)F * D), D, 0, D, staging));
        TRY(dev_upload(h, &ly.c_1, cvec.data(), (size_t)F * 4));
        TRY(dev_upload(h, &ly.b1, dvec.data(), (size_t)F * 4));
    } else {
        const float ps_qkv = pack_scale({{tm.get(p + "attention.q_proj.weight"), qscale}, {tm.get(p + "attention.k_proj.weight"), 1.f},
                                         {tm.get(p + "attention.v_proj.weight"), 1.f}});
        ly.r_qkv = 1.f / ps_qkv;
        for (int j = 0; j < 3; ++j) {
            float sc = j == 0 ? qscale : 1.f;
            TRY(pack_linear(h, tm, p + "attention." + names[j] + ".weight", D, D, sc * ps_qkv, ly.wqkv, pln(h, (int64_t)3 * D * D), D, j * D, D, staging));
            const amx_tensor* b = tm.get(p + "attention." + names[j] + ".bias");
            if (!b || b->numel != D) return fail(h, AMX_EINVAL, "missing tensor " + p + "attention." + names[j] + ".bias");
            if (hipMemcpy(staging, b->data, (size_t)D * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(h, AMX_EHIP, "H2D failed");
            launch_scale_copy(staging, ly.bqkv + j * D, D, sc, 0);
            if (hipDeviceSynchronize() != hipSuccess) return fail(h, AMX_EHIP, "scale_copy failed");
        }
    }
    TRY(linear("attention.out_proj", D, D, ly.wo, ly.r_o, &ly.bo));
    if (!h->stable) TRY(linear("feed_forward.intermediate_dense", F, D, ly.w1, ly.r_1, &ly.b1));
    TRY(linear("feed_forward.output_dense", D, F, ly.w2, ly.r_2, &ly.b2));
    return create_adapter(h, tm, l);
}

// the hierarchical projection: one HeadStep per classifier in evaluation order (direct-output classifiers stacked), then their
// weights packed
static int create_heads(amx_handle h, const TensorMap& tm, float* staging) {
    const amx_config& cfg = h->cfg;
    h->need_hidden.assign(cfg.layers + 1, false);
    const bool blanks = cfg.dependency_blanks != 0;
    auto dep_width = [&](int dep) -> int {
        if (dep < 0) return cfg.hidden;
        return h->classes[dep].size + (blanks ? 1 : 0);
    };
    for (size_t oi = 0; oi < h->order.size(); ++oi) {
        int ci = h->order[oi];
        const amx_class_desc& c = h->classes[ci];
        bool composed = cfg.embedding_size > 0 && !strcmp(c.name, "phoneme");
        if (composed) {
            if (c.out_features != cfg.embedding_size) return fail(h, AMX_EINVAL, "phoneme out_features must equal embedding_size");
            h->composed_class = ci;
        }
        bool direct = c.n_deps == 1 && c.deps[0] == AMX_DEP_OUTPUT;
        int K = 0;
        for (int d = 0; d < c.n_deps; ++d) {
            K += dep_width(c.deps[d]);
            if (c.deps[d] < -1) h->need_hidden[-2 - c.deps[d]] = true;
        }
        // stack onto the previous step when both read the final LayerNorm output directly and neither is composed
        if (direct && !composed && c.time_heads == 0 && !h->steps.empty() && h->steps.back().direct_output &&
            !h->steps.back().composed && h->steps.back().time_heads == 0) {
            h->steps.back().classes.push_back(ci);
            h->steps.back().rows += c.out_features;
            continue;
        }
        HeadStep st{};
        st.classes = {ci};
        st.direct_output = direct;
        st.K = K;
        st.Kpad = round_up(K, kalign(h));
        st.rows = c.out_features;
        st.composed = composed;
        st.parts_dev = nullptr;
        st.time_heads = c.time_heads;
        st.Cpad = round_up(c.out_features, kalign(h));
        if (!direct) {
            int colp = 0;
            for (int d = 0; d < c.n_deps; ++d) {
                ConcatPart pt{};
                int dep = c.deps[d];
                pt.type = dep < 0 ? 0 : 1;
                pt.width = dep_width(dep);
                pt.dst_col = colp;
                pt.src_col = 0;
                pt.src = nullptr;
                colp += pt.width;
                st.parts.push_back(pt);
                st.part_dep.push_back(dep);
            }
        }
        h->steps.push_back(st);
    }
    for (auto& st : h->steps) {
        st.W = alloc_planes(h, (int64_t)st.rows * st.Kpad);
        st.bias = (float*)dev_alloc(h, (size_t)st.rows * 4);
        if (!st.W || !st.bias) return alloc_failed(h);
        int row0 = 0;
        float ps_w = 1.f;
        {   // one scale for the stacked rows of the step
            float m = 0.f;
            for (int ci : st.classes) {
                std::string key = PROJ + h->classes[ci].name + "._time_distributed_layer." + (st.time_heads > 0 ? "input_projection." : "") + "weight";
                const amx_tensor* t = tm.get(key);
                if (t) for (int64_t i = 0; i < t->numel; ++i) m = std::max(m, std::fabs(t->data[i]));
            }
            ps_w = pow2_for(m);
        }
        st.r_w = 1.f / ps_w;
        for (int ci : st.classes) {
            const amx_class_desc& c = h->classes[ci];
            std::string p = PROJ + c.name + "._time_distributed_layer.";
            if (st.time_heads > 0) {
                // module tree of ProjectingMultiheadAttention: input_projection, layer_norm, attention (nn.MultiheadAttention)
                const int Co = c.out_features;
                const int64_t plane_in = (int64_t)3 * Co * st.Cpad, plane_out = (int64_t)Co * st.Cpad;
                st.tl_win = alloc_planes(h, plane_in);
                st.tl_wout = alloc_planes(h, plane_out);
                if (!st.tl_win || !st.tl_wout) return alloc_failed(h);
                const float ps_in = pack_scale({{tm.get(p + "attention.in_proj_weight"), 1.f}});
                const float ps_out = pack_scale({{tm.get(p + "attention.out_proj.weight"), 1.f}});
                st.r_tin = 1.f / ps_in; st.r_tout = 1.f / ps_out;
                TRY(pack_linear(h, tm, p + "attention.in_proj_weight", 3 * Co, Co, ps_in, st.tl_win, pln(h, plane_in), st.Cpad, 0, st.Cpad, staging));
                TRY(pack_linear(h, tm, p + "attention.out_proj.weight", Co, Co, ps_out, st.tl_wout, pln(h, plane_out), st.Cpad, 0, st.Cpad, staging));
                TRY(upload_f32(h, tm, p + "attention.in_proj_bias", 3 * Co, &st.tl_bin));
                TRY(upload_f32(h, tm, p + "attention.out_proj.bias", Co, &st.tl_bout));
                TRY(upload_f32(h, tm, p + "layer_norm.weight", Co, &st.tl_g));
                TRY(upload_f32(h, tm, p + "layer_norm.bias", Co, &st.tl_b));
                if (c.time_positional) {
                    // SinusoidalPositionEmbeddings (acoustic_model.py:34-69): base_k = exp(-2k ln(1e4) / size) for the
                    // column pair (2k, 2k+1)
                    std::vector<float> base(Co);
                    // fp32 like upstream: arange(0, size, 2) * float(-ln(1e4) / size), then exp
                    const float step = (float)(-(std::log(10000.0) / Co));
                    for (int col = 0; col < Co; ++col) {
                        volatile float arg = (float)(col & ~1) * step;
                        base[col] = (float)std::exp((double)arg);
                    }
                    st.tl_pe = (float*)dev_alloc(h, (size_t)Co * 4);
                    if (!st.tl_pe) return alloc_failed(h);
                    if (hipMemcpy(st.tl_pe, base.data(), (size_t)Co * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(h, AMX_EHIP, "H2D failed");
                }
                p += "input_projection.";
            }
            TRY(pack_linear(h, tm, p + "weight", c.out_features, st.K, ps_w, st.W, pln(h, (int64_t)st.rows * st.Kpad), st.Kpad, row0, st.Kpad, staging));
            const amx_tensor* b = tm.get(p + "bias");
            if (!b || b->numel != c.out_features) return fail(h, AMX_EINVAL, "missing tensor " + p + "bias");
            if (hipMemcpy(st.bias + row0, b->data, (size_t)c.out_features * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(h, AMX_EHIP, "H2D failed");
            row0 += c.out_features;
        }
        if (!st.parts.empty()) {
            st.parts_dev = (ConcatPart*)dev_alloc(h, st.parts.size() * sizeof(ConcatPart));
            if (!st.parts_dev) return alloc_failed(h);
        }
    }
    return AMX_OK;
}

// the composition embedding table (kept on the host too: install_inventory scales each composed matrix from it)
static int create_composition(amx_handle h, const TensorMap& tm) {
    const std::string key = PROJ + "phoneme._composition_layer._attribute_embeddings.weight";
    const amx_tensor* t = tm.get(key);
    if (!t || t->numel % h->cfg.embedding_size) return fail(h, AMX_EINVAL, "missing tensor " + key);
    h->emb_rows = (int)(t->numel / h->cfg.embedding_size);
    h->emb_host.assign(t->data, t->data + t->numel);
    return upload_f32(h, tm, key, t->numel, &h->emb);
}
#undef TRY

extern "C" int amx_create(amx_handle* out, int device, const amx_config* cfg, const amx_class_desc* classes, int n_classes,
                          const amx_tensor* tensors, int n_tensors) {
    if (!out || !cfg || !classes || !tensors) return fail(nullptr, AMX_EINVAL, "null argument");
    *out = nullptr;
    const Conv0Route c0 = conv0_route(cfg->precision, planes_interleaved(cfg), cfg->conv_dim, cfg->conv_kernel[0], cfg->conv_stride[0],
                                      cfg->feat_extract_norm == AMX_NORM_GROUP);
    if (int rc = check_config(cfg, n_classes, c0)) return rc;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, AMX_EHIP, "no HIP device available: liballophant_amx has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, AMX_EINVAL, "device index out of range");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");

    amx_handle h = new amx_handle_s();
    h->device = device;
    h->cfg = *cfg;
    h->prec = cfg->precision;
    h->NT = prec_planes(cfg->precision);
    h->gn = cfg->feat_extract_norm == AMX_NORM_GROUP;
    h->stable = cfg->stable_layer_norm != 0;
    h->masked = cfg->use_attention_mask != 0;
    // (the post-LN layer class builds no adapter even when the config names one: the field has no effect there, as upstream)
    h->adapter = h->stable ? cfg->adapter_attn_dim : 0;
    // (hidden too -- round 6: the residual-stream planes [M, hidden] are GEMM operands like the others; a hidden size off the
    // 32-element blocks -- 240 = 2 heads of 120 -- ran interleaved planes through kernels that assume block-aligned rows)
    h->il = planes_interleaved(cfg);
    h->c0 = c0;
    h->classes.assign(classes, classes + n_classes);
    auto bail = [&](int code) {
        g_create_error = h->err;
        amx_destroy(h);
        return code;
    };
    int rc = check_classes(h);
    if (rc) return bail(rc);

    TensorMap tm;
    int64_t max_numel = 0;
    for (int i = 0; i < n_tensors; ++i) {
        tm.m[tensors[i].name] = &tensors[i];
        max_numel = std::max(max_numel, tensors[i].numel);
    }
    // (the fused, LayerNorm-folded Q / K / V matrix is packed from one host buffer of 3 hidden^2 floats: larger than any single
    // tensor when ffn < 3 hidden)
    max_numel = std::max<int64_t>(max_numel, (int64_t)3 * cfg->hidden * cfg->hidden);
    float* staging = nullptr;
    if (hipMalloc(&staging, (size_t)max_numel * 4 + 16) != hipSuccess) { h->err = "staging allocation failed"; return bail(AMX_ENOMEM); }
    struct StagingGuard {
        float* p;
        ~StagingGuard() { (void)hipFree(p); }
    } guard{staging};

    const int D = cfg->hidden;
    rc = create_feature_extractor(h, tm, staging);
    if (!rc) rc = create_projection(h, tm, staging);
    h->layers.resize(cfg->layers);
    for (int l = 0; l < cfg->layers && !rc; ++l) rc = create_layer(h, tm, l, staging);
    // the affine part of a folded LayerNorm lives in the weights: its row pass (short batches) normalises with (1, 0)
    const std::vector<float> ones(D, 1.f);
    if (!rc) rc = dev_upload(h, &h->unit_g, ones.data(), (size_t)D * 4);
    if (!rc) rc = dev_upload(h, &h->zero_b, nullptr, (size_t)D * 4);
    if (!rc) rc = upload_f32(h, tm, AM + "encoder.layer_norm.weight", D, &h->fln_g);
    if (!rc) rc = upload_f32(h, tm, AM + "encoder.layer_norm.bias", D, &h->fln_b);
    if (!rc) rc = create_heads(h, tm, staging);
    if (!rc && h->composed_class >= 0) rc = create_composition(h, tm);
    if (!rc) rc = dev_upload(h, &h->nonfinite, nullptr, 16);
    // no composition layer: one implicit inventory (fixed output widths)
    if (!rc && h->composed_class < 0) rc = install_inventory(h, std::vector<int64_t>{}, std::vector<int64_t>{}, 0, 0, 0);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(h, AMX_EHIP, "device synchronisation failed after packing");
    if (rc) return bail(rc);
    *out = h;
    return AMX_OK;
}

extern "C" int amx_destroy(amx_handle h) {
    if (!h) return AMX_OK;
    // teardown is best effort: a failing release cannot be reported more usefully than by carrying on
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (void* p : h->allocs) (void)hipFree(p);
    for (auto& kv : h->ws)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& e : h->inventories) free_inventory(e);
    for (int i = 0; i < amx_handle_s::PIN_SLOTS; ++i) {
        if (h->h_lengths_pinned[i]) (void)hipHostFree(h->h_lengths_pinned[i]);
        if (h->h_frames_pinned[i]) (void)hipHostFree(h->h_frames_pinned[i]);
        if (h->h_rowoff_pinned[i]) (void)hipHostFree(h->h_rowoff_pinned[i]);
        if (h->h_tiles_pinned[i]) (void)hipHostFree(h->h_tiles_pinned[i]);
        if (h->pin_event[i]) (void)hipEventDestroy(h->pin_event[i]);
    }
    drop_graphs(h);
    if (h->capture_stream) (void)hipStreamDestroy(h->capture_stream);
    for (auto& sl : h->range) {
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.ev) (void)hipEventDestroy(sl.ev);
    }
    for (auto& sp : h->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (auto e : h->event_pool) (void)hipEventDestroy(e);
    if (h->al_buf) (void)hipFree(h->al_buf);
    delete h;
    return AMX_OK;
}

extern "C" const char* amx_last_error(amx_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

extern "C" int64_t amx_device_bytes(amx_handle h) { return h ? h->weight_bytes + h->ws_bytes : 0; }

// =================================================================================================================
// inventory
// =================================================================================================================
// (column, width) of every class in the logits buffer and the (column, classes, class prefix) tables of the outputs for an
// inventory of P1 - 1 phones; geometry-independent
static void build_tables(amx_handle h, int P1, std::vector<int>& col, std::vector<int>& width, int& ld_logits,
                         std::vector<OutDesc>& uniq, std::vector<OutDesc>& all) {
    const int nc = (int)h->classes.size();
    col.assign(nc, 0);
    width.assign(nc, 0);
    int colp = 0;
    for (int ci : h->order) {
        col[ci] = colp;
        width[ci] = ci == h->composed_class ? P1 : h->classes[ci].out_features;
        colp += width[ci];
    }
    ld_logits = round_up(colp, 4);
    uniq.clear();
    all.clear();
    int64_t prefix = 0;
    for (int ci : h->order) {
        OutDesc od{col[ci], width[ci], prefix};
        uniq.push_back(od);
        if (!strcmp(h->classes[ci].name, "phoneme") && h->cfg.allophone_layer) all.push_back(od);  // "phone" alias
        all.push_back(od);
        prefix += width[ci];
    }
}

static void free_inventory(amx_handle_s::Inventory& e) {
    if (e.composed_w) (void)hipFree(e.composed_w);
    if (e.composed_f32) (void)hipFree(e.composed_f32);
    if (e.idx_dev) (void)hipFree(e.idx_dev);
    if (e.out_unique_dev) (void)hipFree(e.out_unique_dev);
    if (e.out_all_dev) (void)hipFree(e.out_all_dev);
    e = amx_handle_s::Inventory{};
}

static void select_inventory(amx_handle h, int i) {
    h->inventories[i].last_use = ++h->inv_clock;
    h->inv = i;
}

// the inventory the next pass uses (callers have checked h->inv >= 0: compute_layout)
static const amx_handle_s::Inventory& cur_inv(amx_handle h) { return h->inventories[h->inv]; }

// builds a new cache entry on `s`: every buffer is fresh, so nothing in flight can be reading it
static int install_inventory(amx_handle h, std::vector<int64_t>&& key, const std::vector<int64_t>& idx, int P1, int features,
                             hipStream_t s) {
    int slot = -1;
    if ((int)h->inventories.size() < amx_handle_s::INV_CAP) {
        h->inventories.emplace_back();
        slot = (int)h->inventories.size() - 1;
    } else {
        // evict the least recently used entry; a forward pass still in flight may read its buffers
        for (int i = 0; i < (int)h->inventories.size(); ++i)
            if (i != h->inv && (slot < 0 || h->inventories[i].last_use < h->inventories[slot].last_use)) slot = i;
        HIPCHK(h, hipDeviceSynchronize());
        free_inventory(h->inventories[slot]);
    }
    auto& e = h->inventories[slot];
    e.P1 = P1;
    const int E = h->cfg.embedding_size;
    std::vector<int> col, width;
    int ld;
    std::vector<OutDesc> uniq, all;
    build_tables(h, P1, col, width, ld, uniq, all);
    auto fail_free = [&](int code, const char* msg) {
        free_inventory(e);
        if (slot == (int)h->inventories.size() - 1) h->inventories.pop_back();
        return fail(h, code, msg);
    };
    if (hipMalloc((void**)&e.out_unique_dev, uniq.size() * sizeof(OutDesc)) != hipSuccess ||
        hipMalloc((void**)&e.out_all_dev, all.size() * sizeof(OutDesc)) != hipSuccess)
        return fail_free(AMX_ENOMEM, "inventory table allocation failed");
    if (hipMemcpyAsync(e.out_unique_dev, uniq.data(), uniq.size() * sizeof(OutDesc), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(e.out_all_dev, all.data(), all.size() * sizeof(OutDesc), hipMemcpyHostToDevice, s) != hipSuccess)
        return fail_free(AMX_EHIP, "inventory table upload failed");
    if (P1 > 0) {
        if (hipMalloc((void**)&e.idx_dev, idx.size() * 8) != hipSuccess ||
            hipMalloc(&e.composed_w, (size_t)P1 * round_up(E, kalign(h)) * 2 * h->NT + PLANE_SLACK) != hipSuccess ||
            hipMalloc((void**)&e.composed_f32, (size_t)P1 * E * 4) != hipSuccess)
            return fail_free(AMX_ENOMEM, "inventory allocation failed");
        if (hipMemcpyAsync(e.idx_dev, idx.data(), idx.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess)
            return fail_free(AMX_EHIP, "inventory upload failed");
        {   // largest entry of the composed matrix (sums of embedding rows), on the host
            float m = 0.f;
            for (int p = 0; p < P1; ++p)
                for (int col = 0; col < E; ++col) {
                    float acc = 0.f;
                    for (int f = 0; f < features; ++f) {
                        const int64_t r = idx[(size_t)p * features + f];
                        if (r >= 0) acc += h->emb_host[(size_t)r * E + col];
                    }
                    m = std::max(m, std::fabs(acc));
                }
            const float ps = pow2_for(m);
            e.r_composed = 1.f / ps;
            const int Eld = round_up(E, kalign(h));  // row stride of the planes; the pad columns are never read (K = E)
            if (Eld != E && hipMemsetAsync(e.composed_w, 0, (size_t)P1 * Eld * 2 * h->NT, s) != hipSuccess)
                return fail_free(AMX_EHIP, "inventory upload failed");
            launch_compose(h->prec, h->emb, E, e.idx_dev, P1, features, ps, e.composed_f32, e.composed_w, pln(h, (int64_t)P1 * Eld), Eld, s);
        }
        if (hipGetLastError() != hipSuccess) return fail_free(AMX_EHIP, "compose kernel launch failed");
    }
    // the uploads above read pageable host vectors that die with this call; a new inventory is a rare event (the cache
    // serves repeats), so the call simply waits for them instead of relying on the runtime's staging behaviour
    if (hipStreamSynchronize(s) != hipSuccess) return fail_free(AMX_EHIP, "inventory upload failed");
    e.key = std::move(key);
    e.generation = ++h->inv_gen;
    select_inventory(h, slot);
    return AMX_OK;
}

extern "C" int amx_set_inventory(amx_handle h, const int64_t* tfi, int phones, int features, const int64_t* offsets,
                                 void* stream) {
    if (!h) return AMX_EINVAL;
    if (h->composed_class < 0) return fail(h, AMX_ESTATE, "model has no embedding composition layer");
    if (!tfi || !offsets || phones < 1 || features < 1) return fail(h, AMX_EINVAL, "bad inventory arguments");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<int64_t> key;
    key.reserve(2 + (size_t)phones * features + features);
    key.push_back(phones);
    key.push_back(features);
    key.insert(key.end(), tfi, tfi + (size_t)phones * features);
    key.insert(key.end(), offsets, offsets + features);
    for (int i = 0; i < (int)h->inventories.size(); ++i)
        if (h->inventories[i].key == key) {
            select_inventory(h, i);
            return AMX_OK;
        }
    const int P1 = phones + 1;
    std::vector<int64_t> idx((size_t)P1 * features, -1);
    idx[0] = 0;  // blank embedding = row 0 (acoustic_model.py:226-228)
    for (int p = 0; p < phones; ++p)
        for (int f = 0; f < features; ++f) {
            int64_t r = tfi[(size_t)p * features + f] + offsets[f];
            if (r < 0 || r >= h->emb_rows) return fail(h, AMX_EINVAL, "composition feature index out of range of the embedding table");
            idx[(size_t)(p + 1) * features + f] = r;
        }
    return install_inventory(h, std::move(key), idx, P1, features, (hipStream_t)stream);
}

// =================================================================================================================
// layout
// =================================================================================================================
// frontend.py:192-203 applied per conv layer (acoustic_model.py:832-835) with floor division: the frames of `len` samples, and
// in Ts (when given) Ts[0] = len and Ts[i + 1] = the output rows of layer i.  0 from the first layer whose input is shorter than
// its kernel on (the reference's formula goes non-positive there)
static int64_t conv_lengths(const amx_config& c, int64_t len, int64_t* Ts = nullptr) {
    if (Ts) Ts[0] = len;
    for (int i = 0; i < c.n_conv; ++i) {
        len = len < c.conv_kernel[i] ? 0 : (len - c.conv_kernel[i]) / c.conv_stride[i] + 1;
        if (Ts) Ts[i + 1] = len;
    }
    return len;
}

// Largest N for which a batch padded to L samples stays inside the 32-bit offsets of the kernels: in the two-plane modes
// the lo plane of an activation is addressed as (32-bit byte offset of the hi plane element) + (plane bytes), so every
// activation plane plus the largest offset inside a tile must stay below 4 GiB; row indices are 32-bit.
static int64_t max_utterances_for(const amx_config& c, int NT, int64_t L) {
    int64_t Ts[AMX_MAX_CONV + 1];
    const int64_t T = conv_lengths(c, L, Ts), Tp = (T + 63) / 64 * 64;
    if (T == 0) return 0;
    const int64_t C = c.conv_dim, D = c.hidden, F = c.ffn, H = c.heads;
    const int64_t wide = std::max<int64_t>(F, 3 * D);
    const int64_t LIMIT = ((int64_t)1 << 32) - ((int64_t)64 << 20);  // 4 GiB minus slack for the offsets inside a tile
    int64_t best = INT32_MAX / std::max<int64_t>(Ts[1], 1);           // 32-bit row indices of the first conv output
    best = std::min(best, (int64_t)INT32_MAX / std::max<int64_t>(T, 1));
    best = std::min(best, ((int64_t)INT32_MAX * 4 / wide) / std::max<int64_t>(T, 1));
    // one plane of every activation stays below 4 GiB in the single-plane modes too: the buffer loads of those kernels use
    // the same 32-bit byte offsets (NT only decides whether a second plane follows)
    (void)NT;
    // conv activations [N * Ts[i], C]: plane + one utterance (tiles crossing an utterance boundary)
    for (int i = 1; i < c.n_conv; ++i) best = std::min(best, LIMIT / (Ts[i] * C * 2) - 1);
    best = std::min(best, LIMIT / (T * wide * 2));        // FFN activation / fused QKV rows
    best = std::min(best, LIMIT / (H * Tp * (D / H > 64 ? 128 : 64) * 2));     // Q / K / V planes (rows padded to 64 / 128 columns)
    best = std::min(best, LIMIT / ((T + c.pos_kernel) * D * 2));  // padded image of the positional convolution
    return std::max<int64_t>(best, 0);
}

extern "C" int64_t amx_max_utterances(amx_handle h, int64_t L) {
    if (!h || L < 1) return 0;
    return max_utterances_for(h->cfg, h->NT, L);
}

static int compute_layout(amx_handle h, int N, int64_t L) {
    if (N < 1 || L < 1) return fail(h, AMX_EINVAL, "empty batch");
    const int64_t T = conv_lengths(h->cfg, L);
    if (T == 0) return fail(h, AMX_EINVAL, "utterances are shorter than the receptive field of the feature extractor");
    if (T > 1 << 20) return fail(h, AMX_EINVAL, "utterance too long");
    if (h->inv < 0)
        return fail(h, AMX_ESTATE, "composition model needs amx_set_inventory before prediction (the training inventory is a non-persistent buffer upstream)");
    if (h->layout_N == N && h->layout_T == T && h->layout_inv == h->inv && h->layout_gen == cur_inv(h).generation)
        return AMX_OK;
    build_tables(h, cur_inv(h).P1, h->col, h->width, h->ld_logits, h->out_unique, h->out_all);
    h->outputs.clear();
    int64_t off = 0;
    for (int ci : h->order) {
        const amx_class_desc& c = h->classes[ci];
        bool is_phoneme = !strcmp(c.name, "phoneme");
        if (is_phoneme && h->cfg.allophone_layer) {
            amx_output_desc d{};
            strncpy(d.name, "phone", AMX_NAME_LEN - 1);
            d.classes = h->width[ci];
            d.offset = off;
            h->outputs.push_back(d);
        }
        amx_output_desc d{};
        strncpy(d.name, c.name, AMX_NAME_LEN - 1);
        d.classes = h->width[ci];
        d.offset = off;
        h->outputs.push_back(d);
        off += (int64_t)T * N * h->width[ci];
    }
    h->layout_N = N;
    h->layout_T = T;
    h->layout_inv = h->inv;
    h->layout_gen = cur_inv(h).generation;
    return AMX_OK;
}

static int64_t layout_total(amx_handle h, int N, int64_t T) {
    int64_t tot = 0;
    for (auto& o : h->out_unique) tot += (int64_t)T * N * o.C;
    return tot;
}

extern "C" int amx_output_layout(amx_handle h, int N, int64_t L, amx_output_desc* descs, int* n_outputs, int64_t* T,
                                 int64_t* total) {
    if (!h) return AMX_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    int rc = compute_layout(h, N, L);
    if (rc) return rc;
    if (n_outputs) *n_outputs = (int)h->outputs.size();
    if (T) *T = h->layout_T;
    if (total) *total = layout_total(h, N, h->layout_T);
    if (descs) memcpy(descs, h->outputs.data(), h->outputs.size() * sizeof(amx_output_desc));
    return AMX_OK;
}

// =================================================================================================================
// forward
// =================================================================================================================
static void drop_graphs(amx_handle h) {
    for (auto& g : h->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
    h->graph_seen.clear();
}

// Reads a completed range slot: adds its frames to `total` and "pass #id: frames" to `readings`.  A continuation slice's reading is
// the chain's running count: what it adds is the difference to its predecessor's reading.
static void range_read(amx_handle h, amx_handle_s::RangeSlot& sl, int64_t& total, std::string& readings) {
    sl.pending = false;
    const int reading = *sl.host;
    const int added = sl.cont && h->range_chain_open ? reading - h->range_chain_seen : reading;
    h->range_chain_seen = reading;
    h->range_chain_open = true;
    if (added > 0) {
        total += added;
        readings += (readings.empty() ? "" : ", ") + std::string("pass #") + std::to_string(sl.pass_id) + ": " + std::to_string(added);
    }
}

// Range report of EARLIER forward passes: reads the pinned count of every pass whose trailing event has completed (`wait`:
// of every pass issued -- the caller has just synchronised or accepts to).  Returns AMX_ERANGE when one of them counted valid
// frames with non-finite logits; the report is consumed by the call that returns it.
static int range_poll(amx_handle h, bool wait) {
    // (one handle = one stream, include/allophant_amx.h: passes complete in issue order, so the slots are read oldest first and the
    // first one that is not ready ends the poll)
    int64_t total = 0;
    std::string readings;
    for (int i = 0; i < amx_handle_s::RANGE_SLOTS; ++i) {
        auto& sl = h->range[(h->range_next + i) % amx_handle_s::RANGE_SLOTS];  // oldest first
        if (!sl.pending) continue;
        if (wait) {
            HIPCHK(h, hipEventSynchronize(sl.ev));
        } else {
            const hipError_t q = hipEventQuery(sl.ev);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) { (void)hipGetLastError(); break; }
        }
        range_read(h, sl, total, readings);
    }
    if (h->range_carry > 0) {
        total += h->range_carry;
        readings += (readings.empty() ? "" : ", ") + h->range_carry_ids;
    }
    h->range_carry = 0;
    h->range_carry_ids.clear();
    if (total > 0)
        return fail(h, AMX_ERANGE, std::to_string(total) + " valid frame(s) of an EARLIER forward pass hold non-finite logits: an activation left the "
                                   "range of the 16-bit planes (fp16: |x| <= 65504) or the input was not finite; the outputs of that pass "
                                   "are not usable.  The bf16 planes (precision bf16x3) have the range of fp32; AMX_FLAG_NO_RANGE_CHECK "
                                   "turns this report off (frames per offending pass -- passes are numbered from 1 per handle, the one being "
                                   "issued now would be #" + std::to_string(h->pass_counter + 1) + " -- " + readings + ")");
    return AMX_OK;
}

// enqueues the count of the pass just issued on `s` into the next pinned slot
static int range_record(amx_handle h, bool cont, hipStream_t s) {
    auto& sl = h->range[h->range_next];
    if (!sl.host) {
        HIPCHK(h, hipHostMalloc((void**)&sl.host, 16));
        HIPCHK(h, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    }
    if (sl.pending) {
        // RANGE_SLOTS passes ago and never read since (the host ran that far ahead): wait for that pass and carry its count
        // into the next report instead of losing it
        HIPCHK(h, hipEventSynchronize(sl.ev));
        range_read(h, sl, h->range_carry, h->range_carry_ids);
    }
    HIPCHK(h, hipMemcpyAsync(sl.host, h->nonfinite, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipEventRecord(sl.ev, s));
    sl.pending = true;
    sl.cont = cont;
    sl.pass_id = h->pass_counter;
    h->range_next = (h->range_next + 1) % amx_handle_s::RANGE_SLOTS;
    return AMX_OK;
}


namespace {

// split-K workspace (fp32 partial slabs of products too small to fill the chip; see launch_gemm): the partials of one product never
// exceed CUs x 256 x 256 floats
constexpr size_t SPLITK_BYTES = (size_t)72 << 20;

// Everything amx_forward decides before it launches anything -- the PLAN of a pass: geometry, row layout, which optional forms the
// pass takes (packed rows, skipped conv tiles, the LayerNorm fold, the stream kept in planes), every buffer, the products of an
// encoder layer.  A plain value: plan_pass() fills it (and is the only place that may allocate, upload or synchronise),
// enqueue_pass() reads it and issues nothing but kernels -- eagerly on the caller's stream, or once on the capture stream when
// the pass is recorded into a HIP graph.  (Round 6: until then "plan + enqueue" was a lambda inside one 800-line function.)
struct PassPlan {
    // the call
    uint32_t flags = 0;
    int N = 0;
    int64_t L = 0;
    const float* d_audio = nullptr;
    float* d_out = nullptr;
    int64_t total = 0;
    // model shorthands
    int NT = 2, prec = 0, C = 0, D = 0, F = 0, H = 0, dh = 64, dhp = 64, E = 0, Eld = 0, cg = 0;
    // geometry
    int64_t Ts[AMX_MAX_CONV + 1] = {};
    int T = 0, Tp = 0, TpTot = 0, Tpad = 0;
    int64_t M = 0, Mp = 0, Mrows = 0, Mh = 0, rows1 = 0, rows2 = 0, xp_plane = 0, qk_plane = 0;
    size_t qkv_bytes = 0, qkv_zero_bytes = 0;  // (of each of Q / K / V: what the pass uses, what it zeroes first when needs_qkv_zero)
    // the forms the pass takes
    bool keep = false, masked = true, stable = true, blanks = true;
    bool packed = false, packed_early = false, ragged = false, window_ok = false, needs_qkv_zero = false;
    bool fold = false, stream_in_planes = false;
    // buffers (workspace of the handle: valid until a later plan grows one of them)
    void *d_len = nullptr, *d_frames = nullptr, *d_rowoff = nullptr, *d_partial = nullptr, *d_stats = nullptr, *actA = nullptr, *actB = nullptr,
         *preln = nullptr, *hbuf = nullptr, *xp = nullptr, *hg = nullptr, *qb = nullptr, *kb = nullptr, *vtb = nullptr, *ao = nullptr, *ff = nullptr,
         *hfin = nullptr, *logits = nullptr, *hpk = nullptr, *splitk = nullptr, *gn_partial = nullptr, *gn_scale = nullptr, *gn_shift = nullptr,
         *ebuf = nullptr, *cat = nullptr, *tl_x = nullptr, *tl_p = nullptr, *tl_qkv = nullptr, *ln_rowps = nullptr, *ln_coef = nullptr,
         *ln_partial = nullptr;
    const int* d_frames_enc = nullptr;
    int* d_tiles = nullptr;
    size_t tile_first[AMX_MAX_CONV + 1] = {};
    std::vector<float*> saved;   // per layer: where hidden state l is published (null: nobody reads it)
    float* conv_dbg = nullptr;
    float* hfin_rows = nullptr;
    float* stream = nullptr;     // the residual stream of the layers [Mrows, D]
    // host copies the tail of amx_forward keeps for amx_debug_fetch (packed_early only)
    std::vector<int> rowoff_host, frames_host;

    GemmParams with_ws(GemmParams g) const {
        g.splitk_ws = (float*)splitk;
        g.splitk_ws_elems = splitk ? (int64_t)(SPLITK_BYTES / 4) : 0;
        return g;
    }
    // ---- the attention of an encoder layer (the same for every layer) ----
    AttnParams attn_params() const {
        AttnParams a{};
        a.q = qb; a.k = kb; a.v = vtb;
        a.qk_plane = qk_plane;
        a.out = ao; a.out_plane = xp_plane;
        a.frame_len = d_frames_enc;
        a.N = N; a.H = H; a.T = T; a.Tp = packed ? TpTot : Tp; a.dh = dh; a.dhp = dhp;
        a.row_off = packed ? (const int*)d_rowoff : nullptr;
        a.order = packed ? (const int*)d_rowoff + N + 1 : nullptr;
        return a;
    }
    // ---- the products of an encoder layer ----
    GemmParams qkv_params(amx_handle h, const Layer& ly) const {
        GemmParams g{};
        g.A = xp; g.a_plane = xp_plane; g.lda = D; g.rows_per_batch = Mrows;
        g.W = ly.wqkv; g.w_plane = pln(h, (int64_t)3 * D * D); g.ldw = D;
        g.M = (int)Mrows; g.N = 3 * D; g.K = D;
        g.scale = ly.r_qkv; g.bias = ly.bqkv;
        g.mode = 1; g.q = qb; g.k = kb; g.v = vtb;
        g.qk_plane = qk_plane;
        // packed rows: one "utterance" of Mp rows, so the scatter writes row m of head hh to [hh][m][:]
        g.T = packed ? (int)std::max<int64_t>(Mp, 8) : T; g.Tp = packed ? TpTot : Tp; g.H = H; g.dh = dh; g.dhp = dhp;
        return with_ws(g);
    }
    GemmParams oproj_params(amx_handle h, const Layer& ly) const {
        GemmParams g{};
        g.A = ao; g.a_plane = xp_plane; g.lda = D; g.rows_per_batch = Mrows;
        g.W = ly.wo; g.w_plane = pln(h, (int64_t)D * D); g.ldw = D;
        g.M = (int)Mrows; g.N = D; g.K = D;
        g.scale = ly.r_o; g.bias = ly.bo;
        g.residual = stream; g.ldr = D; g.out_f32 = stream; g.ldo = D;
        return with_ws(g);
    }
    GemmParams ffn1_params(amx_handle h, const Layer& ly) const {
        GemmParams g{};
        g.A = xp; g.a_plane = xp_plane; g.lda = D; g.rows_per_batch = Mrows;
        g.W = ly.w1; g.w_plane = pln(h, (int64_t)F * D); g.ldw = D;
        g.M = (int)Mrows; g.N = F; g.K = D;
        g.scale = ly.r_1; g.bias = ly.b1; g.act = 1;
        g.out_p = ff; g.out_plane = pln(h, Mrows * F); g.ldp = F;
        return with_ws(g);
    }
    GemmParams ffn2_params(amx_handle h, const Layer& ly) const {
        GemmParams g{};
        g.A = ff; g.a_plane = pln(h, Mrows * F); g.lda = F; g.rows_per_batch = Mrows;
        g.W = ly.w2; g.w_plane = pln(h, (int64_t)D * F); g.ldw = F;
        g.M = (int)Mrows; g.N = D; g.K = F;
        g.scale = ly.r_2; g.bias = ly.b2;
        g.residual = stream; g.ldr = D; g.out_f32 = stream; g.ldo = D;
        return with_ws(g);
    }
    // LayerNorm fold (pre-LN layers; GemmParams.ln_partial / row_coef): the out-projection and FFN2 leave the planes and the row
    // statistics of the stream they have just updated, QKV and FFN1 apply the normalisation in their epilogues -- no LayerNorm
    // pass between the products of a layer.  Only where all four products run on the ping-pong kernel in one piece (batches
    // from a few thousand frames: every benchmark configuration); short batches keep the row pass -- with (1, 0) as its affine
    // part, since the weights hold gamma and beta either way -- fused with the split-K fix-up as before.
    GemmParams as_consumer(GemmParams g, const float* col_c) const {
        g.row_coef = (const float2*)ln_coef; g.col_c = col_c;
        return g;
    }
    // Two-plane modes (stream_in_planes): between the products of a layer the stream lives in its planes only -- a producer reads its
    // residual from them and writes fp32 rows only where something reads those (`f32`: a published hidden state, the last layer:
    // the final LayerNorm and the unpacking read fp32)
    GemmParams as_producer(GemmParams g, bool f32 = true) const {
        g.ln_partial = (float2*)ln_partial; g.ln_rowps = (const float4*)ln_rowps;
        g.out_p = xp; g.out_plane = xp_plane; g.ldp = D;
        if (stream_in_planes) {
            g.ln_res_planes = 1;
            g.residual = nullptr;
            if (!f32) g.out_f32 = nullptr;
        }
        return g;
    }
};

}  // namespace

// (re)allocates the pinned ring for batches of up to N utterances (waits for the stream: the old slots may be in use)
static int pin_reserve(amx_handle h, int N, hipStream_t s) {
    HIPCHK(h, hipStreamSynchronize(s));
    for (int i = 0; i < amx_handle_s::PIN_SLOTS; ++i) {
        if (h->h_lengths_pinned[i]) {
            (void)hipHostFree(h->h_lengths_pinned[i]);
            (void)hipHostFree(h->h_frames_pinned[i]);
            (void)hipHostFree(h->h_rowoff_pinned[i]);
        }
        HIPCHK(h, hipHostMalloc((void**)&h->h_lengths_pinned[i], (size_t)N * 8));
        HIPCHK(h, hipHostMalloc((void**)&h->h_frames_pinned[i], (size_t)N * 4));
        HIPCHK(h, hipHostMalloc((void**)&h->h_rowoff_pinned[i], (size_t)(3 * N + 1) * 4));  // offsets, the order, encoder frames
        if (!h->pin_event[i]) HIPCHK(h, hipEventCreateWithFlags(&h->pin_event[i], hipEventDisableTiming));
        h->pin_busy[i] = false;
    }
    h->pinned_cap = N;
    return AMX_OK;
}

// Ragged batch: per conv layer i >= 1 the ascending list of its 128-row output tiles that hold a row some utterance owns
// (`valid_rows`: [conv layer][n]), staged in pinned slot `slot` and uploaded behind the lengths
static int plan_conv_tiles(amx_handle h, PassPlan& P, int slot, const std::vector<int>& valid_rows, hipStream_t s) {
    const amx_config& c = h->cfg;
    const int N = P.N;
    size_t total_tiles = 0;
    constexpr int64_t TR = GEMM_LN_TILE_ROWS;
    for (int i = 1; i < c.n_conv; ++i) total_tiles += (size_t)((N * P.Ts[i + 1] + TR - 1) / TR);
    if (h->tiles_cap[slot] < total_tiles) {  // the slot is idle: plan_pass waited for its event
        if (h->h_tiles_pinned[slot]) (void)hipHostFree(h->h_tiles_pinned[slot]);
        h->h_tiles_pinned[slot] = nullptr;
        h->tiles_cap[slot] = 0;
        HIPCHK(h, hipHostMalloc((void**)&h->h_tiles_pinned[slot], (total_tiles + total_tiles / 4 + 64) * 4));
        h->tiles_cap[slot] = total_tiles + total_tiles / 4 + 64;
    }
    int* list = h->h_tiles_pinned[slot];
    size_t count = 0;
    for (int i = 1; i < c.n_conv; ++i) {
        P.tile_first[i] = count;
        const int64_t rpb = P.Ts[i + 1], rows = N * rpb;
        const int* valid = valid_rows.data() + (size_t)i * N;
        for (int64_t first = 0; first < rows; first += TR) {
            const int64_t last = std::min(first + TR, rows) - 1;
            const int64_t b0 = first / rpb, b1 = last / rpb;
            if (b0 != b1 || first - b0 * rpb < valid[b0]) list[count++] = (int)(first / TR);
        }
    }
    P.tile_first[c.n_conv] = count;
    void* p;
    if (int rc = ws_get(h, "conv_tiles", std::max<size_t>(count, 1) * 4, &p)) return rc;
    P.d_tiles = (int*)p;
    HIPCHK(h, hipMemcpyAsync(P.d_tiles, list, count * 4, hipMemcpyHostToDevice, s));
    return AMX_OK;
}

// the concatenation recipe of every classifier with dependencies: source pointers / logit columns of this pass
static int plan_concat(amx_handle h, const PassPlan& P, hipStream_t s) {
    for (auto& st : h->steps) {
        if (st.direct_output) continue;
        for (size_t i = 0; i < st.parts.size(); ++i) {
            int dep = st.part_dep[i];
            if (dep < 0) {
                st.parts[i].src = dep == AMX_DEP_OUTPUT ? P.hfin_rows : P.saved[-2 - dep];
            } else {
                st.parts[i].src_col = h->col[dep] + (P.blanks ? 0 : 1);
                // a composed dependency has an inventory-dependent width; the classifier was trained on the training
                // inventory, so the widths must agree
                int w = h->width[dep] - (P.blanks ? 0 : 1);
                if (w != st.parts[i].width)
                    return fail(h, AMX_EINVAL, "inventory size does not match the input width of a dependent classifier");
            }
        }
        if (st.parts_uploaded.size() != st.parts.size() ||
            memcmp(st.parts_uploaded.data(), st.parts.data(), st.parts.size() * sizeof(ConcatPart)) != 0) {
            // the recipe only changes with the workspace pointers or the inventory; st.parts is pageable host memory,
            // so this (rare) upload completes before the call goes on.  A captured graph never holds it: parts_dev is
            // read by the concat kernel, and a changed recipe comes with a changed workspace generation or inventory.
            HIPCHK(h, hipMemcpyAsync(st.parts_dev, st.parts.data(), st.parts.size() * sizeof(ConcatPart), hipMemcpyHostToDevice, s));
            HIPCHK(h, hipStreamSynchronize(s));
            st.parts_uploaded = st.parts;
        }
    }
    return AMX_OK;
}

// The plan region of a forward pass (see PassPlan): argument and geometry checks, pinned uploads of lengths / frame counts / row
// offsets / tile lists, every workspace buffer (ws_get may allocate, free and synchronise), the concatenation recipes of dependent
// classifiers, and the decisions that depend on the lengths.
static int plan_pass(amx_handle h, const float* audio, const int64_t* lengths, int N, int64_t L, float* out, int64_t* out_lengths,
                     uint32_t flags, hipStream_t s, PassPlan& P) {
    int rc;
    const amx_config& c = h->cfg;
    h->timing = (flags & AMX_FLAG_TIMING) != 0;
    h->timing_stream = s;
    P.flags = flags; P.N = N; P.L = L;
    P.keep = (flags & AMX_FLAG_KEEP_HIDDEN) != 0;
    P.NT = h->NT; P.prec = h->prec; P.C = c.conv_dim; P.D = c.hidden; P.F = c.ffn; P.H = c.heads;
    const int NT = P.NT, C = P.C, D = P.D, F = P.F, H = P.H;

    P.T = (int)conv_lengths(c, L, P.Ts);
    P.M = (int64_t)N * P.T;
    {
        const int64_t nmax = max_utterances_for(c, NT, L);
        if (N > nmax)
            return fail(h, AMX_EINVAL, "batch too large for the 32-bit offsets of the kernels: at most " + std::to_string(nmax) +
                                           " utterances of " + std::to_string(L) + " samples per call (amx_max_utterances); split the batch");
    }
    P.Tp = round_up(P.T, 64);

    int64_t maxlen = 0;
    for (int n = 0; n < N; ++n) {
        if (lengths[n] < 1 || lengths[n] > L) return fail(h, AMX_EINVAL, "lengths must lie in [1, L]");
        maxlen = std::max(maxlen, lengths[n]);
    }
    if (maxlen != L && !(flags & AMX_FLAG_PADDED))
        return fail(h, AMX_EINVAL, "the batch must be padded to exactly max(lengths) (reference utils.py:62-63, acoustic_model.py:765-767)");

    // ---- pinned host staging of lengths (ring of event-guarded slots: no stream synchronisation on the hot path) ----
    if (h->pinned_cap < N && (rc = pin_reserve(h, N, s))) return rc;
    const int slot = h->pin_next;
    h->pin_next = (h->pin_next + 1) % amx_handle_s::PIN_SLOTS;
    if (h->pin_busy[slot]) HIPCHK(h, hipEventSynchronize(h->pin_event[slot]));  // its copies ran PIN_SLOTS calls ago
    int64_t* pin_len = h->h_lengths_pinned[slot];
    int* pin_frames = h->h_frames_pinned[slot];
    int* pin_rowoff = h->h_rowoff_pinned[slot];
    std::vector<int> conv_rows((size_t)c.n_conv * N);  // [conv layer][n]: valid output rows
    P.Mp = 0;  // valid frames of the batch = rows of the packed layout
    for (int n = 0; n < N; ++n) {
        pin_len[n] = lengths[n];
        int64_t rows_n[AMX_MAX_CONV + 1];
        const int64_t f = conv_lengths(c, lengths[n], rows_n);
        for (int i = 0; i < c.n_conv; ++i) conv_rows[(size_t)i * N + n] = (int)rows_n[i + 1];
        if (f < 1) return fail(h, AMX_EINVAL, "utterance shorter than the receptive field of the feature extractor");
        pin_frames[n] = (int)f;
        pin_rowoff[n] = (int)P.Mp;
        P.Mp += f;
        if (out_lengths) out_lengths[n] = f;
    }
    pin_rowoff[N] = (int)P.Mp;
    {   // utterances by descending length (ties by index): the order the packed attention dispatches them in
        int* order = pin_rowoff + N + 1;
        for (int n = 0; n < N; ++n) order[n] = n;
        std::stable_sort(order, order + N, [&](int a, int b) { return pin_frames[a] > pin_frames[b]; });
    }
    // The frames the ENCODER treats as valid: the utterance's own, or -- a model whose preprocessor has
    // return_attention_mask = False is called with attention_mask=None (acoustic_model.py:814,842-846) -- every frame of the
    // padded length: nothing is zeroed, every key is attended to.  `Predictions.lengths` are the utterance's own either way.
    P.masked = h->masked;
    for (int n = 0; n < N; ++n) pin_rowoff[2 * N + 1 + n] = P.masked ? pin_frames[n] : P.T;
    if (!P.masked) P.Mp = P.M;  // no padding as far as the encoder is concerned: nothing to pack, nothing to skip

    // ---- workspace ----
    P.cg = D / c.pos_groups;
    P.Tpad = P.T + c.pos_kernel;
    P.rows1 = (int64_t)N * P.Ts[1];
    P.rows2 = (int64_t)N * P.Ts[2];
#define WS(name, bytes, ptr) do { if ((rc = ws_get(h, name, (size_t)(bytes), &ptr))) return rc; } while (0)
    // split-K workspace (fp32 partial slabs of products too small to fill the chip; see launch_gemm): the partials of one
    // product never exceed CUs x 256 x 256 floats
    WS("splitk", SPLITK_BYTES, P.splitk);
    WS("len", (size_t)N * 8, P.d_len);
    WS("frames", (size_t)N * 4, P.d_frames);
    WS("rowoff", (size_t)(3 * N + 1) * 4, P.d_rowoff);
    P.d_frames_enc = (const int*)P.d_rowoff + 2 * N + 1;
    WS("partial", (size_t)N * 64 * 3 * 8, P.d_partial);
    WS("stats", (size_t)N * 2 * 4, P.d_stats);
    WS("actA", (size_t)P.rows1 * C * 2 * NT + PLANE_SLACK, P.actA);
    WS("actB", (size_t)P.rows2 * C * 2 * NT + PLANE_SLACK, P.actB);
    WS("preln", (size_t)P.rows2 * C * 4, P.preln);
    WS("h", (size_t)P.M * D * 4, P.hbuf);
    WS("xp", (size_t)P.M * D * 2 * NT + PLANE_SLACK, P.xp);
    WS("hg", (size_t)N * P.Tpad * D * 2 * NT, P.hg);
    // head dimension and the width of a Q / K / V row: 64 columns, 128 for heads wider than that (the columns beyond dh stay zero:
    // the buffers are zero-filled when they are created and the QKV scatter writes the dh real columns only)
    P.dh = D / H;
    P.dhp = P.dh > 64 ? 128 : 64;
    P.qkv_bytes = (size_t)N * H * P.Tp * P.dhp * 2 * NT;
    if ((rc = ws_get(h, "q", P.qkv_bytes, &P.qb, true))) return rc;
    if ((rc = ws_get(h, "k", P.qkv_bytes, &P.kb, true))) return rc;
    if ((rc = ws_get(h, "vt", P.qkv_bytes, &P.vtb, true))) return rc;
    WS("ao", (size_t)P.M * D * 2 * NT + PLANE_SLACK, P.ao);
    WS("ff", (size_t)P.M * F * 2 * NT + PLANE_SLACK, P.ff);
    WS("hfin", (size_t)P.M * D * 4, P.hfin);
    WS("logits", (size_t)P.M * h->ld_logits * 4, P.logits);
    // Packed rows: a ragged batch runs its encoder layers on the valid frames only (rows of utterance n at row_off[n], all
    // utterances back to back): every kernel of a layer is row-wise except the attention, which takes the offsets.  A row's
    // arithmetic does not depend on its position, so the valid frames come out as in the padded layout (the same bits when
    // the products pick the same kernels for the smaller row count, within rounding of the K-chunk order otherwise).  Used
    // when at least a tenth of the padded rows are padding (not under AMX_FLAG_KEEP_HIDDEN: the debug capture wants every hidden
    // state in the padded layout, padding included); AMX_FLAG_NO_PACK keeps the padded layout.
    P.TpTot = round_up((int)P.Mp, 64) + 64;  // rows per head of the packed Q / K / V planes
    P.packed = !(flags & AMX_FLAG_NO_PACK) && !P.keep && D % 4 == 0 && P.Mp * 10 <= P.M * 9 &&
               (int64_t)P.TpTot <= (int64_t)N * P.Tp;
    // Packed from the feature projection on ("early"): the last conv layer's LayerNorm pass gathers the valid frames, so the
    // feature projection, the positional convolution (window kernel: skips the frame blocks beyond an utterance), the final
    // LayerNorm, the classifier heads and the log-softmax read packed rows too and nothing is packed or unpacked in between.
    // Needs the window kernel (the grouped-GEMM form of the positional convolution addresses padded rows) and no time-layer
    // head (its attention walks (utterance, frame) pairs); otherwise the rows are packed after the positional convolution
    // and unpacked before the final LayerNorm, as in round 2.
    P.window_ok = posconv_window_eligible(D, c.pos_groups, c.pos_kernel, N, P.T, P.Tpad, (int64_t)N * P.Tpad * D);
    bool any_time_layer = false;
    for (auto& st : h->steps) any_time_layer |= st.time_heads > 0;
    // (the post-LN encoder has no LayerNorm pass between its last layer and the heads to unpack behind: it packs early or not at all)
    if (!h->stable && !(P.window_ok && !any_time_layer)) P.packed = false;
    P.packed_early = P.packed && P.window_ok && !any_time_layer;
    if (P.packed) WS("h_packed", (size_t)P.Mp * D * 4, P.hpk);
    P.d_audio = audio;
    P.d_out = out;
    P.total = layout_total(h, N, P.T);
    if (flags & AMX_FLAG_HOST_IO) {
        void *a, *o;
        WS("audio_host_io", (size_t)N * L * 4, a);
        WS("out_host_io", (size_t)P.total * 4, o);
        HIPCHK(h, hipMemcpyAsync(a, audio, (size_t)N * L * 4, hipMemcpyHostToDevice, s));
        P.d_audio = (const float*)a;
        P.d_out = (float*)o;
    }
    P.saved.assign(c.layers + 1, nullptr);
    for (int l = 0; l < c.layers; ++l)
        if (P.keep || h->need_hidden[l]) {
            void* p;
            std::string nm = "hid" + std::to_string(l);
            WS(nm.c_str(), (size_t)P.M * D * 4, p);
            P.saved[l] = (float*)p;
        }
    if (P.keep) {
        void* p;
        WS("conv_dbg", (size_t)P.M * C * 4, p);
        P.conv_dbg = (float*)p;
    }

    HIPCHK(h, hipMemcpyAsync(P.d_len, pin_len, (size_t)N * 8, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(P.d_frames, pin_frames, (size_t)N * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(P.d_rowoff, pin_rowoff, (size_t)(3 * N + 1) * 4, hipMemcpyHostToDevice, s));
    // Ragged batch: the conv stack skips what lies wholly in an utterance's padding (conv0: frame blocks; the row-complete
    // layers 1..n-2: 128-row tiles).  A valid frame of any layer only reads valid frames of the layer below, and the rows
    // left unwritten (stale, possibly non-finite) stay inside padded rows until the feature projection zeroes those.
    // (only from a tenth of padding on -- the threshold of the packed rows: below it the padded frames are simply computed, and
    // NOTHING of the pass depends on the lengths by value any more -- lengths, frame counts and masks are device buffers the plan
    // refreshes -- so a recording of this (N, L) geometry serves every batch of that geometry: see graph_key)
    P.ragged = P.Mp < P.M && P.Mp * 10 <= P.M * 9 && !P.keep && !(flags & AMX_FLAG_NO_PACK);
    if (P.ragged && (rc = plan_conv_tiles(h, P, slot, conv_rows, s))) return rc;
    HIPCHK(h, hipEventRecord(h->pin_event[slot], s));
    h->pin_busy[slot] = true;

    // ---- the rest of the plan: every buffer and host-side table the pass needs exists before anything is enqueued, so that
    // enqueue_pass issues nothing but memsets, kernels and device copies (which is what a HIP graph may hold) ----
    if (h->gn) {
        WS("gn_partial", h->c0.gn_partial_bytes(N, (int)P.Ts[1]), P.gn_partial);
        WS("gn_scale", (size_t)N * C * 4, P.gn_scale);
        WS("gn_shift", (size_t)N * C * 4, P.gn_shift);
    }
    P.stable = h->stable;
    P.Mh = P.packed_early ? P.Mp : P.M;  // rows of the final LayerNorm and of the classifier heads
    // hidden_states[layers]: the final LayerNorm's fp32 rows; post-LN encoder: the stream as the last layer left it (kept in
    // a buffer of its own only for the debug capture)
    P.hfin_rows = (P.stable || P.keep) ? (float*)P.hfin : (float*)(P.packed ? P.hpk : P.hbuf);
    P.saved[c.layers] = P.hfin_rows;
    P.E = c.embedding_size;
    int kcat = 0;
    for (auto& st : h->steps) kcat = std::max(kcat, st.direct_output ? 0 : st.Kpad);
    P.Eld = round_up(P.E, kalign(h));  // row stride of the embedding planes (pad columns are never read: K = E)
    if (P.E > 0) WS("e", (size_t)P.M * P.Eld * 2 * NT + PLANE_SLACK, P.ebuf);
    if (kcat > 0) WS("cat", (size_t)P.M * kcat * 2 * NT + PLANE_SLACK, P.cat);
    {
        int cmax = 0;
        for (auto& st : h->steps)
            if (st.time_heads > 0) {
                cmax = std::max(cmax, st.Cpad);
                if (st.rows / st.time_heads > 4096)
                    return fail(h, AMX_EINVAL, "head_dim of a time-layer classifier beyond 4096");
            }
        if (cmax > 0) {
            WS("tl_x", (size_t)P.M * cmax * 4, P.tl_x);
            WS("tl_p", (size_t)P.M * cmax * 2 * NT + PLANE_SLACK, P.tl_p);
            WS("tl_qkv", (size_t)P.M * cmax * 3 * 4, P.tl_qkv);
        }
    }
    P.blanks = c.dependency_blanks != 0;
    if ((rc = plan_concat(h, P, s))) return rc;
    P.needs_qkv_zero = !P.packed && (h->last_N != N || h->last_T != P.T || h->qkv_dirty);
    P.qkv_zero_bytes = P.qkv_bytes;
    if (h->qkv_pad_dirty && P.dh != P.dhp) {
        // the pad columns of a row are never written, in either row layout, and packed rows of a later, larger batch lie anywhere
        // in the allocation: all of it (the three buffers are asked for together, so they are of one size)
        P.needs_qkv_zero = true;
        P.qkv_zero_bytes = std::min({h->ws["q"].bytes, h->ws["k"].bytes, h->ws["vt"].bytes}) / 4 * 4;
    }
    P.Mrows = P.packed ? P.Mp : P.M;  // rows the layers work on
    P.xp_plane = pln(h, P.Mrows * D);
    P.qk_plane = P.packed ? (int64_t)H * P.TpTot * P.dhp : (int64_t)N * H * P.Tp * P.dhp;
    P.stream = (float*)(P.packed ? P.hpk : P.hbuf);
    if (P.packed_early) {
        P.rowoff_host.assign(pin_rowoff, pin_rowoff + N);
        P.frames_host.assign(pin_frames, pin_frames + N);
    }
    // LayerNorm fold: decided on the products as they will be launched
    P.stream_in_planes = NT == 2;
    // (not with attention adapters: the adapter would have to sit inside the fold's producer / consumer chain -- FFN2 leaves planes
    // and statistics of a stream the adapter then changes.  Adapter models keep the row passes, the adapter writing one of them.)
    if (P.stable && c.layers > 0 && D % 64 == 0 && D <= 2048 && !h->adapter) {
        WS("ln_rowps", (size_t)P.Mrows * 16, P.ln_rowps);
        WS("ln_coef", (size_t)P.Mrows * 8, P.ln_coef);
        WS("ln_partial", (size_t)P.Mrows * (D / 64) * 8, P.ln_partial);
        const Layer& ly = h->layers[0];
        const int prec = P.prec;
        // (the producers as enqueue_pass launches them: the out-projection without fp32 rows, FFN2 with and without)
        P.fold = gemm_ln_fold_ok(prec, P.as_consumer(P.qkv_params(h, ly), ly.c_qkv)) &&
                 gemm_ln_fold_ok(prec, P.as_producer(P.oproj_params(h, ly), false)) &&
                 gemm_ln_fold_ok(prec, P.as_consumer(P.ffn1_params(h, ly), ly.c_1)) &&
                 gemm_ln_fold_ok(prec, P.as_producer(P.ffn2_params(h, ly), false)) &&
                 gemm_ln_fold_ok(prec, P.as_producer(P.ffn2_params(h, ly), true));
    }
    ++h->pass_counter;
    h->last_fold = P.fold;
    h->last_packed = P.packed_early ? 2 : (P.packed ? 1 : 0);
    h->last_attention = c.layers > 0 ? attention_form(P.attn_params()) : -1;
    h->last_rows = P.Mrows;
    h->last_graph = 0;
#undef WS
    return AMX_OK;
}

// The enqueue region: the whole pass on stream `s` -- kernels only (zero fills and device copies are kernels too: amx_rowops.hip,
// launch_zero), nothing that allocates, uploads or synchronises.
static int enqueue_pass(amx_handle h, const PassPlan& P, hipStream_t s) {
    const amx_config& c = h->cfg;
    const int prec = P.prec, N = P.N, C = P.C, D = P.D, T = P.T;
    const int64_t M = P.M, Mh = P.Mh;
    void* hbuf = P.hbuf;  // the residual stream: the layers switch it to the packed rows and back
    // Every GEMM of the pass: split-K workspace, timed under its kernel class (the one launch_gemm picks unless the caller names
    // one), refusals recorded.  launch_gemm refuses fold products only, and P.fold checked those with these very params.
    bool refused = false;
    auto gemm = [&](const GemmParams& g, int cls = -1) {
        Timed t_(h, cls < 0 ? gemm_class(prec, g) : cls);
        refused |= !launch_gemm(prec, P.with_ws(g), s);
    };
    // K/V/Q padding rows [T, Tp) must stay finite: re-zero when the geometry changes
    // (zero fills inside a pass are kernels, never memsets: amx_rowops.hip, launch_zero)
    if (P.needs_qkv_zero) {
        launch_zero(P.qb, P.qkv_zero_bytes, s);
        launch_zero(P.kb, P.qkv_zero_bytes, s);
        launch_zero(P.vtb, P.qkv_zero_bytes, s);
    }
    if (P.packed) {
        // rows [Mp, TpTot) of every head are read (never used) by the last key tile and query block: keep them finite
        const size_t row_b = (size_t)P.dhp * 2, tail = (size_t)(P.TpTot - P.Mp) * row_b, pitch = (size_t)P.TpTot * row_b;
        for (void* buf : {P.qb, P.kb, P.vtb})  // the planes lie back to back: NT * H blocks of TpTot rows
            launch_zero_2d((char*)buf + (size_t)P.Mp * row_b, pitch, tail, (size_t)P.NT * P.H, s);
    }
    // amx_check_finite reports on THIS forward pass; the later slices of one over-long batch (AMX_FLAG_CONTINUE) add up
    if (!(P.flags & AMX_FLAG_CONTINUE)) launch_zero(h->nonfinite, 4, s);
    // ---- input normalisation statistics + conv layer 0 (fused norm + conv + LN + GELU) ----
    { Timed t_(h, AMX_KC_OTHER); launch_audio_stats(P.d_audio, (const int64_t*)P.d_len, N, P.L, (double*)P.d_partial, (float*)P.d_stats, c.do_normalize, s); }
    {
        // (group-norm variant: GroupNorm statistics over ALL frames of the padded length -- upstream normalises the padded batch
        // tensor --, then conv + affine + GELU; frame blocks in an utterance's padding may still be skipped in the second pass)
        Conv0Args a{};
        a.audio = P.d_audio; a.lengths = (const int64_t*)P.d_len; a.mean_rstd = (const float*)P.d_stats;
        a.N = N; a.L = P.L; a.T1 = (int)P.Ts[1]; a.C = C; a.k = c.conv_kernel[0]; a.stride = c.conv_stride[0];
        a.w = h->c0_w; a.b = h->conv_b[0]; a.gamma = h->conv_g[0]; a.beta = h->conv_be[0];
        a.eps = 1e-5f; a.do_normalize = c.do_normalize;
        a.table = h->c0_stats; a.w_scale = h->c0_wscale;
        a.gn_partial = (double*)P.gn_partial; a.gn_scale = (float*)P.gn_scale; a.gn_shift = (float*)P.gn_shift;
        a.out = P.actA; a.out_plane = pln(h, P.rows1 * C); a.skip_padding = P.ragged ? 1 : 0;
        Timed t_(h, AMX_KC_CONV0);
        launch_conv0(h->c0, a, s);
    }
    // ---- conv layers 1..n-1: implicit GEMM over overlapping channels-last windows, then LN + GELU rows ----
    void* cur = P.actA;
    int64_t cur_plane = pln(h, P.rows1 * C);
    void* other = P.actB;
    for (int i = 1; i < c.n_conv; ++i) {
        const int64_t rows_out = (int64_t)N * P.Ts[i + 1];
        GemmParams g{};
        g.A = cur; g.a_plane = cur_plane; g.lda = (int64_t)c.conv_stride[i] * C; g.rows_per_batch = P.Ts[i + 1];
        g.a_batch_stride = P.Ts[i] * C;
        g.W = h->conv_w[i]; g.w_plane = pln(h, (int64_t)C * C * c.conv_kernel[i]); g.ldw = (int64_t)C * c.conv_kernel[i];
        g.M = (int)rows_out; g.N = C; g.K = C * c.conv_kernel[i];
        g.scale = h->conv_r[i]; g.bias = h->conv_b[i];
        if (P.ragged) {  // honoured by the row-complete kernel only
            g.tile_list = P.d_tiles + P.tile_first[i];
            g.n_tiles = (int)(P.tile_first[i + 1] - P.tile_first[i]);
        }
        const bool last = i == c.n_conv - 1;
        const int64_t out_plane = pln(h, rows_out * C);
        if (h->gn) {
            // group-norm variant: conv + GELU, no norm (Wav2Vec2NoLayerNormConvLayer): the GELU sits in the product's epilogue
            g.act = 1;
            g.tile_list = nullptr; g.n_tiles = 0;
            if (!last) {
                g.out_p = other; g.out_plane = out_plane; g.ldp = C;
                gemm(g);
            } else {
                // last layer: fp32 GELU output, then the feature-projection LayerNorm -> planes (packed_early: valid frames only)
                g.out_f32 = P.keep ? P.conv_dbg : (float*)P.preln; g.ldo = C;
                gemm(g, AMX_KC_CONV_TAIL);
                Timed t_(h, AMX_KC_CONV_TAIL);
                if (P.packed_early)
                    launch_rownorm_to_packed(prec, g.out_f32, C, rows_out, C, nullptr, nullptr, 0, h->fp_g, h->fp_b, 0.f, c.eps, other,
                                             out_plane, C, (const int*)P.d_rowoff, (const int*)P.d_frames, T, s);
                else
                    launch_rownorm(prec, g.out_f32, C, rows_out, C, nullptr, nullptr, 0, h->fp_g, h->fp_b, 0.f, c.eps, other, out_plane,
                                   C, nullptr, 0, s);
            }
            std::swap(cur, other);
            cur_plane = out_plane;
            continue;
        }
        if (!last) {
            // LayerNorm + GELU fused into the GEMM epilogue when the row-complete kernel takes the shape (C == 512)
            GemmParams f = g;
            f.act = 1; f.ln_gamma = h->conv_g[i]; f.ln_beta = h->conv_be[i]; f.ln_eps = 1e-5f;
            f.out_p = other; f.out_plane = out_plane; f.ldp = C;
            if (gemm_fuses_ln(prec, f)) {
                if (h->conv_w_tm[i] && gemm_ln_tap_minor_slice(prec, f) == h->conv_tm_slice) {
                    // tap-minor K order: the input row two output rows share is fetched in adjacent slices (an L2 hit)
                    f.W = h->conv_w_tm[i];
                    f.a_taps = c.conv_kernel[i];
                    f.a_tap_stride = C;
                }
                gemm(f, AMX_KC_GEMM_LN);
                std::swap(cur, other);
                cur_plane = out_plane;
                continue;
            }
        }
        g.out_f32 = (float*)P.preln; g.ldo = C;
        gemm(g, last ? AMX_KC_CONV_TAIL : gemm_class(prec, g));
        if (!last) {
            { Timed t_(h, AMX_KC_ROWNORM); launch_rownorm(prec, (const float*)P.preln, C, rows_out, C, h->conv_g[i], h->conv_be[i], 1, nullptr, nullptr, 1e-5f,
                           0.f, other, out_plane, C, nullptr, 0, s); }
        } else if (!P.keep) {
            // last conv layer: LN + GELU, then the feature-projection LayerNorm in the same pass (packed_early: only the valid
            // frames, written back to back)
            Timed t_(h, AMX_KC_CONV_TAIL);
            if (P.packed_early)
                launch_rownorm_to_packed(prec, (const float*)P.preln, C, rows_out, C, h->conv_g[i], h->conv_be[i], 1, h->fp_g, h->fp_b, 1e-5f,
                                         c.eps, other, out_plane, C, (const int*)P.d_rowoff, (const int*)P.d_frames, T, s);
            else
                launch_rownorm(prec, (const float*)P.preln, C, rows_out, C, h->conv_g[i], h->conv_be[i], 1, h->fp_g, h->fp_b, 1e-5f,
                               c.eps, other, out_plane, C, nullptr, 0, s);
        } else {
            { Timed t_(h, AMX_KC_ROWNORM); launch_rownorm(prec, (const float*)P.preln, C, rows_out, C, h->conv_g[i], h->conv_be[i], 1, nullptr, nullptr, 1e-5f,
                           0.f, nullptr, 0, 0, P.conv_dbg, C, s); }
            { Timed t_(h, AMX_KC_ROWNORM); launch_rownorm(prec, P.conv_dbg, C, rows_out, C, h->fp_g, h->fp_b, 0, nullptr, nullptr, c.eps, 0.f, other, out_plane,
                           C, nullptr, 0, s); }
        }
        std::swap(cur, other);
        cur_plane = out_plane;
    }
    // ---- feature projection (+ zero padded frames) ----
    {
        GemmParams g{};
        const int64_t Mfp = P.packed_early ? P.Mp : M;  // packed_early: the valid frames only, no row mask needed
        g.A = cur; g.a_plane = cur_plane; g.lda = C; g.rows_per_batch = Mfp; g.a_batch_stride = 0;
        g.W = h->fp_w; g.w_plane = pln(h, (int64_t)D * C); g.ldw = C;
        g.M = (int)Mfp; g.N = D; g.K = C;
        g.scale = h->fp_r; g.bias = h->fp_bias;
        if (!P.packed_early && P.masked) { g.row_len = (const int*)P.d_frames; g.rows_T = T; }  // hidden_states[~mask] = 0
        g.out_f32 = (float*)(P.packed_early ? P.hpk : hbuf); g.ldo = D;
        gemm(g);
    }
    // ---- positional conv embedding: h += GELU(grouped conv(h)) ----
    {
        const int cg = P.cg, Tpad = P.Tpad;
        const int* pk_off = P.packed_early ? (const int*)P.d_rowoff : nullptr;
        const int* pk_len = P.packed_early ? (const int*)P.d_frames : nullptr;
        float* hcur = (float*)(P.packed_early ? P.hpk : hbuf);
        { Timed t_(h, AMX_KC_OTHER); launch_posconv_pack(prec, hcur, N, T, D, c.pos_groups, c.pos_kernel / 2, Tpad, P.hg,
                            (int64_t)N * Tpad * D, pk_off, pk_len, s); }
        // the window kernel where it takes the shape, the grouped implicit GEMM on the tile kernels otherwise
        if (P.window_ok) {
            Timed t_(h, AMX_KC_GEMM_TILE);
            launch_posconv_window(prec, P.hg, (int64_t)N * Tpad * D, h->pos_w, (int64_t)D * cg * c.pos_kernel,
                                  (int64_t)cg * c.pos_kernel, h->pos_b, h->pos_r, hcur, N, T, Tpad, D, c.pos_groups, c.pos_kernel,
                                  pk_off, pk_len, s);
        } else {
            GemmParams g{};
            g.A = P.hg; g.a_plane = (int64_t)N * Tpad * D; g.lda = cg; g.rows_per_batch = T; g.a_batch_stride = (int64_t)Tpad * cg;
            g.za = (int64_t)N * Tpad * cg;
            g.W = h->pos_w; g.w_plane = (int64_t)D * cg * c.pos_kernel; g.ldw = (int64_t)cg * c.pos_kernel;
            g.zw = (int64_t)cg * cg * c.pos_kernel;
            g.M = (int)M; g.N = cg; g.K = cg * c.pos_kernel;
            g.scale = h->pos_r; g.bias = h->pos_b; g.zbias = cg; g.act = 1;
            g.residual = (const float*)hbuf; g.ldr = D; g.out_f32 = (float*)hbuf; g.ldo = D; g.zout = cg;
            { Timed t_(h, AMX_KC_GEMM_TILE); launch_gemm_grouped(prec, g, c.pos_groups, s); }
        }
    }
    // ---- transformer encoder (pre-LN) ----
    void* const hpad = hbuf;     // the padded residual stream [N * T, D]
    if (P.packed) {
        if (!P.packed_early) { Timed t_(h, AMX_KC_OTHER); launch_pack_rows((const float*)hpad, (float*)P.hpk, (const int*)P.d_rowoff, (const int*)P.d_frames, N, T, D, false, s); }
        hbuf = P.hpk;
    }
    // A residual product that launch_gemm cuts into K chunks (short batches) leaves its fix-up -- slab sum + bias + residual
    // -> h -- to the LayerNorm that follows it: one kernel instead of the fix-up and a LayerNorm pass that re-reads h.
    struct { bool on = false; GemmParams g; int splits = 0; } pending;
    auto residual_gemm = [&](GemmParams g, bool may_defer) {
        const int splits = may_defer ? gemm_planned_splits(prec, g) : 1;
        if (splits > 1 && fixup_rownorm_eligible(g)) {
            g.defer_fixup = 1;
            pending.on = true;
            pending.g = g;
            pending.splits = splits;
        }
        gemm(g);
    };
    // LayerNorm of the residual stream (rows of hbuf) -> planes (and the fp32 rows, for the final one)
    auto stream_norm = [&](const float* gamma, const float* beta, int64_t rows, int64_t plane, float* out_ln) {
        Timed t_(h, AMX_KC_ROWNORM);
        if (pending.on) {
            launch_fixup_rownorm(prec, pending.g, pending.splits, gamma, beta, c.eps, P.xp, plane, D, out_ln, D, s);
            pending.on = false;
        } else {
            launch_rownorm(prec, (const float*)hbuf, D, rows, D, gamma, beta, 0, nullptr, nullptr, c.eps, 0.f, P.xp, plane, D, out_ln, D, s);
        }
    };
    // post-LN encoder (Wav2Vec2Encoder): h = LayerNorm(h + pos_conv(h)) first; every layer is h = LN1(h + attention(h)),
    // h = LN2(h + FFN(h)); hidden_states[layers] is the last layer's output as it is.  The LayerNorm passes write the fp32
    // rows back in place (the residual stream IS the normalised tensor) next to the planes the products read.
    float* const ln_inplace = P.stable ? nullptr : (float*)hbuf;
    if (!P.stable) stream_norm(h->fln_g, h->fln_b, P.Mrows, P.xp_plane, ln_inplace);
    // (pre-LN layers: gamma / beta of both norms live in the QKV / FFN1 weights -- fold_layer_norm at amx_create -- so a row pass
    // normalises with (1, 0))
    // the fold's padded frames (padded layout of a ragged batch, keys the attention masks) are written under a smaller scale: see
    // ln_plane_scale.  Without the attention mask every frame is a key, and none is padding.
    const int* const fold_frames = P.packed || !P.masked ? nullptr : P.d_frames_enc;
    auto ln_finalize = [&]() {
        Timed t_(h, AMX_KC_ROWNORM);
        launch_ln_finalize((const float2*)P.ln_partial, D / 64, P.Mrows, c.eps, (float4*)P.ln_rowps, (float2*)P.ln_coef, fold_frames, T, s);
    };
    for (int l = 0; l < c.layers; ++l) {
        const Layer& ly = h->layers[l];
        if (P.fold) {
            // the first norm of the stack from the stream itself; later ones: the previous FFN2 left planes and statistics
            if (l == 0) {
                Timed t_(h, AMX_KC_ROWNORM);
                launch_ln_rowprep(prec, (const float*)hbuf, D, P.Mrows, D, c.eps, P.xp, P.xp_plane, D, (float4*)P.ln_rowps, (float2*)P.ln_coef,
                                  fold_frames, T, s);
            }
        } else if (P.stable && !(h->adapter && l > 0)) {
            // (completes the previous layer's FFN2 when that was deferred; behind an attention adapter the planes are there already)
            stream_norm(h->unit_g, h->zero_b, P.Mrows, P.xp_plane, nullptr);
        }
        if (P.saved[l]) {
            // a classifier reads hidden state l (OUTPUT_l, acoustic_model.py:478-483): padded layout; with packed rows the padded
            // frames take their pre-encoder rows (finite, as meaningless as any padded frame) and the valid ones are scattered in
            // (packed_early: the classifiers read packed rows, the copy is the packed stream as it is)
            if (P.packed_early) {
                launch_copy(P.saved[l], hbuf, (size_t)P.Mp * D * 4, s);  // (a kernel, not a memcpy node: see launch_zero)
            } else {
                launch_copy(P.saved[l], P.packed ? hpad : hbuf, (size_t)M * D * 4, s);
                if (P.packed) launch_pack_rows(P.saved[l], (float*)hbuf, (const int*)P.d_rowoff, (const int*)P.d_frames, N, T, D, true, s);
            }
        }
        gemm(P.fold ? P.as_consumer(P.qkv_params(h, ly), ly.c_qkv) : P.qkv_params(h, ly));
        {
            // (the form is what plan_pass reported: attention_form of the same parameters)
            Timed t_(h, AMX_KC_ATTENTION);
            launch_attention(prec, P.attn_params(), s);
        }
        if (P.fold) {
            residual_gemm(P.as_producer(P.oproj_params(h, ly), false), false);  // (nothing reads the stream between the two halves of a layer)
            ln_finalize();
        } else {
            residual_gemm(P.oproj_params(h, ly), true);
            // pre-LN: the LayerNorm in front of the FFN (`final_layer_norm`); post-LN: `layer_norm` behind the attention residual
            if (P.stable) stream_norm(h->unit_g, h->zero_b, P.Mrows, P.xp_plane, nullptr);
            else stream_norm(ly.ln1_g, ly.ln1_b, P.Mrows, P.xp_plane, ln_inplace);
        }
        gemm(P.fold ? P.as_consumer(P.ffn1_params(h, ly), ly.c_1) : P.ffn1_params(h, ly));
        if (P.fold && (l + 1 < c.layers || P.stream_in_planes)) {
            // fp32 rows where the next reader needs them: hidden state l + 1 is published, or this is the last layer (final LayerNorm,
            // unpacking); the last layer's planes and statistics have no reader (it is a producer for the residual's sake)
            const bool last = l + 1 == c.layers;
            residual_gemm(P.as_producer(P.ffn2_params(h, ly), last || P.saved[l + 1] != nullptr), false);
            if (!last) ln_finalize();
        } else {
            // (the last layer of a packed batch is followed by the unpacking, not by a LayerNorm of these rows)
            // (nor is the FFN2 of an adapter layer: the adapter needs finished rows)
            residual_gemm(P.ffn2_params(h, ly), !P.fold && !h->adapter && !(P.packed && !P.packed_early && l == c.layers - 1));
        }
        if (h->adapter) {
            // attention adapter, in place on the stream; every layer but the last: also the planes of the next layer's first
            // LayerNorm (the last layer is followed by the final LayerNorm of the fp32 rows, after unpacking where rows are packed)
            Timed t_(h, AMX_KC_ROWNORM);
            const bool last = l + 1 == c.layers;
            launch_adapter(prec, (float*)hbuf, P.Mrows, D, h->adapter, ly.ad_w1, ly.ad_b1, ly.ad_w2t, ly.ad_b2, c.eps, last ? nullptr : P.xp,
                           P.xp_plane, s);
        }
        if (!P.stable) stream_norm(ly.ln2_g, ly.ln2_b, P.Mrows, P.xp_plane, ln_inplace);  // `final_layer_norm` closes the post-LN layer
    }
    if (refused) return fail(h, AMX_EINVAL, "internal: an encoder product of the LayerNorm fold had no kernel for its plan and was not launched");
    if (P.packed && !P.packed_early) {
        // back to the padded layout for the final LayerNorm and the projection (padded frames keep their pre-encoder rows)
        { Timed t_(h, AMX_KC_OTHER); launch_pack_rows((const float*)hpad, (float*)P.hpk, (const int*)P.d_rowoff, (const int*)P.d_frames, N, T, D, true, s); }
        hbuf = hpad;
    }
    if (P.stable) {
        stream_norm(h->fln_g, h->fln_b, Mh, pln(h, Mh * D), (float*)P.hfin);
    } else if (P.keep) {
        // post-LN: hidden_states[layers] = the stream as the last layer left it (hfin_rows); its planes are in xp already
        launch_copy(P.hfin, hbuf, (size_t)Mh * D * 4, s);
    }

    // ---- hierarchical projection ----
    for (auto& st : h->steps) {
        const void* A = P.xp;
        int64_t a_plane = pln(h, Mh * D), lda = D;
        if (!st.direct_output) {
            { Timed t_(h, AMX_KC_OTHER); launch_concat(prec, st.parts_dev, (int)st.parts.size(), (const float*)P.logits, h->ld_logits, Mh, P.cat,
                          pln(h, Mh * st.Kpad), st.Kpad, st.Kpad, s); }
            A = P.cat; a_plane = pln(h, Mh * st.Kpad); lda = st.Kpad;
        }
        GemmParams g{};
        g.A = A; g.a_plane = a_plane; g.lda = lda; g.rows_per_batch = Mh;
        g.W = st.W; g.w_plane = pln(h, (int64_t)st.rows * st.Kpad); g.ldw = st.Kpad;
        g.M = (int)Mh; g.N = st.rows; g.K = st.Kpad;
        g.scale = st.r_w; g.bias = st.bias;
        if (st.time_heads > 0) {
            // ProjectingMultiheadAttention.forward (acoustic_model.py:255-268)
            const int Co = st.rows, Cp = st.Cpad;
            g.out_f32 = (float*)P.tl_x; g.ldo = Co;
            gemm(g);
            { Timed t_(h, AMX_KC_OTHER); launch_time_ln_pe(prec, (const float*)P.tl_x, Mh, Co, T, st.tl_g, st.tl_b, 1e-5f, st.tl_pe, P.tl_p,
                              pln(h, Mh * Cp), Cp, s); }
            GemmParams gi{};
            gi.A = P.tl_p; gi.a_plane = pln(h, Mh * Cp); gi.lda = Cp; gi.rows_per_batch = Mh;
            gi.W = st.tl_win; gi.w_plane = pln(h, (int64_t)3 * Co * Cp); gi.ldw = Cp;
            gi.M = (int)Mh; gi.N = 3 * Co; gi.K = Cp;
            gi.scale = st.r_tin; gi.bias = st.tl_bin;
            gi.out_f32 = (float*)P.tl_qkv; gi.ldo = 3 * Co;
            gemm(gi);
            { Timed t_(h, AMX_KC_OTHER); launch_time_attention(prec, (const float*)P.tl_qkv, (const int*)P.d_frames, N, T, Co, st.time_heads,
                                  P.tl_p, pln(h, Mh * Cp), Cp, s); }
            // out_proj lands where the plain linear classifier would have written
            g = GemmParams{};
            g.A = P.tl_p; g.a_plane = pln(h, Mh * Cp); g.lda = Cp; g.rows_per_batch = Mh;
            g.W = st.tl_wout; g.w_plane = pln(h, (int64_t)Co * Cp); g.ldw = Cp;
            g.M = (int)Mh; g.N = Co; g.K = Cp;
            g.scale = st.r_tout; g.bias = st.tl_bout;
        }
        if (st.composed) {
            g.out_p = P.ebuf; g.out_plane = pln(h, Mh * P.Eld); g.ldp = P.Eld;
            gemm(g);
            // logits = (e @ composed) / sqrt(E)   (acoustic_model.py:234)
            const auto& inv = cur_inv(h);
            GemmParams g2{};
            g2.A = P.ebuf; g2.a_plane = pln(h, Mh * P.Eld); g2.lda = P.Eld; g2.rows_per_batch = Mh;
            g2.W = inv.composed_w; g2.w_plane = pln(h, (int64_t)inv.P1 * P.Eld); g2.ldw = P.Eld;
            g2.M = (int)Mh; g2.N = inv.P1; g2.K = P.E;
            g2.scale = inv.r_composed / sqrtf((float)P.E);
            g2.out_f32 = (float*)P.logits + h->col[st.classes[0]]; g2.ldo = h->ld_logits;
            gemm(g2);
        } else {
            g.out_f32 = (float*)P.logits + h->col[st.classes[0]]; g.ldo = h->ld_logits;
            gemm(g);
        }
    }
    { Timed t_(h, AMX_KC_OTHER); launch_logsoftmax_out(cur_inv(h).out_unique_dev, (int)h->out_unique.size(), (const float*)P.logits, h->ld_logits, N, T,
                          (const int*)P.d_frames, (P.flags & AMX_FLAG_RAW_LOGITS) ? 0 : 1, P.d_out, h->nonfinite,
                          P.packed_early ? (const int*)P.d_rowoff : nullptr, s); }
    HIPCHK(h, hipGetLastError());
    return AMX_OK;
}

// what a recording of a pass is keyed on: its buffers, geometry, flags, inventory, the workspace generation and the stream, and
// the lengths where they size grids and tile lists
constexpr size_t KEY_WS_GEN = 8;  // key[KEY_WS_GEN]: the workspace generation (ws_get) the recording's pointers belong to
static std::vector<int64_t> graph_key(amx_handle h, const PassPlan& P, const int64_t* lengths, hipStream_t s) {
    std::vector<int64_t> key;
    key.reserve(10 + (size_t)P.N);
    key.insert(key.end(), {(int64_t)(intptr_t)P.d_audio, (int64_t)(intptr_t)P.d_out, (int64_t)P.N, P.L, (int64_t)P.flags,
                           P.needs_qkv_zero ? (int64_t)P.qkv_zero_bytes : 0, (int64_t)h->inv, (int64_t)cur_inv(h).generation, (int64_t)h->ws_gen});
    // (the stream is part of the key: an executable graph is launched on one stream at a time -- a handle is meant for one
    // stream, include/allophant_amx.h, but a caller that moves to another one gets a recording of its own, not a shared one)
    key.push_back((int64_t)(intptr_t)s);
    // A recording is keyed on GEOMETRY where it can be (ABI 6): in the padded layout without tile skipping every kernel reads
    // lengths / frame counts / masks from the device buffers the plan region has just refreshed (no length travels by value in a
    // kernel node), so batches of one (N, L) with different lengths -- the reference's loop feeds a new batch every iteration,
    // run.py:742-753 -- replay one recording.  Packed rows and skipped conv tiles size grids and tile lists by the lengths:
    // those passes keep them in the key.
    key.push_back(P.packed ? 2 : (P.ragged ? 1 : 0));
    if (P.packed || P.ragged) key.insert(key.end(), lengths, lengths + P.N);
    return key;
}

// The recording cache of amx_forward: replays the graph of a pass whose key was recorded, records one for a key that ran eagerly
// among the last few passes (and launches it), and otherwise notes the key.  `done`: the pass has been launched.
static int run_recorded(amx_handle h, const PassPlan& P, const int64_t* lengths, hipStream_t s, bool& done) {
    std::vector<int64_t> key = graph_key(h, P, lengths, s);
    if (!h->graphs.empty() && h->graphs.front().key[KEY_WS_GEN] != (int64_t)h->ws_gen) {
        // a workspace buffer moved since these were recorded (ws_get synchronised the device before freeing it)
        drop_graphs(h);
    }
    for (auto& g : h->graphs)
        if (g.key == key) {
            HIPCHK(h, hipGraphLaunch(g.exec, s));
            g.last_use = ++h->graph_clock;
            g.last_stream = s;
            ++h->graph_replays;
            h->last_graph = 2;
            done = true;
            return AMX_OK;
        }
    if (std::find(h->graph_seen.begin(), h->graph_seen.end(), key) == h->graph_seen.end()) {
        if ((int)h->graph_seen.size() >= amx_handle_s::GRAPH_SEEN) h->graph_seen.erase(h->graph_seen.begin());
        h->graph_seen.push_back(std::move(key));
        return AMX_OK;
    }
    // this key ran eagerly a moment ago: record it.  Capture runs on a private stream (the caller's may be the null stream, which
    // cannot be captured) in thread-local mode; nothing executes until the launch below.
    if (!h->capture_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->capture_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    if (hipStreamBeginCapture(h->capture_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        h->graph_broken = true;
        return AMX_OK;
    }
    const int erc = enqueue_pass(h, P, h->capture_stream);
    const hipError_t end = hipStreamEndCapture(h->capture_stream, &graph);
    if (erc) {
        if (graph) (void)hipGraphDestroy(graph);
        return erc;
    }
    if (end != hipSuccess || !graph || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        h->graph_broken = true;  // this runtime does not record the pass: stay eager from here on
        return AMX_OK;
    }
    if ((int)h->graphs.size() >= amx_handle_s::GRAPH_CAP) {
        // evict the least recently used recording once nothing on the stream can still be running it
        size_t lru = 0;
        for (size_t i = 1; i < h->graphs.size(); ++i)
            if (h->graphs[i].last_use < h->graphs[lru].last_use) lru = i;
        HIPCHK(h, hipStreamSynchronize(h->graphs[lru].last_stream));  // (its last launch may be on another stream than `s`)
        (void)hipGraphExecDestroy(h->graphs[lru].exec);
        if (h->graphs[lru].graph) (void)hipGraphDestroy(h->graphs[lru].graph);
        h->graphs.erase(h->graphs.begin() + (long)lru);
    }
    HIPCHK(h, hipGraphLaunch(exec, s));
    amx_handle_s::GraphEntry entry;
    entry.key = std::move(key);
    entry.exec = exec;
    entry.graph = graph;
    entry.last_use = ++h->graph_clock;
    entry.last_stream = s;
    h->graphs.push_back(std::move(entry));
    ++h->graph_captures;
    h->last_graph = 1;
    done = true;
    return AMX_OK;
}

extern "C" int amx_forward(amx_handle h, const float* audio, const int64_t* lengths, int N, int64_t L, float* out,
                           int64_t* out_lengths, uint32_t flags, void* stream_) {
    if (!h) return AMX_EINVAL;
    if (!audio || !lengths || !out) return fail(h, AMX_EINVAL, "null buffer");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream_;
    int rc;
    // Safe by default: the reference computes in fp32 and cannot overflow (estimator.py:1035-1046); the fp16 planes can.  A
    // pass that produced non-finite logits on valid frames is reported -- AMX_ERANGE -- by the first amx_forward /
    // amx_synchronize issued after it has completed; nothing of THIS call has been enqueued when that happens.  No host
    // synchronisation: only passes whose trailing event has completed are read.
    if (!(flags & AMX_FLAG_NO_RANGE_CHECK) && (rc = range_poll(h, false))) return rc;
    rc = compute_layout(h, N, L);
    if (rc) return rc;
    PassPlan P;
    if ((rc = plan_pass(h, audio, lengths, N, L, out, out_lengths, flags, s, P))) return rc;

    // ---- run the pass: replay its graph, record one, or enqueue it eagerly ----
    const bool graph_ok = !h->graph_broken && !(flags & (AMX_FLAG_NO_GRAPH | AMX_FLAG_TIMING | AMX_FLAG_KEEP_HIDDEN));
    bool done = false;
    if (graph_ok && (rc = run_recorded(h, P, lengths, s, done))) return rc;
    if (!done && (rc = enqueue_pass(h, P, s))) return rc;
    // the pass's non-finite frame count travels to a pinned slot behind it; the next call reads it (see range_poll)
    if (!(flags & AMX_FLAG_NO_RANGE_CHECK) && (rc = range_record(h, (flags & AMX_FLAG_CONTINUE) != 0, s))) return rc;
    if (flags & AMX_FLAG_HOST_IO) {
        HIPCHK(h, hipMemcpyAsync(out, P.d_out, (size_t)P.total * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
    }
    h->last_N = N; h->last_L = L; h->last_T = P.T; h->last_keep = P.keep;
    h->last_packed_rows = P.packed_early;
    if (P.packed_early) {
        h->last_rowoff = P.rowoff_host;
        h->last_frames = P.frames_host;
    }
    h->qkv_dirty = P.packed;  // a packed call leaves other rows in the Q / K / V planes: the next padded call re-zeroes them
    if (P.dh != P.dhp) h->qkv_pad_dirty = false;  // (if it was set, this pass zeroed the allocations whole: plan_pass)
    // a host-I/O call has synchronised and handed the outputs over already: its own range report does not wait for the next call
    if ((flags & AMX_FLAG_HOST_IO) && !(flags & AMX_FLAG_NO_RANGE_CHECK) && (rc = range_poll(h, true))) return rc;
    return AMX_OK;
}

extern "C" int amx_pass_info(amx_handle h, int32_t* info, int n) {
    if (!h || !info || n < 0) return AMX_EINVAL;
    const int32_t values[AMX_PASS_INFO_COUNT] = {h->last_fold ? 1 : 0, h->last_packed, h->last_graph,
                                                 (int32_t)std::min<int64_t>(h->last_rows, INT32_MAX), (int32_t)(h->pass_counter & 0x7fffffff),
                                                 h->last_attention, h->c0.code()};
    for (int i = 0; i < n && i < AMX_PASS_INFO_COUNT; ++i) info[i] = values[i];
    return AMX_OK;
}

extern "C" int amx_synchronize(amx_handle h, void* stream) {
    if (!h) return AMX_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(h, hipGetLastError());
    return range_poll(h, true);  // every pass issued has completed: AMX_ERANGE if one of them left the range of the planes
}

extern "C" int amx_check_finite(amx_handle h, void* stream, int64_t* frames) {
    if (!h) return AMX_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    int count = 0;
    // read and reset IN STREAM ORDER: callers pass non-blocking streams, which the null stream does not order against, so a
    // reset on the null stream could land after a later forward pass had started counting
    HIPCHK(h, hipMemcpyAsync(&count, h->nonfinite, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemsetAsync(h->nonfinite, 0, 4, s));  // a check closes its reporting period
    HIPCHK(h, hipStreamSynchronize(s));
    if (frames) *frames = count;
    // an explicit check also consumes the pending reports of earlier passes (the stream has drained: their slots are complete)
    const int earlier = range_poll(h, true);
    if (count == 0 && earlier) return earlier;
    if (count > 0)
        return fail(h, AMX_ERANGE, std::to_string(count) + " valid frame(s) of the last forward pass hold non-finite logits: an activation left the "
                                   "range of the 16-bit planes (fp16: |x| <= 65504) or the input was not finite; the bf16 planes "
                                   "(precision bf16x3) have the range of fp32");
    return AMX_OK;
}

extern "C" int amx_graph_info(amx_handle h, int64_t* captures, int64_t* replays) {
    if (!h) return AMX_EINVAL;
    if (captures) *captures = h->graph_captures;
    if (replays) *replays = h->graph_replays;
    return AMX_OK;
}

// the frame counts of a decode call: each in [0, T] of the output block, uploaded as int32
static int upload_frame_lengths(amx_handle h, const int64_t* frame_lengths, int N, int T, hipStream_t s, const int** d_fl) {
    std::vector<int> fl(N);
    for (int n = 0; n < N; ++n) {
        if (frame_lengths[n] < 0 || frame_lengths[n] > T) return fail(h, AMX_EINVAL, "frame length out of range");
        fl[n] = (int)frame_lengths[n];
    }
    void* d;
    if (int rc = ws_get(h, "ctc_frames", (size_t)N * 4, &d)) return rc;
    HIPCHK(h, hipMemcpyAsync(d, fl.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));  // fl is pageable host memory
    *d_fl = (const int*)d;
    return AMX_OK;
}

// ---- the call frame that the CTC entry points share ----
static int check_workspace(amx_handle h, const char* what, size_t need, const void* workspace, size_t bytes) {
    if (bytes < need || (need && !workspace))
        return fail(h, AMX_EINVAL, std::string(what) + " workspace too small: " + std::to_string(need) + " bytes needed");
    return AMX_OK;
}
// the launch of either form of a call: the handle form (h) keeps HIP's own error text
static int ctc_launched(amx_handle h, const char* what) {
    if (!h) return hipGetLastError() == hipSuccess ? AMX_OK : fail(nullptr, AMX_EHIP, std::string(what) + " kernel launch failed");
    HIPCHK(h, hipGetLastError());
    return AMX_OK;
}
// The emission source of an alignment or scoring call, the first half of its CtcRows.  Of a handle: every output block of
// `out` under the layout of (N, L), one row each, blank 0; its frame lengths are on the host, and ctc_rows_begin uploads them once the
// other arguments are checked.  Of a tensor: as the caller describes it, one row per utterance; ctc_rows_begin selects its
// device.
static int rows_of_handle(amx_handle h, const float* out, int N, int64_t L, CtcRows* c) {
    if (int rc = compute_layout(h, N, L)) return rc;
    *c = CtcRows{};
    c->emissions = out, c->descs = cur_inv(h).out_all_dev, c->N = N, c->T = (int)h->layout_T;
    c->rows = (int64_t)h->out_all.size() * N;
    return AMX_OK;
}
static CtcRows rows_of_tensor(const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths, int N, int64_t T,
                              int C, int blank) {
    CtcRows c{};
    c.emissions = emissions, c.stride_n = stride_n, c.stride_t = stride_t, c.frame_lengths = frame_lengths;
    c.rows = N, c.N = N, c.T = (int)T, c.C = C, c.blank = blank;
    return c;
}
static int ctc_rows_begin(amx_handle h, int device, const int64_t* host_lengths, CtcRows* c, hipStream_t s) {
    if (h) return upload_frame_lengths(h, host_lengths, c->N, c->T, s, &c->frame_lengths);
    return hipSetDevice(device) == hipSuccess ? AMX_OK : fail(nullptr, AMX_EHIP, "hipSetDevice failed");
}

extern "C" int amx_greedy_ctc(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L,
                              int64_t* tokens, int64_t* timesteps, int32_t* counts, float* scores, void* stream) {
    if (!h || !out || !frame_lengths || !tokens || !timesteps || !counts || !scores) return AMX_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = compute_layout(h, N, L);  // output block geometry is a function of (N, L, inventory) only
    if (rc) return rc;
    const int T = (int)h->layout_T;
    const int* d_fl;
    if ((rc = upload_frame_lengths(h, frame_lengths, N, T, s, &d_fl))) return rc;
    launch_greedy_ctc(cur_inv(h).out_all_dev, (int)h->out_all.size(), out, d_fl, N, T, tokens, timesteps, counts, scores, s);
    return ctc_launched(h, "greedy CTC");
}

extern "C" int amx_greedy_ctc_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                        const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index,
                                        int64_t* tokens, int64_t* timesteps, int32_t* counts, float* scores, void* stream) {
    if (!emissions || !frame_lengths || !tokens || !timesteps || !counts || !scores) return fail(nullptr, AMX_EINVAL, "null buffer");
    if (N < 1 || T < 1 || C < 1) return fail(nullptr, AMX_EINVAL, "empty emission tensor");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_greedy_ctc_emissions(emissions, stride_n, stride_t, frame_lengths, N, (int)T, C, blank_index, tokens, timesteps, counts,
                                scores, (hipStream_t)stream);
    return ctc_launched(nullptr, "greedy CTC");
}

// =================================================================================================================
// CTC beam search
// =================================================================================================================
namespace {
int beam_check(amx_handle h, int beam_width, int n_best, uint32_t flags) {
    if (beam_width < 1 || beam_width > BEAM_MAX)
        return fail(h, AMX_EINVAL, "beam_width must be 1 to " + std::to_string(BEAM_MAX) + ", got " + std::to_string(beam_width));
    if (n_best < 1 || n_best > beam_width)
        return fail(h, AMX_EINVAL, "n_best must be 1 to beam_width (" + std::to_string(beam_width) + "), got " + std::to_string(n_best));
    if (flags & ~AMX_BEAM_EXP_EMISSIONS) return fail(h, AMX_EINVAL, "unknown beam-search flags");
    return AMX_OK;
}
int beam_check_classes(amx_handle h, int C) {
    if (C < 2 || C > BEAM_MAX_CLASSES)
        return fail(h, AMX_EINVAL, "beam search needs 2 to " + std::to_string(BEAM_MAX_CLASSES) + " classes, got " + std::to_string(C));
    return AMX_OK;
}
}  // namespace

extern "C" int amx_beam_ctc_workspace(int beam_width, int64_t rows, int64_t T, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (int rc = beam_check(nullptr, beam_width, 1, 0)) return rc;
    if (rows < 0 || T < 0) return fail(nullptr, AMX_EINVAL, "negative beam-search geometry");
    *bytes = (size_t)rows * (size_t)T * (size_t)beam_width * sizeof(uint32_t);
    return AMX_OK;
}

namespace {
// The checks that the two decoders of an emission tensor make alike, in three steps between which each entry point makes
// its own: the blank; the geometry (after it, N == 0 means there is nothing to decode); and, once the buffers are known to
// be there, the workspace and the device.
int beam_check_blank(int C, int blank_index) {
    return blank_index < 0 || blank_index >= C ? fail(nullptr, AMX_EINVAL, "blank_index out of range") : AMX_OK;
}
int beam_check_geometry(int N, int64_t T) {
    if (N < 0 || T < 0) return fail(nullptr, AMX_EINVAL, "negative emission geometry");
    return T > INT32_MAX ? fail(nullptr, AMX_EINVAL, "too many frames") : AMX_OK;
}
int beam_tensor_begin(int device, int beam_width, int N, int64_t T, void* workspace, size_t workspace_bytes) {
    size_t need = 0;
    amx_beam_ctc_workspace(beam_width, N, T, &need);
    if (int rc = check_workspace(nullptr, "beam-search", need, workspace, workspace_bytes)) return rc;
    return hipSetDevice(device) == hipSuccess ? AMX_OK : fail(nullptr, AMX_EHIP, "hipSetDevice failed");
}
// the two halves of a BeamArgs: an emission tensor whose geometry has been checked, and the search with its results
void beam_tensor(BeamArgs* a, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths, int N, int64_t T,
                 int C, int blank_index) {
    a->emissions = emissions, a->stride_n = stride_n, a->stride_t = stride_t, a->frame_lengths = frame_lengths;
    a->N = N, a->T = (int)T, a->C = C, a->blank = blank_index;
}
void beam_search(BeamArgs* a, int beam_width, int n_best, uint32_t flags, void* workspace, int64_t* tokens, int64_t* timesteps,
                 int32_t* counts, double* scores, int32_t* hyp_counts) {
    a->beam = beam_width, a->n_best = n_best, a->exp_mode = (flags & AMX_BEAM_EXP_EMISSIONS) ? 1 : 0;
    a->workspace = (uint32_t*)workspace, a->tokens = tokens, a->timesteps = timesteps, a->counts = counts, a->scores = scores;
    a->hyp_counts = hyp_counts;
}
}  // namespace

extern "C" int amx_beam_ctc(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L, int beam_width, int n_best,
                            uint32_t flags, void* workspace, size_t workspace_bytes, int64_t* tokens, int64_t* timesteps,
                            int32_t* counts, double* scores, int32_t* hyp_counts, void* stream) {
    if (!h) return AMX_EINVAL;
    if (!out || !frame_lengths || !tokens || !timesteps || !counts || !scores || !hyp_counts) return fail(h, AMX_EINVAL, "null buffer");
    if (int rc = beam_check(h, beam_width, n_best, flags)) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = compute_layout(h, N, L);
    if (rc) return rc;
    const int T = (int)h->layout_T;
    for (const OutDesc& d : h->out_all)
        if ((rc = beam_check_classes(h, d.C))) return rc;
    BeamArgs a{};
    a.emissions = out, a.descs = cur_inv(h).out_all_dev, a.n_out = (int)h->out_all.size(), a.N = N, a.T = T;
    size_t need = 0;
    amx_beam_ctc_workspace(beam_width, (int64_t)a.n_out * N, T, &need);
    if ((rc = check_workspace(h, "beam-search", need, workspace, workspace_bytes))) return rc;
    if ((rc = upload_frame_lengths(h, frame_lengths, N, T, s, &a.frame_lengths))) return rc;
    beam_search(&a, beam_width, n_best, flags, workspace, tokens, timesteps, counts, scores, hyp_counts);
    launch_beam_ctc(a, s);
    return ctc_launched(h, "beam-search");
}

extern "C" int amx_beam_ctc_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                      const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index, int beam_width,
                                      int n_best, uint32_t flags, void* workspace, size_t workspace_bytes, int64_t* tokens,
                                      int64_t* timesteps, int32_t* counts, double* scores, int32_t* hyp_counts, void* stream) {
    if (int rc = beam_check(nullptr, beam_width, n_best, flags)) return rc;
    if (int rc = beam_check_classes(nullptr, C)) return rc;
    if (int rc = beam_check_blank(C, blank_index)) return rc;
    if (int rc = beam_check_geometry(N, T)) return rc;
    if (N == 0) return AMX_OK;
    if (!emissions || !frame_lengths || !tokens || !timesteps || !counts || !scores || !hyp_counts)
        return fail(nullptr, AMX_EINVAL, "null buffer");
    if (int rc = beam_tensor_begin(device, beam_width, N, T, workspace, workspace_bytes)) return rc;
    BeamArgs a{};
    beam_tensor(&a, emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index);
    beam_search(&a, beam_width, n_best, flags, workspace, tokens, timesteps, counts, scores, hyp_counts);
    launch_beam_ctc_emissions(a, (hipStream_t)stream);
    return ctc_launched(nullptr, "beam-search");
}

extern "C" int amx_beam_ctc_lm_workspace(int beam_width, int64_t rows, int64_t T, size_t* bytes) {
    return amx_beam_ctc_workspace(beam_width, rows, T, bytes);
}

extern "C" int amx_beam_ctc_lm_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                         const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index, int beam_width,
                                         int n_best, uint32_t flags, const float* lm, int n_lm, const int32_t* lm_index,
                                         double lm_weight, double token_score, void* workspace, size_t workspace_bytes,
                                         int64_t* tokens, int64_t* timesteps, int32_t* counts, double* scores, int32_t* hyp_counts,
                                         void* stream) {
    if (int rc = beam_check(nullptr, beam_width, n_best, flags)) return rc;
    if (C < 2 || C > AMX_BEAM_LM_MAX_CLASSES)
        return fail(nullptr, AMX_EINVAL, "beam search with a language model needs 2 to " + std::to_string(AMX_BEAM_LM_MAX_CLASSES) +
                                             " classes, got " + std::to_string(C));
    if (int rc = beam_check_blank(C, blank_index)) return rc;
    if (n_lm < 1) return fail(nullptr, AMX_EINVAL, "n_lm must be at least 1, got " + std::to_string(n_lm));
    if (!std::isfinite(lm_weight) || !std::isfinite(token_score)) return fail(nullptr, AMX_EINVAL, "lm_weight and token_score must be finite");
    if (int rc = beam_check_geometry(N, T)) return rc;
    if (N == 0) return AMX_OK;
    if (!emissions || !frame_lengths || !lm || !lm_index || !tokens || !timesteps || !counts || !scores || !hyp_counts)
        return fail(nullptr, AMX_EINVAL, "null buffer");
    if (int rc = beam_tensor_begin(device, beam_width, N, T, workspace, workspace_bytes)) return rc;
    BeamLmArgs a{};
    beam_tensor(&a, emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index);
    beam_search(&a, beam_width, n_best, flags, workspace, tokens, timesteps, counts, scores, hyp_counts);
    a.lm = lm, a.n_lm = n_lm, a.lm_index = lm_index, a.lm_weight = lm_weight, a.token_score = token_score;
    launch_beam_ctc_lm_emissions(a, (hipStream_t)stream);
    return ctc_launched(nullptr, "beam-search");
}

// =================================================================================================================
// CTC forced alignment
// =================================================================================================================
namespace {
int align_check(amx_handle h, int64_t rows, int64_t T, int64_t max_target, int64_t limit = AMX_ALIGN_MAX_TARGET) {
    if (rows < 0 || T < 0) return fail(h, AMX_EINVAL, "negative alignment geometry");
    if (max_target < 0 || max_target > limit)
        return fail(h, AMX_EINVAL, "max_target must be 0 to " + std::to_string(limit) + ", got " + std::to_string(max_target));
    int64_t cells = 0;
    if (__builtin_mul_overflow(rows, T, &cells) || cells > INT32_MAX) return fail(h, AMX_EINVAL, "rows * T must be below 2^31");
    return AMX_OK;
}
int align_check_classes(amx_handle h, int C, int blank) {
    if (C < 2) return fail(h, AMX_EINVAL, "alignment needs at least 2 classes, got " + std::to_string(C));
    if (blank < 0 || blank >= C) return fail(h, AMX_EINVAL, "blank_index out of range");
    return AMX_OK;
}
// false when the size is not representable in size_t
bool align_workspace_bytes(bool long_form, int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    if (!long_form) return ctc_align_workspace_bytes(rows, T, max_target, bytes);
    AlignLongLayout at;
    if (!ctc_align_long_layout(rows, T, max_target, &at)) return false;
    *bytes = at.bytes;
    return true;
}
// amx_ctc_align / amx_ctc_align_emissions and their long forms from the workspace check on: `c` holds the emission source and
// the row count
int align_rows(amx_handle h, int device, CtcRows c, const int64_t* host_lengths, const int32_t* target_offsets,
               const int32_t* target_ids, int64_t max_target, void* workspace, size_t workspace_bytes, int32_t* paths,
               float* frame_scores, int32_t* spans, float* span_scores, float* totals, int32_t* status, hipStream_t s,
               bool long_form = false) {
    size_t need = 0;
    if (!align_workspace_bytes(long_form, c.rows, c.T, max_target, &need))
        return fail(h, AMX_EINVAL, "alignment workspace size not representable");
    if (int rc = check_workspace(h, "alignment", need, workspace, workspace_bytes)) return rc;
    if (int rc = ctc_rows_begin(h, device, host_lengths, &c, s)) return rc;
    c.target_offsets = target_offsets, c.target_ids = target_ids, c.max_target = (int)max_target;
    AlignLongArgs a{};
    static_cast<CtcRows&>(a) = c;
    a.workspace = (uint4*)workspace;
    a.paths = paths, a.frame_scores = frame_scores, a.spans = spans, a.span_scores = span_scores, a.totals = totals, a.status = status;
    if (long_form)
        launch_ctc_align_long(a, s);
    else
        launch_ctc_align(a, s);
    return ctc_launched(h, "alignment");
}
// the two forms of amx_ctc_align_emissions and of amx_ctc_align
int align_emissions(bool long_form, int device, const float* emissions, int64_t stride_n, int64_t stride_t, const int32_t* frame_lengths,
                    int N, int64_t T, int C, int blank_index, const int32_t* target_offsets, const int32_t* target_ids,
                    int64_t max_target, void* workspace, size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans,
                    float* span_scores, float* totals, int32_t* status, void* stream) {
    if (int rc = align_check(nullptr, N, T, max_target, long_form ? AMX_ALIGN_LONG_MAX_TARGET : AMX_ALIGN_MAX_TARGET)) return rc;
    if (int rc = align_check_classes(nullptr, C, blank_index)) return rc;
    if (N == 0) return AMX_OK;
    if (!frame_lengths || !target_offsets || !totals || !status || (T && (!emissions || !paths || !frame_scores)) ||
        (max_target && (!target_ids || !spans || !span_scores)))
        return fail(nullptr, AMX_EINVAL, "null buffer");
    const CtcRows c = rows_of_tensor(emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index);
    return align_rows(nullptr, device, c, nullptr, target_offsets, target_ids, max_target, workspace, workspace_bytes, paths,
                      frame_scores, spans, span_scores, totals, status, (hipStream_t)stream, long_form);
}
int align_handle(bool long_form, amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L,
                 const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace, size_t workspace_bytes,
                 int32_t* paths, float* frame_scores, int32_t* spans, float* span_scores, float* totals, int32_t* status, void* stream) {
    if (!h) return AMX_EINVAL;
    if (!out || !frame_lengths || !target_offsets || !paths || !frame_scores || !totals || !status ||
        (max_target > 0 && (!target_ids || !spans || !span_scores)))
        return fail(h, AMX_EINVAL, "null buffer");
    HIPCHK(h, hipSetDevice(h->device));
    CtcRows c;
    int rc = rows_of_handle(h, out, N, L, &c);
    if (rc) return rc;
    if ((rc = align_check(h, c.rows, c.T, max_target, long_form ? AMX_ALIGN_LONG_MAX_TARGET : AMX_ALIGN_MAX_TARGET))) return rc;
    if (c.rows == 0) return AMX_OK;
    for (const OutDesc& d : h->out_all)
        if ((rc = align_check_classes(h, d.C, 0))) return rc;
    return align_rows(h, 0, c, frame_lengths, target_offsets, target_ids, max_target, workspace, workspace_bytes, paths, frame_scores,
                      spans, span_scores, totals, status, (hipStream_t)stream, long_form);
}
}  // namespace

extern "C" int amx_ctc_align_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (int rc = align_check(nullptr, rows, T, max_target)) return rc;
    if (!ctc_align_workspace_bytes(rows, T, max_target, bytes)) return fail(nullptr, AMX_EINVAL, "alignment workspace size not representable");
    return AMX_OK;
}

extern "C" int amx_ctc_align_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                       const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index,
                                       const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace,
                                       size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans, float* span_scores,
                                       float* totals, int32_t* status, void* stream) {
    return align_emissions(false, device, emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index, target_offsets, target_ids,
                           max_target, workspace, workspace_bytes, paths, frame_scores, spans, span_scores, totals, status, stream);
}

extern "C" int amx_ctc_align(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L,
                             const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace,
                             size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans, float* span_scores,
                             float* totals, int32_t* status, void* stream) {
    return align_handle(false, h, out, frame_lengths, N, L, target_offsets, target_ids, max_target, workspace, workspace_bytes, paths,
                        frame_scores, spans, span_scores, totals, status, stream);
}

extern "C" int amx_ctc_align_long_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (int rc = align_check(nullptr, rows, T, max_target, AMX_ALIGN_LONG_MAX_TARGET)) return rc;
    if (!align_workspace_bytes(true, rows, T, max_target, bytes)) return fail(nullptr, AMX_EINVAL, "alignment workspace size not representable");
    return AMX_OK;
}

extern "C" int amx_ctc_align_long_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                            const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index,
                                            const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target,
                                            void* workspace, size_t workspace_bytes, int32_t* paths, float* frame_scores,
                                            int32_t* spans, float* span_scores, float* totals, int32_t* status, void* stream) {
    return align_emissions(true, device, emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index, target_offsets, target_ids,
                           max_target, workspace, workspace_bytes, paths, frame_scores, spans, span_scores, totals, status, stream);
}

extern "C" int amx_ctc_align_long(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L,
                                  const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace,
                                  size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans, float* span_scores,
                                  float* totals, int32_t* status, void* stream) {
    return align_handle(true, h, out, frame_lengths, N, L, target_offsets, target_ids, max_target, workspace, workspace_bytes, paths,
                        frame_scores, spans, span_scores, totals, status, stream);
}

// ---- alignment over label graphs (include/allophant_amx_align_graph.h): the same call frame, five graph arrays for the two
// target arrays ----
namespace {
struct AlignGraph {
    const int32_t *node_offsets, *node_classes, *node_flags, *arc_offsets, *arc_preds;
    int64_t max_nodes;
    // what a call dereferences on the device (arc_preds may be empty, but not when a row can hold an arc)
    bool complete() const { return node_offsets && arc_offsets && (max_nodes == 0 || (node_classes && node_flags)) && (max_nodes < 2 || arc_preds); }
};
int align_graph_check(amx_handle h, int64_t rows, int64_t T, int64_t max_nodes) {
    if (max_nodes < 0 || max_nodes > AMX_ALIGN_GRAPH_MAX_NODES)
        return fail(h, AMX_EINVAL, "max_nodes must be 0 to " + std::to_string(AMX_ALIGN_GRAPH_MAX_NODES) + ", got " + std::to_string(max_nodes));
    return align_check(h, rows, T, max_nodes);
}
int align_graph_rows(amx_handle h, int device, CtcRows c, const int64_t* host_lengths, const AlignGraph& g, void* workspace,
                     size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans, float* span_scores, float* totals,
                     int32_t* status, hipStream_t s) {
    size_t need = 0;
    if (!ctc_align_graph_workspace_bytes(c.rows, c.T, g.max_nodes, &need))
        return fail(h, AMX_EINVAL, "graph alignment workspace size not representable");
    if (int rc = check_workspace(h, "graph alignment", need, workspace, workspace_bytes)) return rc;
    if (int rc = ctc_rows_begin(h, device, host_lengths, &c, s)) return rc;
    c.target_offsets = g.node_offsets, c.target_ids = g.node_classes, c.max_target = (int)g.max_nodes;
    AlignGraphArgs a{};
    static_cast<CtcRows&>(a) = c;
    a.node_flags = g.node_flags, a.arc_offsets = g.arc_offsets, a.arc_preds = g.arc_preds;
    a.workspace = (uint4*)workspace;
    a.paths = paths, a.frame_scores = frame_scores, a.spans = spans, a.span_scores = span_scores, a.totals = totals, a.status = status;
    launch_ctc_align_graph(a, s);
    return ctc_launched(h, "graph alignment");
}
}  // namespace

extern "C" int amx_ctc_align_graph_workspace(int64_t rows, int64_t T, int64_t max_nodes, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (int rc = align_graph_check(nullptr, rows, T, max_nodes)) return rc;
    if (!ctc_align_graph_workspace_bytes(rows, T, max_nodes, bytes))
        return fail(nullptr, AMX_EINVAL, "graph alignment workspace size not representable");
    return AMX_OK;
}

extern "C" int amx_ctc_align_graph_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                             const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index,
                                             const int32_t* node_offsets, const int32_t* node_classes, const int32_t* node_flags,
                                             const int32_t* arc_offsets, const int32_t* arc_preds, int64_t max_nodes, void* workspace,
                                             size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans,
                                             float* span_scores, float* totals, int32_t* status, void* stream) {
    if (int rc = align_graph_check(nullptr, N, T, max_nodes)) return rc;
    if (int rc = align_check_classes(nullptr, C, blank_index)) return rc;
    if (N == 0) return AMX_OK;
    const AlignGraph g{node_offsets, node_classes, node_flags, arc_offsets, arc_preds, max_nodes};
    if (!frame_lengths || !g.complete() || !totals || !status || (T && (!emissions || !paths || !frame_scores)) ||
        (max_nodes && (!spans || !span_scores)))
        return fail(nullptr, AMX_EINVAL, "null buffer");
    const CtcRows c = rows_of_tensor(emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index);
    return align_graph_rows(nullptr, device, c, nullptr, g, workspace, workspace_bytes, paths, frame_scores, spans, span_scores, totals,
                            status, (hipStream_t)stream);
}

extern "C" int amx_ctc_align_graph(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L,
                                   const int32_t* node_offsets, const int32_t* node_classes, const int32_t* node_flags,
                                   const int32_t* arc_offsets, const int32_t* arc_preds, int64_t max_nodes, void* workspace,
                                   size_t workspace_bytes, int32_t* paths, float* frame_scores, int32_t* spans, float* span_scores,
                                   float* totals, int32_t* status, void* stream) {
    if (!h) return AMX_EINVAL;
    const AlignGraph g{node_offsets, node_classes, node_flags, arc_offsets, arc_preds, max_nodes};
    if (!out || !frame_lengths || !g.complete() || !paths || !frame_scores || !totals || !status || (max_nodes > 0 && (!spans || !span_scores)))
        return fail(h, AMX_EINVAL, "null buffer");
    HIPCHK(h, hipSetDevice(h->device));
    CtcRows c;
    int rc = rows_of_handle(h, out, N, L, &c);
    if (rc) return rc;
    if ((rc = align_graph_check(h, c.rows, c.T, max_nodes))) return rc;
    if (c.rows == 0) return AMX_OK;
    for (const OutDesc& d : h->out_all)
        if ((rc = align_check_classes(h, d.C, 0))) return rc;
    return align_graph_rows(h, 0, c, frame_lengths, g, workspace, workspace_bytes, paths, frame_scores, spans, span_scores, totals,
                            status, (hipStream_t)stream);
}

// =================================================================================================================
// CTC forward-backward scoring (the alignment's geometry checks, on rows that count the candidates)
// =================================================================================================================
namespace {
int score_rows(amx_handle h, int64_t rows, int candidates, int64_t* out) {
    if (candidates < 1) return fail(h, AMX_EINVAL, "candidates must be at least 1, got " + std::to_string(candidates));
    if (rows < 0) return fail(h, AMX_EINVAL, "negative scoring geometry");
    if (__builtin_mul_overflow(rows, (int64_t)candidates, out)) return fail(h, AMX_EINVAL, "rows * T must be below 2^31");
    return AMX_OK;
}

// amx_ctc_score / amx_ctc_score_emissions from the workspace check on: `c` holds the emission source and the row count
int score_rows_run(amx_handle h, int device, CtcRows c, const int64_t* host_lengths, int candidates, const int32_t* target_offsets,
                   const int32_t* target_ids, int64_t max_target, void* workspace, size_t workspace_bytes, float* log_likelihood,
                   float* occupancy, float* position_sums, float* score_sums, float* posteriors, int32_t* status, hipStream_t s) {
    size_t need = 0;
    if (!ctc_score_workspace_bytes(c.rows, c.T, max_target, &need)) return fail(h, AMX_EINVAL, "scoring workspace size not representable");
    if (int rc = check_workspace(h, "scoring", need, workspace, workspace_bytes)) return rc;
    if (int rc = ctc_rows_begin(h, device, host_lengths, &c, s)) return rc;
    c.target_offsets = target_offsets, c.target_ids = target_ids, c.max_target = (int)max_target;
    ScoreArgs a{};
    static_cast<CtcRows&>(a) = c;
    a.candidates = candidates;
    a.workspace = (float*)workspace;
    a.log_likelihood = log_likelihood, a.occupancy = occupancy, a.position_sums = position_sums, a.score_sums = score_sums;
    a.posteriors = posteriors, a.status = status;
    launch_ctc_score(a, s);
    return ctc_launched(h, "scoring");
}
}  // namespace

extern "C" int amx_ctc_score_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (int rc = align_check(nullptr, rows, T, max_target)) return rc;
    if (!ctc_score_workspace_bytes(rows, T, max_target, bytes)) return fail(nullptr, AMX_EINVAL, "scoring workspace size not representable");
    return AMX_OK;
}

extern "C" int amx_ctc_score_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                       const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index, int candidates,
                                       const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace,
                                       size_t workspace_bytes, float* log_likelihood, float* occupancy, float* position_sums,
                                       float* score_sums, float* posteriors, int32_t* status, void* stream) {
    CtcRows c = rows_of_tensor(emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index);
    if (int rc = score_rows(nullptr, N, candidates, &c.rows)) return rc;
    if (int rc = align_check(nullptr, c.rows, T, max_target)) return rc;
    if (int rc = align_check_classes(nullptr, C, blank_index)) return rc;
    if (N == 0) return AMX_OK;
    if (!frame_lengths || !target_offsets || !log_likelihood || !status || (T && !emissions) ||
        (max_target && (!target_ids || !occupancy || !position_sums || !score_sums)))
        return fail(nullptr, AMX_EINVAL, "null buffer");
    return score_rows_run(nullptr, device, c, nullptr, candidates, target_offsets, target_ids, max_target, workspace, workspace_bytes,
                          log_likelihood, occupancy, position_sums, score_sums, posteriors, status, (hipStream_t)stream);
}

extern "C" int amx_ctc_score(amx_handle h, const float* out, const int64_t* frame_lengths, int N, int64_t L, int candidates,
                             const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace,
                             size_t workspace_bytes, float* log_likelihood, float* occupancy, float* position_sums,
                             float* score_sums, float* posteriors, int32_t* status, void* stream) {
    if (!h) return AMX_EINVAL;
    if (!out || !frame_lengths || !target_offsets || !log_likelihood || !status ||
        (max_target > 0 && (!target_ids || !occupancy || !position_sums || !score_sums)))
        return fail(h, AMX_EINVAL, "null buffer");
    HIPCHK(h, hipSetDevice(h->device));
    CtcRows c;
    int rc = rows_of_handle(h, out, N, L, &c);
    if (rc) return rc;
    if ((rc = score_rows(h, c.rows, candidates, &c.rows))) return rc;
    if ((rc = align_check(h, c.rows, c.T, max_target))) return rc;
    if (c.rows == 0) return AMX_OK;
    for (const OutDesc& d : h->out_all)
        if ((rc = align_check_classes(h, d.C, 0))) return rc;
    return score_rows_run(h, 0, c, frame_lengths, candidates, target_offsets, target_ids, max_target, workspace, workspace_bytes,
                          log_likelihood, occupancy, position_sums, score_sums, posteriors, status, (hipStream_t)stream);
}

// =================================================================================================================
// CTC scoring of every one-edit variant of a transcript (the alignment's geometry checks)
// =================================================================================================================
extern "C" int amx_ctc_variants_workspace(int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (int rc = align_check(nullptr, rows, T, max_target, AMX_VARIANTS_MAX_TARGET)) return rc;
    if (!ctc_variants_workspace_bytes(rows, T, max_target, bytes))
        return fail(nullptr, AMX_EINVAL, "variants workspace size not representable");
    return AMX_OK;
}

extern "C" int amx_ctc_variants_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                          const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index,
                                          const int32_t* target_offsets, const int32_t* target_ids, int64_t max_target, void* workspace,
                                          size_t workspace_bytes, float* log_likelihood, float* substitutions, float* insertions,
                                          int32_t* status, void* stream) {
    if (int rc = align_check(nullptr, N, T, max_target, AMX_VARIANTS_MAX_TARGET)) return rc;
    if (int rc = align_check_classes(nullptr, C, blank_index)) return rc;
    if (C > AMX_VARIANTS_MAX_CLASSES)
        return fail(nullptr, AMX_EINVAL, "variants take at most " + std::to_string(AMX_VARIANTS_MAX_CLASSES) + " classes, got " + std::to_string(C));
    if (N == 0) return AMX_OK;
    if (!frame_lengths || !target_offsets || !log_likelihood || !insertions || !status || (T && !emissions) ||
        (max_target && (!target_ids || !substitutions)))
        return fail(nullptr, AMX_EINVAL, "null buffer");
    size_t need = 0;
    if (!ctc_variants_workspace_bytes(N, T, max_target, &need)) return fail(nullptr, AMX_EINVAL, "variants workspace size not representable");
    if (int rc = check_workspace(nullptr, "variants", need, workspace, workspace_bytes)) return rc;
    CtcRows c = rows_of_tensor(emissions, stride_n, stride_t, frame_lengths, N, T, C, blank_index);
    if (int rc = ctc_rows_begin(nullptr, device, nullptr, &c, (hipStream_t)stream)) return rc;
    c.target_offsets = target_offsets, c.target_ids = target_ids, c.max_target = (int)max_target;
    VariantsArgs a{};
    static_cast<CtcRows&>(a) = c;
    a.forward = (float*)workspace;
    a.log_likelihood = log_likelihood, a.substitutions = substitutions, a.insertions = insertions, a.status = status;
    launch_ctc_variants(a, (hipStream_t)stream);
    return ctc_launched(nullptr, "variants");
}

// =================================================================================================================
// CTC search for label sequences within utterances
// =================================================================================================================
namespace {
int search_check(int64_t N, int64_t Q, int64_t T, int64_t max_query) {
    if (N < 0 || Q < 0 || T < 0) return fail(nullptr, AMX_EINVAL, "negative search geometry");
    if (max_query < 1 || max_query > AMX_SEARCH_MAX_QUERY)
        return fail(nullptr, AMX_EINVAL, "max_query must be 1 to " + std::to_string(AMX_SEARCH_MAX_QUERY) + ", got " + std::to_string(max_query));
    int64_t cells = 0;
    if (__builtin_mul_overflow(N, Q, &cells) || cells > INT32_MAX || __builtin_mul_overflow(cells, T, &cells) || cells > INT32_MAX)
        return fail(nullptr, AMX_EINVAL, "N * Q * T must be below 2^31");
    return AMX_OK;
}
}  // namespace

extern "C" int amx_ctc_search_workspace(int64_t N, int64_t Q, int64_t T, int64_t max_query, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (int rc = search_check(N, Q, T, max_query)) return rc;
    if (!ctc_search_workspace_bytes(N, T, bytes)) return fail(nullptr, AMX_EINVAL, "search workspace size not representable");
    return AMX_OK;
}

extern "C" int amx_ctc_search_emissions(int device, const float* emissions, int64_t stride_n, int64_t stride_t,
                                        const int32_t* frame_lengths, int N, int64_t T, int C, int blank_index,
                                        const int32_t* query_offsets, const int32_t* query_ids, int Q, int64_t max_query,
                                        void* workspace, size_t workspace_bytes, float* best_scores, int32_t* best_spans,
                                        int32_t* status, float* end_scores, int32_t* end_starts, void* stream) {
    if (int rc = search_check(N, Q, T, max_query)) return rc;
    if (int rc = align_check_classes(nullptr, C, blank_index)) return rc;
    if ((end_scores == nullptr) != (end_starts == nullptr))
        return fail(nullptr, AMX_EINVAL, "end_scores and end_starts must both be null or both be given");
    if (N == 0 || Q == 0) return AMX_OK;
    if (!frame_lengths || !query_offsets || !query_ids || !best_scores || !best_spans || !status || (T && !emissions))
        return fail(nullptr, AMX_EINVAL, "null buffer");
    size_t need = 0;
    if (!ctc_search_workspace_bytes(N, T, &need)) return fail(nullptr, AMX_EINVAL, "search workspace size not representable");
    if (int rc = check_workspace(nullptr, "search", need, workspace, workspace_bytes)) return rc;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    SearchArgs a{};
    a.emissions = emissions, a.stride_n = stride_n, a.stride_t = stride_t;
    a.frame_lengths = frame_lengths, a.query_offsets = query_offsets, a.query_ids = query_ids;
    a.N = N, a.T = (int)T, a.C = C, a.blank = blank_index, a.Q = Q, a.max_query = (int)max_query;
    a.frame_max = (float*)workspace;
    a.best_scores = best_scores, a.best_spans = best_spans, a.status = status, a.end_scores = end_scores, a.end_starts = end_starts;
    launch_ctc_search(a, (hipStream_t)stream);
    return ctc_launched(nullptr, "search");
}

// =================================================================================================================
// restriction of a union-inventory output to each utterance's language
// =================================================================================================================
namespace {
// false when the offset of the last element of a [T, N, C] tensor with these strides is not below 2^63
bool restrict_extent(int64_t T, int64_t N, int64_t C, int64_t stride_t, int64_t stride_n) {
    int64_t a = 0, b = 0;
    return !__builtin_mul_overflow(T - 1, stride_t, &a) && !__builtin_mul_overflow(N - 1, stride_n, &b) &&
           !__builtin_add_overflow(a, b, &a) && !__builtin_add_overflow(a, C - 1, &a);
}
}  // namespace

extern "C" int amx_restrict_outputs(int device, const float* src, int64_t stride_t, int64_t stride_n, int C,
                                    const int32_t* frame_lengths, const int32_t* language_ids, const uint64_t* member_bits,
                                    int n_lang, int N, int64_t T, uint32_t flags, float* out, int64_t out_stride_t,
                                    int64_t out_stride_n, int32_t* status, void* stream) {
    if (C < 2 || C > AMX_RESTRICT_MAX_CLASSES)
        return fail(nullptr, AMX_EINVAL, "classes must be 2 to " + std::to_string(AMX_RESTRICT_MAX_CLASSES) + ", got " + std::to_string(C));
    if (n_lang < 1) return fail(nullptr, AMX_EINVAL, "n_lang must be at least 1, got " + std::to_string(n_lang));
    if (flags & ~AMX_RESTRICT_NORMALIZE) return fail(nullptr, AMX_EINVAL, "unknown restriction flags");
    if (N < 0 || T < 0 || stride_t < 0 || stride_n < 0 || out_stride_t < 0 || out_stride_n < 0)
        return fail(nullptr, AMX_EINVAL, "negative restriction geometry");
    if (N == 0 || T == 0) return AMX_OK;
    int64_t rows = 0;
    if (__builtin_mul_overflow((int64_t)N, T, &rows) || rows > (int64_t)UINT32_MAX)
        return fail(nullptr, AMX_EINVAL, "N * T must be below 2^32");
    if (!restrict_extent(T, N, C, stride_t, stride_n) || !restrict_extent(T, N, C, out_stride_t, out_stride_n))
        return fail(nullptr, AMX_EINVAL, "restriction tensor extent must be below 2^63");
    if (!src || !out || !frame_lengths || !language_ids || !member_bits || !status) return fail(nullptr, AMX_EINVAL, "null buffer");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    RestrictArgs a{};
    a.src = src, a.stride_t = stride_t, a.stride_n = stride_n;
    a.out = out, a.out_stride_t = out_stride_t, a.out_stride_n = out_stride_n;
    a.frame_lengths = frame_lengths, a.language_ids = language_ids, a.member_bits = member_bits, a.status = status;
    a.T = T, a.N = N, a.C = C, a.n_lang = n_lang, a.normalize = (flags & AMX_RESTRICT_NORMALIZE) != 0;
    launch_restrict(a, (hipStream_t)stream);
    return ctc_launched(nullptr, "restriction");
}

// =================================================================================================================
// long recordings as windows: the plan, the gather of the windows' audio, the stitch of their kept frames
// =================================================================================================================
extern "C" int amx_long_plan(const int64_t* lengths, int R, int64_t window, int32_t context, const int32_t* conv_kernel,
                             const int32_t* conv_stride, int n_conv, amx_long_window* windows, int64_t capacity,
                             int64_t* n_windows, int64_t* frames) {
    const std::string err = long_plan(lengths, R, window, context, conv_kernel, conv_stride, n_conv, windows, capacity, n_windows, frames);
    return err.empty() ? AMX_OK : fail(nullptr, AMX_EINVAL, err);
}

extern "C" int amx_long_gather(int device, const float* audio, int64_t stride, const int64_t* lengths, int R,
                               const amx_long_window* windows, int n, int64_t hop, int64_t L_out, float* batch,
                               int32_t* status, void* stream) {
    int64_t extent = 0;
    if (n < 0 || R < 0 || L_out < 0 || stride < 0) return fail(nullptr, AMX_EINVAL, "negative gather geometry");
    if (hop < 1 || hop >= ((int64_t)1 << 31)) return fail(nullptr, AMX_EINVAL, "hop must be 1 to 2^31 - 1 samples");
    if (__builtin_mul_overflow((int64_t)R, stride, &extent) || __builtin_mul_overflow((int64_t)n, L_out, &extent))
        return fail(nullptr, AMX_EINVAL, "gather extent must be below 2^63");
    if (n == 0) return AMX_OK;
    if (!audio || !lengths || !windows || !batch || !status) return fail(nullptr, AMX_EINVAL, "null buffer");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_long_gather(audio, stride, lengths, R, windows, n, hop, L_out, batch, status, (hipStream_t)stream);
    return ctc_launched(nullptr, "gather");
}

extern "C" int amx_long_stitch(int device, const float* src, int64_t src_T, int n, const amx_long_window* windows,
                               const amx_long_block* blocks, int n_blocks, float* dst, int R, int64_t dst_T,
                               int32_t* status, void* stream) {
    if (n < 0 || R < 0 || src_T < 0 || dst_T < 0 || n_blocks < 0) return fail(nullptr, AMX_EINVAL, "negative stitch geometry");
    if (n_blocks > AMX_LONG_MAX_BLOCKS)
        return fail(nullptr, AMX_EINVAL, "at most " + std::to_string(AMX_LONG_MAX_BLOCKS) + " blocks per call, got " + std::to_string(n_blocks));
    if (n_blocks > 0 && !blocks) return fail(nullptr, AMX_EINVAL, "null buffer");
    const int64_t LIMIT = (int64_t)1 << 62;
    for (int b = 0; b < n_blocks; ++b) {
        const amx_long_block& k = blocks[b];
        if (k.classes < 1 || k.src_offset < 0 || k.dst_offset < 0) return fail(nullptr, AMX_EINVAL, "a block needs classes >= 1 and offsets >= 0");
        if (src_T >= ((int64_t)1 << 31) || src_T * k.classes >= ((int64_t)1 << 31))
            return fail(nullptr, AMX_EINVAL, "src_T * classes must be below 2^31");
        int64_t a = 0, d = 0;
        if (__builtin_mul_overflow(src_T * k.classes, (int64_t)n, &a) ||
            __builtin_add_overflow(a, k.src_offset, &a) || a >= LIMIT || __builtin_mul_overflow(dst_T, (int64_t)R * k.classes, &d) ||
            __builtin_add_overflow(d, k.dst_offset, &d) || d >= LIMIT)
            return fail(nullptr, AMX_EINVAL, "stitch block extent must be below 2^62 floats");
    }
    if (n == 0 || n_blocks == 0) return AMX_OK;
    if (!src || !windows || !dst || !status) return fail(nullptr, AMX_EINVAL, "null buffer");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_long_stitch(src, src_T, n, windows, blocks, n_blocks, dst, R, dst_T, status, (hipStream_t)stream);
    return ctc_launched(nullptr, "stitch");
}

// =================================================================================================================
// sinc resampling
// =================================================================================================================
extern "C" int amx_resample_bank(int64_t orig_freq, int64_t new_freq, int32_t lowpass_filter_width, double rolloff,
                                 amx_resample_geometry* geometry, float* bank, int32_t* phases) {
    if (!geometry) return fail(nullptr, AMX_EINVAL, "null geometry pointer");
    amx_resample_geometry g{};
    const std::string err = resample_bank(orig_freq, new_freq, lowpass_filter_width, rolloff, &g, bank, phases);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    *geometry = g;
    return AMX_OK;
}

extern "C" int amx_resample(int device, const float* x, int64_t stride, int64_t L_in, const int64_t* lengths,
                            const amx_resample_row* rows, const float* bank, const int32_t* phases, int64_t window, int N,
                            int64_t L_out, float* y, void* stream) {
    if (N < 0 || L_in < 0 || L_out < 0) return fail(nullptr, AMX_EINVAL, "negative resampling geometry");
    if (N > 65535) return fail(nullptr, AMX_EINVAL, "at most 65535 utterances per call");
    if (L_out > ((int64_t)1 << 40)) return fail(nullptr, AMX_EINVAL, "L_out exceeds 2^40 samples");
    if (window < 0 || window > AMX_RESAMPLE_MAX_WINDOW)
        return fail(nullptr, AMX_EINVAL, "window must be 0 to " + std::to_string(AMX_RESAMPLE_MAX_WINDOW));
    if (N > 1 && stride < L_in) return fail(nullptr, AMX_EINVAL, "row stride below L_in");
    if (N == 0 || L_out == 0) return AMX_OK;
    if (!x || !lengths || !rows || !y || (window > 0 && (!bank || !phases))) return fail(nullptr, AMX_EINVAL, "null buffer");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_resample(x, stride, L_in, lengths, rows, bank, phases, (int)window, N, L_out, y, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return fail(nullptr, AMX_EHIP, "resampling kernel launch failed");
    return AMX_OK;
}

// =================================================================================================================
// edit statistics
// =================================================================================================================
static std::string edit_limits(int64_t max_expected, int64_t max_actual) {
    if (max_expected < 0 || max_expected > AMX_EDIT_MAX_LENGTH || max_actual < 0 || max_actual > AMX_EDIT_MAX_LENGTH)
        return "expanded lengths must be 0 to " + std::to_string(AMX_EDIT_MAX_LENGTH);
    return "";
}

extern "C" int amx_edit_workspace(int64_t rows, int64_t max_expected, int64_t max_actual, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (rows < 0 || rows > INT32_MAX) return fail(nullptr, AMX_EINVAL, "rows must be 0 to 2^31 - 1");
    const std::string err = edit_limits(max_expected, max_actual);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    *bytes = edit_workspace_bytes(rows, max_expected, max_actual);
    return AMX_OK;
}

// ---- the call frame that the six row entries share ----
// Their leading arguments after `device`, in the entry points' order; the operations calls have one candidate (stride_k 0, K 1).
struct EditRows {
    const int64_t* tokens;
    int64_t stride_o, stride_n, stride_k;
    int O, N, K;
    int64_t T;
    const int32_t *counts, *hyp_counts, *label_offsets, *label_ids, *groups;
    int G;
    const int32_t *map_offsets, *map_values, *label_maps, *hyp_maps;
    int H;
    int64_t max_expected, max_actual;
    void* workspace;
    size_t workspace_bytes;
};

// Checks them in one order and fills `a`.  `candidates`: K is an argument of the entry, checked and part of its row count.
// `codes`: the workspace is amx_edit_operations_workspace's, one row per (output, utterance); otherwise amx_edit_workspace's,
// one row per candidate.  `outputs`: the entry's own required pointers are all there.  Returns AMX_OK with *pairs == 0 when
// there is nothing to launch.
static int edit_frame(const EditRows& r, bool candidates, bool codes, bool outputs, amx::EditArgs& a, int64_t* pairs) {
    *pairs = 0;
    if (r.O < 0 || r.N < 0 || r.T < 0) return fail(nullptr, AMX_EINVAL, "negative edit geometry");
    if (r.K < 1 || r.K > AMX_EDIT_MAX_CANDIDATES)
        return fail(nullptr, AMX_EINVAL, "K must be 1 to " + std::to_string(AMX_EDIT_MAX_CANDIDATES) + " candidates");
    const std::string err = edit_limits(r.max_expected, r.max_actual);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    if (r.G < 1) return fail(nullptr, AMX_EINVAL, "at least one group");
    if (r.H != 1 && r.H != r.G) return fail(nullptr, AMX_EINVAL, "H must be 1 or G hypothesis-map sets");
    const int64_t rows = (int64_t)r.O * r.N;
    if (rows > INT32_MAX / r.K)
        return fail(nullptr, AMX_EINVAL, candidates ? "O * N * K must stay below 2^31" : "O * N must stay below 2^31");
    size_t needed = 0;
    if (!codes) needed = edit_workspace_bytes(rows * r.K, r.max_expected, r.max_actual);
    else if (!edit_operations_workspace_bytes(rows, r.max_expected, r.max_actual, &needed))
        return fail(nullptr, AMX_EINVAL, "workspace size not representable");
    if (rows == 0) return AMX_OK;
    if (!r.tokens || !r.counts || !r.label_offsets || !r.label_ids || !r.groups || !r.map_offsets || !r.map_values ||
        !r.label_maps || !r.hyp_maps || !r.workspace || !outputs)
        return fail(nullptr, AMX_EINVAL, "null buffer");
    if (r.workspace_bytes < needed)
        return fail(nullptr, AMX_EINVAL, codes ? "workspace smaller than amx_edit_operations_workspace"
                                               : "workspace smaller than amx_edit_workspace");
    a.tokens = r.tokens, a.stride_o = r.stride_o, a.stride_n = r.stride_n, a.stride_k = r.stride_k, a.T = r.T;
    a.O = r.O, a.N = r.N, a.K = r.K, a.G = r.G, a.H = r.H;
    a.counts = r.counts, a.hyp_counts = r.hyp_counts, a.label_offsets = r.label_offsets, a.label_ids = r.label_ids;
    a.groups = r.groups, a.map_offsets = r.map_offsets, a.map_values = r.map_values, a.label_maps = r.label_maps;
    a.hyp_maps = r.hyp_maps, a.cap_a = (int)r.max_expected, a.cap_b = (int)r.max_actual, a.workspace = (int32_t*)r.workspace;
    *pairs = rows;
    return AMX_OK;
}
static int edit_launched(const char* what) {
    return hipGetLastError() == hipSuccess ? AMX_OK : fail(nullptr, AMX_EHIP, std::string(what) + " launch failed");
}

extern "C" int amx_edit_statistics(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k, int O,
                                   int N, int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts,
                                   const int32_t* label_offsets, const int32_t* label_ids, const int32_t* groups, int G,
                                   const int32_t* map_offsets, const int32_t* map_values, const int32_t* label_maps,
                                   const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual, void* workspace,
                                   size_t workspace_bytes, int32_t* statistics, int32_t* best, uint64_t* totals, void* stream) {
    const EditRows r{tokens, stride_o, stride_n, stride_k, O, N, K, T, counts, hyp_counts, label_offsets, label_ids, groups, G,
                     map_offsets, map_values, label_maps, hyp_maps, H, max_expected, max_actual, workspace, workspace_bytes};
    amx::EditArgs a{};
    int64_t pairs = 0;
    const int code = edit_frame(r, true, false, statistics && best && totals, a, &pairs);
    if (code != AMX_OK || pairs == 0) return code;
    a.statistics = statistics, a.best = best, a.totals = totals;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_statistics(a, (hipStream_t)stream);
    return edit_launched("edit statistics");
}

extern "C" int amx_edit_operations_workspace(int64_t rows, int64_t max_expected, int64_t max_actual, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (rows < 0 || rows > INT32_MAX) return fail(nullptr, AMX_EINVAL, "rows must be 0 to 2^31 - 1");
    const std::string err = edit_limits(max_expected, max_actual);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    if (!edit_operations_workspace_bytes(rows, max_expected, max_actual, bytes))
        return fail(nullptr, AMX_EINVAL, "workspace size not representable");
    return AMX_OK;
}

extern "C" int amx_edit_operations(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int O, int N, int64_t T,
                                   const int32_t* counts, const int32_t* hyp_counts, const int32_t* label_offsets,
                                   const int32_t* label_ids, const int32_t* groups, int G, const int32_t* map_offsets,
                                   const int32_t* map_values, const int32_t* label_maps, const int32_t* hyp_maps, int H,
                                   int64_t max_expected, int64_t max_actual, void* workspace, size_t workspace_bytes,
                                   int64_t max_ops, int32_t* operations, int32_t* operation_counts, void* stream) {
    // (lengths beyond the limits are the frame's to report: they give no bound for max_ops)
    if (edit_limits(max_expected, max_actual).empty() && (max_ops < std::max(max_expected, max_actual) || max_ops > INT32_MAX))
        return fail(nullptr, AMX_EINVAL, "max_ops must be max(max_expected, max_actual) to 2^31 - 1");
    const EditRows r{tokens, stride_o, stride_n, 0, O, N, 1, T, counts, hyp_counts, label_offsets, label_ids, groups, G,
                     map_offsets, map_values, label_maps, hyp_maps, H, max_expected, max_actual, workspace, workspace_bytes};
    amx::EditOpsArgs x{};
    int64_t pairs = 0;
    const int code = edit_frame(r, false, true, operations && operation_counts, x.e, &pairs);
    if (code != AMX_OK || pairs == 0) return code;
    x.max_ops = max_ops, x.operations = operations, x.operation_counts = operation_counts;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_operations(x, (hipStream_t)stream);
    return edit_launched("edit operations");
}

// feature-weighted edit distance
static std::string edit_cost_limits(float insertion_cost, float deletion_cost) {
    if (!std::isfinite(insertion_cost) || !std::isfinite(deletion_cost) || insertion_cost <= 0.f || deletion_cost <= 0.f)
        return "insertion and deletion costs must be finite and above 0";
    return "";
}

extern "C" int amx_edit_cost_table_bytes(int64_t V, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    if (V < 1 || V > AMX_EDIT_MAX_SYMBOLS)
        return fail(nullptr, AMX_EINVAL, "a cost table covers 1 to " + std::to_string(AMX_EDIT_MAX_SYMBOLS) + " symbols");
    *bytes = (size_t)V * (size_t)V;
    return AMX_OK;
}

extern "C" int amx_edit_cost_table(int device, const uint8_t* codes, int64_t V, int64_t F, uint8_t* table, void* stream) {
    if (V < 1 || V > AMX_EDIT_MAX_SYMBOLS)
        return fail(nullptr, AMX_EINVAL, "a cost table covers 1 to " + std::to_string(AMX_EDIT_MAX_SYMBOLS) + " symbols");
    if (F < 0 || F > AMX_EDIT_MAX_FEATURES)
        return fail(nullptr, AMX_EINVAL, "feature rows hold 0 to " + std::to_string(AMX_EDIT_MAX_FEATURES) + " columns");
    if (!table || (F > 0 && !codes)) return fail(nullptr, AMX_EINVAL, "null buffer");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_cost_table(codes, (int)V, (int)F, table, (hipStream_t)stream);
    return edit_launched("cost table");
}

extern "C" int amx_edit_weighted_statistics(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k,
                                            int O, int N, int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts,
                                            const int32_t* label_offsets, const int32_t* label_ids, const int32_t* groups, int G,
                                            const int32_t* map_offsets, const int32_t* map_values, const int32_t* label_maps,
                                            const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual,
                                            void* workspace, size_t workspace_bytes, float insertion_cost, float deletion_cost,
                                            const int64_t* cost_tables, const uint8_t* cost_table_data, int32_t* statistics,
                                            int32_t* best, uint64_t* totals, float* costs, void* stream) {
    const std::string err = edit_cost_limits(insertion_cost, deletion_cost);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    const EditRows r{tokens, stride_o, stride_n, stride_k, O, N, K, T, counts, hyp_counts, label_offsets, label_ids, groups, G,
                     map_offsets, map_values, label_maps, hyp_maps, H, max_expected, max_actual, workspace, workspace_bytes};
    amx::EditWeightedArgs w{};
    amx::EditArgs& a = w.x.e;
    int64_t pairs = 0;
    const int code = edit_frame(r, true, false, statistics && best && totals && cost_tables && costs, a, &pairs);
    if (code != AMX_OK || pairs == 0) return code;
    a.statistics = statistics, a.best = best, a.totals = totals;
    w.insertion_cost = insertion_cost, w.deletion_cost = deletion_cost;
    w.tables = cost_tables, w.table_data = cost_table_data, w.costs = costs;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_weighted_statistics(w, (hipStream_t)stream);
    return edit_launched("weighted edit statistics");
}

extern "C" int amx_edit_weighted_operations(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int O, int N,
                                            int64_t T, const int32_t* counts, const int32_t* hyp_counts,
                                            const int32_t* label_offsets, const int32_t* label_ids, const int32_t* groups, int G,
                                            const int32_t* map_offsets, const int32_t* map_values, const int32_t* label_maps,
                                            const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual,
                                            void* workspace, size_t workspace_bytes, float insertion_cost, float deletion_cost,
                                            const int64_t* cost_tables, const uint8_t* cost_table_data, int64_t max_ops,
                                            int32_t* operations, int32_t* operation_counts, float* costs, void* stream) {
    const std::string err = edit_cost_limits(insertion_cost, deletion_cost);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    // (lengths beyond the limits are the frame's to report: they give no bound for max_ops)
    if (edit_limits(max_expected, max_actual).empty() && (max_ops < max_expected + max_actual || max_ops > INT32_MAX))
        return fail(nullptr, AMX_EINVAL, "max_ops must be max_expected + max_actual to 2^31 - 1");
    const EditRows r{tokens, stride_o, stride_n, 0, O, N, 1, T, counts, hyp_counts, label_offsets, label_ids, groups, G,
                     map_offsets, map_values, label_maps, hyp_maps, H, max_expected, max_actual, workspace, workspace_bytes};
    amx::EditWeightedArgs w{};
    int64_t pairs = 0;
    const int code = edit_frame(r, false, true, operations && operation_counts && cost_tables && costs, w.x.e, &pairs);
    if (code != AMX_OK || pairs == 0) return code;
    w.x.max_ops = max_ops, w.x.operations = operations, w.x.operation_counts = operation_counts;
    w.insertion_cost = insertion_cost, w.deletion_cost = deletion_cost;
    w.tables = cost_tables, w.table_data = cost_table_data, w.costs = costs;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_weighted_operations(w, (hipStream_t)stream);
    return edit_launched("weighted edit operations");
}

extern "C" int amx_edit_matrix(int device, const int32_t* expected_offsets, const int32_t* expected_ids,
                               const int32_t* actual_offsets, const int32_t* actual_ids, int64_t rows, int64_t max_expected,
                               int64_t max_actual, float insertion_cost, float deletion_cost, const uint8_t* cost_table, int64_t V,
                               void* workspace, size_t workspace_bytes, float* matrix, int32_t* status, void* stream) {
    if (rows < 0 || rows > INT32_MAX) return fail(nullptr, AMX_EINVAL, "rows must be 0 to 2^31 - 1");
    std::string err = edit_limits(max_expected, max_actual);
    if (err.empty()) err = edit_cost_limits(insertion_cost, deletion_cost);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    if (V < 0 || V > AMX_EDIT_MAX_SYMBOLS)
        return fail(nullptr, AMX_EINVAL, "a cost table covers at most " + std::to_string(AMX_EDIT_MAX_SYMBOLS) + " symbols");
    if (rows == 0) return AMX_OK;
    if (!expected_offsets || !expected_ids || !actual_offsets || !actual_ids || !workspace || !matrix || !status ||
        (V > 0 && !cost_table))
        return fail(nullptr, AMX_EINVAL, "null buffer");
    if (workspace_bytes < edit_workspace_bytes(rows, max_expected, max_actual))
        return fail(nullptr, AMX_EINVAL, "workspace smaller than amx_edit_workspace");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    amx::EditMatrixArgs a{};
    a.expected_offsets = expected_offsets, a.expected_ids = expected_ids;
    a.actual_offsets = actual_offsets, a.actual_ids = actual_ids;
    a.rows = (int)rows, a.cap_a = (int)max_expected, a.cap_b = (int)max_actual, a.V = (int)V, a.table = cost_table;
    a.insertion_cost = insertion_cost, a.deletion_cost = deletion_cost;
    a.workspace = (int2*)workspace, a.matrix = matrix, a.status = status;
    launch_edit_matrix(a, (hipStream_t)stream);
    return edit_launched("edit matrix");
}

// confusion tables
static std::string confusion_capacity_limits(int64_t capacity) {
    if (capacity < AMX_EDIT_CONFUSION_MIN_CAPACITY || capacity > AMX_EDIT_CONFUSION_MAX_CAPACITY || (capacity & (capacity - 1)) != 0)
        return "a confusion table holds a power of two of " + std::to_string(AMX_EDIT_CONFUSION_MIN_CAPACITY) + " to " +
               std::to_string(AMX_EDIT_CONFUSION_MAX_CAPACITY) + " slots";
    return "";
}

extern "C" int amx_edit_confusion_table_bytes(int64_t capacity, size_t* bytes) {
    if (!bytes) return fail(nullptr, AMX_EINVAL, "null size pointer");
    const std::string err = confusion_capacity_limits(capacity);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    *bytes = (size_t)capacity * 2 * sizeof(uint64_t);
    return AMX_OK;
}

extern "C" int amx_edit_confusions(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k, int O,
                                   int N, int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts,
                                   const int32_t* label_offsets, const int32_t* label_ids, const int32_t* groups, int G,
                                   const int32_t* map_offsets, const int32_t* map_values, const int32_t* label_maps,
                                   const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual, void* workspace,
                                   size_t workspace_bytes, const int32_t* best, void* table, int64_t capacity, int32_t* row_events,
                                   uint64_t* counters, void* stream) {
    const std::string err = confusion_capacity_limits(capacity);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    const EditRows r{tokens, stride_o, stride_n, stride_k, O, N, K, T, counts, hyp_counts, label_offsets, label_ids, groups, G,
                     map_offsets, map_values, label_maps, hyp_maps, H, max_expected, max_actual, workspace, workspace_bytes};
    amx::EditConfusionArgs p{};
    int64_t pairs = 0;
    const int code = edit_frame(r, true, true, table && row_events && counters, p.x.e, &pairs);
    if (code != AMX_OK || pairs == 0) return code;
    p.c = {best, (unsigned long long*)table, capacity, row_events, (unsigned long long*)counters};
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_confusions(p, (hipStream_t)stream);
    return edit_launched("edit confusions");
}

extern "C" int amx_edit_weighted_confusions(int device, const int64_t* tokens, int64_t stride_o, int64_t stride_n, int64_t stride_k,
                                            int O, int N, int K, int64_t T, const int32_t* counts, const int32_t* hyp_counts,
                                            const int32_t* label_offsets, const int32_t* label_ids, const int32_t* groups, int G,
                                            const int32_t* map_offsets, const int32_t* map_values, const int32_t* label_maps,
                                            const int32_t* hyp_maps, int H, int64_t max_expected, int64_t max_actual,
                                            void* workspace, size_t workspace_bytes, float insertion_cost, float deletion_cost,
                                            const int64_t* cost_tables, const uint8_t* cost_table_data, const int32_t* best,
                                            void* table, int64_t capacity, int32_t* row_events, uint64_t* counters, void* stream) {
    std::string err = edit_cost_limits(insertion_cost, deletion_cost);
    if (err.empty()) err = confusion_capacity_limits(capacity);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    const EditRows r{tokens, stride_o, stride_n, stride_k, O, N, K, T, counts, hyp_counts, label_offsets, label_ids, groups, G,
                     map_offsets, map_values, label_maps, hyp_maps, H, max_expected, max_actual, workspace, workspace_bytes};
    amx::EditWeightedConfusionArgs p{};
    int64_t pairs = 0;
    const int code = edit_frame(r, true, true, table && row_events && counters && cost_tables, p.w.x.e, &pairs);
    if (code != AMX_OK || pairs == 0) return code;
    p.c = {best, (unsigned long long*)table, capacity, row_events, (unsigned long long*)counters};
    p.w.insertion_cost = insertion_cost, p.w.deletion_cost = deletion_cost;
    p.w.tables = cost_tables, p.w.table_data = cost_table_data, p.w.costs = nullptr;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_weighted_confusions(p, (hipStream_t)stream);
    return edit_launched("weighted edit confusions");
}

extern "C" int amx_edit_confusion_merge(int device, const void* src, int64_t src_capacity, void* dst, int64_t dst_capacity,
                                        uint64_t* counters, void* stream) {
    std::string err = confusion_capacity_limits(src_capacity);
    if (err.empty()) err = confusion_capacity_limits(dst_capacity);
    if (!err.empty()) return fail(nullptr, AMX_EINVAL, err);
    if (!src || !dst || !counters) return fail(nullptr, AMX_EINVAL, "null buffer");
    const char *sb = (const char*)src, *db = (const char*)dst;
    if (sb < db + dst_capacity * 16 && db < sb + src_capacity * 16) return fail(nullptr, AMX_EINVAL, "the tables overlap");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, AMX_EHIP, "hipSetDevice failed");
    launch_edit_confusion_merge((const unsigned long long*)src, src_capacity, (unsigned long long*)dst, dst_capacity,
                                (unsigned long long*)counters, (hipStream_t)stream);
    return edit_launched("confusion merge");
}

// =================================================================================================================
// allophone layer
// =================================================================================================================
extern "C" int amx_set_allophones(amx_handle h, int n_lang, int P1, int Q1, const float* matrices, const uint8_t* mask) {
    if (!h) return AMX_EINVAL;
    if (!h->cfg.allophone_layer) return fail(h, AMX_EINVAL, "Can't map phones to allophones with a model without an allophone layer");
    if (!matrices || !mask) return fail(h, AMX_EINVAL, "null allophone matrices or mask");
    const amx_class_desc* phoneme = nullptr;
    int ci_phoneme = -1;
    for (int ci = 0; ci < (int)h->classes.size(); ++ci)
        if (!strcmp(h->classes[ci].name, "phoneme")) { phoneme = &h->classes[ci]; ci_phoneme = ci; }
    if (!phoneme) return fail(h, AMX_EINVAL, "model has no phoneme classifier");
    if (n_lang < 1) return fail(h, AMX_EINVAL, "the allophone layer needs at least one language");
    if (Q1 != phoneme->size + 1) return fail(h, AMX_EINVAL, "allophone matrices have " + std::to_string(Q1) +
                                              " phoneme columns, the model's phoneme classifier " + std::to_string(phoneme->size + 1));
    // the phone block of a composition model is as wide as its inventory, checked per call by the binding
    if (ci_phoneme != h->composed_class && P1 != phoneme->out_features)
        return fail(h, AMX_EINVAL, "allophone matrices have " + std::to_string(P1) + " phone rows, the model's phone output " +
                                       std::to_string(phoneme->out_features));
    if (P1 < 1 || P1 > AL_MAX_P1) return fail(h, AMX_EINVAL, "allophone matrices need 1 to " + std::to_string(AL_MAX_P1) + " phone rows");
    // compress: column-major walk of every language's matrix, unmasked entries only
    const int64_t cols = (int64_t)n_lang * Q1;
    std::vector<int> col_ptr(cols + 1), ent_p;
    std::vector<float> ent_w, init(cols);
    col_ptr[0] = 0;
    for (int l = 0; l < n_lang; ++l) {
        const int64_t base = (int64_t)l * P1 * Q1;
        for (int q = 0; q < Q1; ++q) {
            bool masked_any = false;
            for (int p = 0; p < P1; ++p) {
                const int64_t i = base + (int64_t)p * Q1 + q;
                if (mask[i]) {
                    masked_any = true;
                } else {
                    ent_p.push_back(p);
                    ent_w.push_back(matrices[i]);
                }
            }
            if (ent_p.size() > (size_t)INT32_MAX) return fail(h, AMX_EINVAL, "allophone matrices too large");
            col_ptr[(int64_t)l * Q1 + q + 1] = (int)ent_p.size();
            init[(int64_t)l * Q1 + q] = masked_any ? -3.40282347e+38f : -INFINITY;
        }
    }
    const size_t n_ent = ent_p.size();
    const size_t b_ptr = (cols + 1) * sizeof(int), b_init = cols * sizeof(float), b_ent = n_ent * sizeof(int);
    const size_t bytes = b_ptr + b_init + 2 * b_ent;
    HIPCHK(h, hipSetDevice(h->device));
    // a map still in flight may read the previous structure
    HIPCHK(h, hipDeviceSynchronize());
    if (h->al_buf) {
        HIPCHK(h, hipFree(h->al_buf));
        h->weight_bytes -= (int64_t)h->al_bytes;
        h->al_buf = nullptr;
        h->al_lang = 0;
    }
    void* buf = nullptr;
    if (hipMalloc(&buf, bytes ? bytes : 16) != hipSuccess) return fail(h, AMX_ENOMEM, "allophone structure allocation failed");
    char* b = (char*)buf;
    h->al_col_ptr = (int*)b;
    h->al_init = (float*)(b + b_ptr);
    h->al_ent_p = (int*)(b + b_ptr + b_init);
    h->al_ent_w = (float*)(b + b_ptr + b_init + b_ent);
    int rc = AMX_OK;
    if (hipMemcpy(h->al_col_ptr, col_ptr.data(), b_ptr, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->al_init, init.data(), b_init, hipMemcpyHostToDevice) != hipSuccess ||
        (n_ent && hipMemcpy(h->al_ent_p, ent_p.data(), b_ent, hipMemcpyHostToDevice) != hipSuccess) ||
        (n_ent && hipMemcpy(h->al_ent_w, ent_w.data(), b_ent, hipMemcpyHostToDevice) != hipSuccess))
        rc = fail(h, AMX_EHIP, "allophone structure upload failed");
    if (rc) {
        (void)hipFree(buf);
        return rc;
    }
    h->al_buf = buf;
    h->al_bytes = bytes;
    h->weight_bytes += (int64_t)bytes;
    h->al_lang = n_lang;
    h->al_P1 = P1;
    h->al_Q1 = Q1;
    return AMX_OK;
}

extern "C" int amx_map_allophones(amx_handle h, const float* phone, int64_t stride_t, int64_t stride_n, const int32_t* language_ids,
                                  int N, int64_t T, float* out, void* stream) {
    if (!h) return AMX_EINVAL;
    if (!h->al_buf) return fail(h, AMX_ESTATE, "amx_map_allophones needs amx_set_allophones first");
    if (N < 0 || T < 0) return fail(h, AMX_EINVAL, "negative batch geometry");
    if (N > 65535) return fail(h, AMX_EINVAL, "at most 65535 utterances per call");
    if (T > ((int64_t)1 << 31)) return fail(h, AMX_EINVAL, "too many frames");
    if (N == 0 || T == 0) return AMX_OK;
    if (!phone || !language_ids || !out) return fail(h, AMX_EINVAL, "null buffer");
    HIPCHK(h, hipSetDevice(h->device));
    launch_allophone_map(phone, stride_t, stride_n, language_ids, h->al_lang, N, T, h->al_P1, h->al_Q1, h->al_col_ptr, h->al_ent_p,
                         h->al_ent_w, h->al_init, out, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return AMX_OK;
}

extern "C" int amx_timing_fetch(amx_handle h, float* ms, int32_t* launches, int n_classes) {
    if (!h || !ms || !launches || n_classes < AMX_KC_COUNT) return AMX_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->timing_stream));
    for (int i = 0; i < n_classes; ++i) { ms[i] = 0.f; launches[i] = 0; }
    for (auto& sp : h->spans) {
        float t = 0.f;
        HIPCHK(h, hipEventElapsedTime(&t, sp.a, sp.b));
        ms[sp.cls] += t;
        launches[sp.cls] += 1;
        h->event_pool.push_back(sp.a);
        h->event_pool.push_back(sp.b);
    }
    h->spans.clear();
    return AMX_OK;
}

extern "C" int amx_debug_fetch(amx_handle h, int what, int index, float* host_out, int64_t capacity, int64_t* ld_out) {
    if (!h || !host_out) return AMX_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    const int64_t M = (int64_t)h->last_N * h->last_T;
    const void* src = nullptr;
    int64_t n = 0;
    if (what == 0) {
        if (!h->last_keep) return fail(h, AMX_ESTATE, "conv output is only kept with AMX_FLAG_KEEP_HIDDEN");
        src = h->ws["conv_dbg"].p; n = M * h->cfg.conv_dim;
    } else if (what == 1) {
        if (index < 0 || index > h->cfg.layers) return fail(h, AMX_EINVAL, "hidden state index out of range");
        std::string nm = index == h->cfg.layers ? "hfin" : "hid" + std::to_string(index);
        if (index == h->cfg.layers && !h->stable && !h->last_keep)
            return fail(h, AMX_ESTATE, "the post-LN encoder keeps its last hidden state for the debug fetch only with AMX_FLAG_KEEP_HIDDEN");
        if (!h->ws.count(nm) || !h->ws[nm].p || (index < h->cfg.layers && !h->last_keep && !h->need_hidden[index]))
            return fail(h, AMX_ESTATE, "hidden state was not kept (AMX_FLAG_KEEP_HIDDEN)");
        src = h->ws[nm].p; n = M * h->cfg.hidden;
    } else if (what == 2) {
        src = h->ws["logits"].p; n = M * h->ld_logits;
        if (ld_out) *ld_out = h->ld_logits;
    } else if (what == 3) {
        // raw workspace bytes (developer diagnostics): index 0 actA, 1 actB, 2 preln
        const char* names[3] = {"actA", "actB", "preln"};
        if (index < 0 || index > 2) return fail(h, AMX_EINVAL, "bad raw buffer index");
        auto& w = h->ws[names[index]];
        src = w.p;
        n = std::min<int64_t>(capacity, (int64_t)(w.bytes / 4));
        if (ld_out) *ld_out = (int64_t)w.bytes;
    } else {
        return fail(h, AMX_EINVAL, "unknown debug item");
    }
    if (!src) return fail(h, AMX_ESTATE, "nothing to fetch before the first amx_forward");
    if (capacity < n) return fail(h, AMX_EINVAL, "debug buffer too small");
    if (h->last_packed_rows && (what == 1 || what == 2)) {
        // the buffer holds the packed rows of a ragged batch (utterance n at last_rowoff[n]): hand them out in the padded
        // [N, T] layout the caller expects, frames beyond an utterance as zeros
        const int64_t ld = n / M;
        int64_t Mp = 0;
        for (int f : h->last_frames) Mp += f;
        std::vector<float> rows((size_t)Mp * ld);
        HIPCHK(h, hipMemcpy(rows.data(), src, rows.size() * 4, hipMemcpyDeviceToHost));
        std::fill(host_out, host_out + n, 0.f);
        for (int u = 0; u < h->last_N; ++u)
            std::memcpy(host_out + (int64_t)u * h->last_T * ld, rows.data() + (int64_t)h->last_rowoff[u] * ld,
                        (size_t)h->last_frames[u] * ld * 4);
        return AMX_OK;
    }
    HIPCHK(h, hipMemcpy(host_out, src, (size_t)n * 4, hipMemcpyDeviceToHost));
    return AMX_OK;
}

// Test hook: every DATA workspace of the handle (ws_get), over its whole allocation -- the geometric slack included -- filled with
// `word16` repeated, by kernels on `stream`.  A pass whose outputs change under it has read something it did not write (DESIGN.md,
// "History independence").  Skipped are the workspaces from which a kernel forms an address, a loop bound or a grid; the plan (or
// the decode call) uploads each of them whole in front of every use, so garbage in them could change nothing but, through a bug
// of the hook's caller, an address:
//   len         int64 sample counts: the loop bounds of the audio statistics and of conv layer 0
//   frames      int32 frame counts: row masks, the key loops of the attention, the walk of the log-softmax
//   rowoff      int32 packed-row offsets, the dispatch order and the encoder's frame counts: row addresses of every packed kernel
//   conv_tiles  int32 tile indices of the conv layers of a ragged batch: the row a workgroup starts at
//   ctc_frames  int32 frame counts of a decode / align / score call: the loop bounds of those kernels
// Everything else in h->ws holds floating-point data (fp16 / bf16 planes, fp32 rows, the fp64 partials of the audio statistics and
// of the GroupNorm) or, audio_host_io / out_host_io, staged samples and outputs.  Not touched: weights, inventories, the
// concatenation recipes (plan_concat's parts_dev: pointers) and the non-finite counter -- all of them dev_alloc, none in h->ws.
// The Q / K / V planes lose their "still zero" premise, so the handle is told: qkv_dirty for the padding rows, qkv_pad_dirty for
// the columns [dh, dhp), which no pass writes (plan_pass).  Recordings stay: no pointer moves, and what a pass zeroes first is
// part of the graph key.
extern "C" int amx_debug_scribble(amx_handle h, uint32_t word16, void* stream) {
    if (!h) return AMX_EINVAL;
    if (word16 > 0xffffu) return fail(h, AMX_EINVAL, "the scribble pattern is one 16-bit word");
    HIPCHK(h, hipSetDevice(h->device));
    static const char* const skipped[] = {"len", "frames", "rowoff", "conv_tiles", "ctc_frames"};
    for (auto& kv : h->ws) {
        if (!kv.second.p || !kv.second.bytes) continue;
        bool skip = false;
        for (const char* name : skipped) skip |= kv.first == name;
        if (!skip) launch_fill16(kv.second.p, kv.second.bytes, word16, (hipStream_t)stream);
    }
    HIPCHK(h, hipGetLastError());
    h->qkv_dirty = h->qkv_pad_dirty = true;
    return AMX_OK;
}
