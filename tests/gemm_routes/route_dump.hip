// Prints the routing table of launch_gemm: one line per (block, product, precision, workspace) case, the public queries of
// amx_common.h first, then the route in detail.  tests/test_gemm_routes.py compares the output byte for byte with routes.txt.
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Iallophant_amd/csrc -Iinclude -o route_dump tests/gemm_routes/route_dump.hip
// Pure host logic: nothing is launched and no GPU is needed (device_cus() falls back to 256, the MI355X's count; the last line
// names the count used).  So that the recording stays a small file, a block is printed as a digest of its lines; in clear text come
// the flagship's own products (xlsr, f16x3, with workspace) and, at the end, the first case that reached each distinct route.
// `route_dump full` prints every line instead; `route_dump rows ...` the products of one layer at a given row count (rows_mode).
// Everything except describe() uses the public queries only and compiles unchanged against an older csrc (-I pointing there, with
// -DROUTE_DUMP_PUBLIC_ONLY where that csrc has no gemm_route: compare the columns up to the second bar of `route_dump full`).
#include "amx_gemm.hip"
#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>
using namespace amx;

struct Detail { const char* kernel; int mi, ni, fold, shape, bn, launches; };

#ifdef ROUTE_DUMP_PUBLIC_ONLY  // against a csrc from before gemm_route: the public columns are what can be compared
static Detail describe(int, const GemmParams&) { return {"-", 0, 0, 0, 0, 0, 0}; }
#else
static Detail describe(int prec, const GemmParams& g) {
    const GemmRoute r = gemm_route(prec_planes(prec), with_vec_flag(g));
    static const char* const names[] = {"LN", "LN_IL", "PP", "DMA", "TILE"};
    return {names[(int)r.kernel], r.mi, r.ni, r.fold, r.shape, r.bn, r.launches ? 1 : 0};
}
#endif

// ---------------------------------------------------------------------------------------------------------------
// output: blocks of lines
// ---------------------------------------------------------------------------------------------------------------
static bool g_full = false;
static std::string g_block;
static std::vector<std::string> g_lines;
static bool g_block_clear = false;  // this block prints the flagship's rows in clear text ...
static bool g_ctx_clear = false;    // ... and this is the flagship's context
static long g_cases = 0;
static std::map<std::string, std::string> g_first;  // distinct route -> the first case that reached it

static void end_block() {
    if (g_block.empty()) return;
    unsigned long long h = 1469598103934665603ull;  // FNV-1a over the lines
    for (auto& l : g_lines)
        for (unsigned char ch : l) h = (h ^ ch) * 1099511628211ull;
    if (!g_full) printf("digest %s %zu %016llx\n", g_block.c_str(), g_lines.size(), h);
    g_cases += (long)g_lines.size();
    g_lines.clear();
    g_block.clear();
}
static void begin_block(const std::string& name, bool clear) {
    end_block();
    g_block = name;
    g_block_clear = clear;
}
static void add_line(const char* line) {
    g_lines.push_back(line);
    if (g_full || (g_block_clear && g_ctx_clear)) fputs(line, stdout);
}

static const char* const PREC_NAME[] = {"bf16", "f16", "bf16x3", "f16x3"};

// one case: block, label, precision, workspace, M x N x K | the public queries | the route
static const char* const HEADER =
    "# block product precision workspace MxNxK | gemm_uses_pp gemm_fuses_ln gemm_ln_tap_minor_slice gemm_planned_splits gemm_ln_fold_ok "
    "fixup_rownorm_eligible | kernel mi ni fold dma_shape tile_bn launches\n";
static void row(int prec, const GemmParams& g, const char* fmt, ...) {
    char label[160], line[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(label, sizeof label, fmt, ap);
    va_end(ap);
    const Detail d = describe(prec, g);
    snprintf(line, sizeof line, "%s %s %s ws%d %dx%dx%d | %d %d %d %d %d %d | %s %d %d %d %d %d %d\n",
             g_block.c_str(), label, PREC_NAME[prec], g.splitk_ws ? 1 : 0, g.M, g.N, g.K, gemm_uses_pp(prec, g) ? 1 : 0,
             gemm_fuses_ln(prec, g) ? 1 : 0, gemm_ln_tap_minor_slice(prec, g), gemm_planned_splits(prec, g), gemm_ln_fold_ok(prec, g) ? 1 : 0,
             fixup_rownorm_eligible(g) ? 1 : 0, d.kernel, d.mi, d.ni, d.fold, d.shape, d.bn, d.launches);
    add_line(line);
    char key[96];
    snprintf(key, sizeof key, "%-5s %d %d %d %d %3d %d chunks%d fold_ok%d", d.kernel, d.mi, d.ni, d.fold, d.shape, d.bn, d.launches,
             gemm_planned_splits(prec, g) > 1 ? 2 : 1, gemm_ln_fold_ok(prec, g) ? 1 : 0);
    g_first.emplace(key, line);
}

// ---------------------------------------------------------------------------------------------------------------
// the products of a pass, built the way amx_api.hip builds them (PassPlan's *_params helpers, enqueue_pass)
// ---------------------------------------------------------------------------------------------------------------
static float g_ws_dummy[4];
static const int64_t SPLITK_ELEMS = ((int64_t)72 << 20) / 4;  // amx_api.hip SPLITK_BYTES / 4: what PassPlan::with_ws passes

template <typename T> static T* fake(uintptr_t a) { return (T*)a; }  // never dereferenced: only its alignment matters
static int round_up(int64_t v, int a) { return (int)((v + a - 1) / a * a); }

struct Ctx {
    int prec;
    bool il;  // interleaved planes (amx_create: two planes and every width a multiple of 32)
    bool ws;
    int NT() const { return prec_planes(prec); }
    int64_t pln(int64_t separate) const { return il ? PLANE_IL : std::max<int64_t>(separate, 64); }
    GemmParams with_ws(GemmParams g) const {
        g.splitk_ws = ws ? g_ws_dummy : nullptr;
        g.splitk_ws_elems = ws ? SPLITK_ELEMS : 0;
        return g;
    }
};

struct Encoder { const char* name; int D, F, H; };
static const Encoder ENCODERS[] = {{"xlsr", 1024, 4096, 16}, {"w2v2-base", 768, 3072, 12}, {"xlsr-1b", 1280, 5120, 16}, {"xlsr-2b", 1920, 7680, 16}};

// batch geometry: N utterances of `seconds` at 16 kHz through the wav2vec2 feature extractor (kernels 10 3 3 3 3 2 2, strides
// 5 2 2 2 2 2 2); Ts[i] = frames after layer i - 1.  Packed: the ragged row count of lengths 50 .. 99 % of the longest.
struct Geo { int N, seconds; };
static const Geo GEOS[] = {{1, 3}, {4, 10}, {32, 10}, {64, 5}, {8, 60}, {1, 60}};
static const int CONV_K[7] = {10, 3, 3, 3, 3, 2, 2}, CONV_S[7] = {5, 2, 2, 2, 2, 2, 2};
static int64_t frames(int64_t samples, int64_t* Ts) {
    int64_t len = samples;
    if (Ts) Ts[0] = len;
    for (int i = 0; i < 7; ++i) {
        len = (len - CONV_K[i]) / CONV_S[i] + 1;
        if (Ts) Ts[i + 1] = len;
    }
    return len;
}
static int64_t packed_rows(const Geo& g) {
    int64_t rows = 0;
    for (int i = 0; i < g.N; ++i) rows += frames((int64_t)g.seconds * 16000 * (i == 0 ? 100 : 50 + (i * 37) % 50) / 100, nullptr);
    return rows;
}

struct Layer {
    const Ctx& c;
    const Encoder& e;
    int64_t Mrows;
    bool packed;
    int T;  // frames of the longest utterance
    GemmParams dense(int64_t a_sep, int N, int K) const {
        GemmParams g{};
        g.A = fake<void>(0x100000); g.a_plane = c.pln(a_sep); g.lda = K; g.rows_per_batch = Mrows;
        g.W = fake<void>(0x200000); g.w_plane = c.pln((int64_t)N * K); g.ldw = K;
        g.M = (int)Mrows; g.N = N; g.K = K;
        g.scale = 1.f; g.bias = fake<float>(0x300000);
        return g;
    }
    GemmParams qkv() const {
        GemmParams g = dense(Mrows * e.D, 3 * e.D, e.D);
        const int dh = e.D / e.H, dhp = dh > 64 ? 128 : 64, Tp = round_up(T, 64), TpTot = round_up(Mrows, 64) + 64;
        g.mode = 1; g.q = fake<void>(0x400000); g.k = fake<void>(0x500000); g.v = fake<void>(0x600000);
        g.qk_plane = packed ? (int64_t)e.H * TpTot * dhp : (Mrows / T) * e.H * Tp * dhp;
        g.T = packed ? (int)std::max<int64_t>(Mrows, 8) : T; g.Tp = packed ? TpTot : Tp; g.H = e.H; g.dh = dh; g.dhp = dhp;
        return c.with_ws(g);
    }
    GemmParams oproj() const {
        GemmParams g = dense(Mrows * e.D, e.D, e.D);
        g.residual = fake<float>(0x700000); g.ldr = e.D; g.out_f32 = fake<float>(0x700000); g.ldo = e.D;
        return c.with_ws(g);
    }
    GemmParams ffn1() const {
        GemmParams g = dense(Mrows * e.D, e.F, e.D);
        g.act = 1; g.out_p = fake<void>(0x800000); g.out_plane = c.pln(Mrows * e.F); g.ldp = e.F;
        return c.with_ws(g);
    }
    GemmParams ffn2() const {
        GemmParams g = dense(Mrows * e.F, e.D, e.F);
        g.residual = fake<float>(0x700000); g.ldr = e.D; g.out_f32 = fake<float>(0x700000); g.ldo = e.D;
        return c.with_ws(g);
    }
    GemmParams as_consumer(GemmParams g) const {
        g.row_coef = fake<float2>(0x900000); g.col_c = fake<float>(0xA00000);
        return g;
    }
    GemmParams as_producer(GemmParams g, bool f32) const {
        g.ln_partial = fake<float2>(0xB00000); g.ln_rowps = fake<float4>(0xC00000);
        g.out_p = fake<void>(0x100000); g.out_plane = c.pln(Mrows * e.D); g.ldp = e.D;
        if (c.NT() > 1) {  // stream_in_planes
            g.ln_res_planes = 1;
            g.residual = nullptr;
            if (!f32) g.out_f32 = nullptr;
        }
        return g;
    }
};

// the products of one layer on Mrows rows (padded: utterances of T frames each)
static void layer_rows_at(const Ctx& c, const Encoder& e, int64_t Mrows, bool packed, int T, const char* where) {
    const Layer L{c, e, Mrows, packed, T};
    row(c.prec, L.qkv(), "%s-qkv", where);
    row(c.prec, L.oproj(), "%s-oproj", where);
    row(c.prec, L.ffn1(), "%s-ffn1", where);
    row(c.prec, L.ffn2(), "%s-ffn2", where);
    row(c.prec, L.as_consumer(L.qkv()), "%s-qkv-consumer", where);
    row(c.prec, L.as_consumer(L.ffn1()), "%s-ffn1-consumer", where);
    row(c.prec, L.as_producer(L.oproj(), false), "%s-oproj-producer", where);
    row(c.prec, L.as_producer(L.ffn2(), false), "%s-ffn2-producer", where);
    row(c.prec, L.as_producer(L.ffn2(), true), "%s-ffn2-producer-f32", where);
    // feature projection (padded: row mask; packed early: the valid frames only)
    GemmParams g = L.dense(L.Mrows * 512, e.D, 512);
    if (!packed) { g.row_len = fake<int>(0xD00000); g.rows_T = T; }
    g.out_f32 = fake<float>(0x700000); g.ldo = e.D;
    row(c.prec, c.with_ws(g), "%s-featproj", where);
}

static void layer_rows(const Ctx& c, const Encoder& e, const Geo& geo, bool packed) {
    const int T = (int)frames((int64_t)geo.seconds * 16000, nullptr);
    char where[64];
    snprintf(where, sizeof where, "%dx%ds%s", geo.N, geo.seconds, packed ? "-packed" : "");
    layer_rows_at(c, e, packed ? packed_rows(geo) : (int64_t)geo.N * T, packed, T, where);
}

// conv layers 1 .. 6: implicit GEMMs over channels-last rows, as the unfused product and with the fused LayerNorm + GELU
static void conv_rows(const Ctx& c, const Geo& geo) {
    const int C = 512;
    int64_t Ts[8];
    frames((int64_t)geo.seconds * 16000, Ts);
    for (int i = 1; i < 7; ++i) {
        const int64_t rows_in = geo.N * Ts[i], rows_out = geo.N * Ts[i + 1];
        GemmParams g{};
        g.A = fake<void>(0x100000); g.a_plane = c.pln(rows_in * C); g.lda = (int64_t)CONV_S[i] * C; g.rows_per_batch = Ts[i + 1];
        g.a_batch_stride = Ts[i] * C;
        g.W = fake<void>(0x200000); g.w_plane = c.pln((int64_t)C * C * CONV_K[i]); g.ldw = (int64_t)C * CONV_K[i];
        g.M = (int)rows_out; g.N = C; g.K = C * CONV_K[i];
        g.scale = 1.f; g.bias = fake<float>(0x300000);
        g = c.with_ws(g);
        GemmParams f = g;
        f.act = 1; f.ln_gamma = fake<float>(0x310000); f.ln_beta = fake<float>(0x320000); f.ln_eps = 1e-5f;
        f.out_p = fake<void>(0x800000); f.out_plane = c.pln(rows_out * C); f.ldp = C;
        g.out_f32 = fake<float>(0x700000); g.ldo = C;
        const char* planes = c.NT() > 1 && !c.il ? "-separate-planes" : "";
        row(c.prec, g, "%dx%ds-conv%d%s", geo.N, geo.seconds, i, planes);
        row(c.prec, f, "%dx%ds-conv%d-ln%s", geo.N, geo.seconds, i, planes);
    }
}

// the hierarchical projection: classifier heads of several widths, K = the hidden width or a concatenation padded to 32, and
// the composed phoneme head (embedding planes, then embeddings x composed inventory)
static void head_rows(const Ctx& c, int64_t Mh) {
    auto head = [&](int N, int K, const char* what) {
        GemmParams g{};
        g.A = fake<void>(0x100000); g.a_plane = c.pln(Mh * K); g.lda = K; g.rows_per_batch = Mh;
        g.W = fake<void>(0x200000); g.w_plane = c.pln((int64_t)N * K); g.ldw = K;
        g.M = (int)Mh; g.N = N; g.K = K;
        g.scale = 1.f; g.bias = fake<float>(0x300000);
        g.out_f32 = fake<float>(0x700000); g.ldo = 1024;
        row(c.prec, c.with_ws(g), "%s", what);
    };
    for (int N : {40, 64, 65, 255, 256, 640}) {
        head(N, 1024, "head");
        head(N, 1056, "head");  // a concatenated input: not a multiple of 64
    }
    const int E = 640, P1 = 230;
    GemmParams g{};
    g.A = fake<void>(0x100000); g.a_plane = c.pln(Mh * 1024); g.lda = 1024; g.rows_per_batch = Mh;
    g.W = fake<void>(0x200000); g.w_plane = c.pln((int64_t)E * 1024); g.ldw = 1024;
    g.M = (int)Mh; g.N = E; g.K = 1024;
    g.scale = 1.f; g.bias = fake<float>(0x300000);
    g.out_p = fake<void>(0x800000); g.out_plane = c.pln(Mh * E); g.ldp = E;
    row(c.prec, c.with_ws(g), "composed-embedding");
    GemmParams g2{};
    g2.A = fake<void>(0x800000); g2.a_plane = c.pln(Mh * E); g2.lda = E; g2.rows_per_batch = Mh;
    g2.W = fake<void>(0x200000); g2.w_plane = c.pln((int64_t)P1 * E); g2.ldw = E;
    g2.M = (int)Mh; g2.N = P1; g2.K = E;
    g2.scale = 0.04f;
    g2.out_f32 = fake<float>(0x700000); g2.ldo = 1024;
    row(c.prec, c.with_ws(g2), "composed-logits");
}

// ---------------------------------------------------------------------------------------------------------------
// the Case list of tools/gemm_bench.hip `check`, with the parameters run_case gives them
// ---------------------------------------------------------------------------------------------------------------
struct Case { const char* name; int M, N, K, act, residual, mask, planes_out, f32_out, qkv, conv_rows_per_batch, conv_lda; };
static const Case BENCH_CASES[] = {
    {"dense-gelu-planes-Mtail", 1500, 512, 256, 1, 0, 0, 1, 0, 0, 0, 0},
    {"dense-f32-res-mask-Ntail", 2100, 640, 384, 0, 1, 1, 0, 1, 0, 0, 0},
    {"dense-f32-planes", 1024, 256, 128, 0, 0, 0, 1, 1, 0, 0, 0},
    {"conv-like", 2800, 512, 384, 0, 0, 0, 0, 1, 0, 700, 256},
    {"qkv", 1497, 384, 256, 0, 0, 0, 0, 0, 1, 0, 0},
    {"qkv-mask", 1497, 384, 256, 0, 0, 1, 0, 0, 1, 0, 0},
    {"long-K", 1100, 256, 4096, 0, 1, 0, 0, 1, 0, 0, 0},
    {"256-rows-f32-res-mask", 16000, 1024, 256, 0, 1, 1, 0, 1, 0, 0, 0},
    {"256-rows-gelu-planes", 15968, 2048, 128, 1, 0, 0, 1, 0, 0, 0, 0},
    {"256-rows-qkv", 15968, 3072, 256, 0, 0, 0, 0, 0, 1, 0, 0},
    {"256-rows-conv-like", 31996, 512, 1536, 0, 0, 0, 0, 1, 0, 7999, 1024},
    {"split-pp-gelu-planes", 2000, 1024, 1024, 1, 0, 0, 1, 0, 0, 0, 0},
    {"split-pp-qkv", 1996, 3072, 1024, 0, 0, 0, 0, 0, 1, 0, 0},
    {"split-pp-qkv-mask", 1996, 3072, 1024, 0, 0, 1, 0, 0, 1, 0, 0},
    {"split-pp-f32-res-mask-planes", 1300, 512, 2048, 0, 1, 1, 1, 1, 0, 0, 0},
    {"split-generic-N%4", 300, 1022, 1024, 0, 1, 1, 0, 1, 0, 0, 0},
    {"split-generic-gelu-planes", 149, 4096, 1024, 1, 0, 0, 1, 0, 0, 0, 0},
    {"split-generic-conv-like", 598, 512, 1536, 0, 0, 0, 0, 1, 0, 299, 1024},
    {"split-generic-qkv", 499, 3072, 1024, 0, 0, 0, 0, 0, 1, 0, 0},
    {"192-wide-qkv-8x10s", 3992, 3072, 1024, 0, 0, 0, 0, 0, 1, 0, 0},
    {"192-wide-qkv-16x10s", 7984, 3072, 512, 0, 0, 0, 0, 0, 1, 0, 0},
    {"Ntail-gelu-planes", 4000, 1088, 256, 1, 0, 0, 1, 0, 0, 0, 0},
    {"N-4-mod-192", 2048, 580, 128, 0, 0, 0, 1, 1, 0, 0, 0},
};

static void bench_rows(const Ctx& c) {
    for (const Case& k : BENCH_CASES) {
        const int64_t rpb = k.conv_rows_per_batch ? k.conv_rows_per_batch : k.M, lda = k.conv_lda ? k.conv_lda : k.K;
        const int64_t stride = k.conv_rows_per_batch ? (rpb - 1) * lda + k.K + 32 * 3 : 0;
        const int64_t a_el = k.conv_rows_per_batch ? (k.M + rpb - 1) / rpb * stride : (int64_t)k.M * k.K;
        const int64_t o_el = (int64_t)k.M * k.N;
        const int T = 499, H = k.N / 3 / 64;
        const int64_t qk_el = (int64_t)((k.M + T - 1) / T) * H * 512 * 64;
        auto plane = [&](int64_t separate) { return c.NT() > 1 ? PLANE_IL : separate; };
        GemmParams g{};
        g.A = fake<void>(0x100000); g.a_plane = plane(a_el); g.lda = lda; g.rows_per_batch = rpb; g.a_batch_stride = stride;
        g.W = fake<void>(0x200000); g.w_plane = plane((int64_t)k.N * k.K); g.ldw = k.K; g.M = k.M; g.N = k.N; g.K = k.K;
        g.scale = 1.f; g.bias = fake<float>(0x300000); g.act = k.act;
        if (k.residual) { g.residual = fake<float>(0x700000); g.ldr = k.N; }
        if (k.mask) { g.row_len = fake<int>(0xD00000); g.rows_T = T; }
        if (k.f32_out) { g.out_f32 = fake<float>(0xE00000); g.ldo = k.N; }
        if (k.planes_out) { g.out_p = fake<void>(0x800000); g.out_plane = plane(o_el); g.ldp = k.N; }
        if (k.qkv) {
            g.mode = 1; g.q = fake<void>(0x400000); g.k = fake<void>(0x500000); g.v = fake<void>(0x600000);
            g.qk_plane = qk_el; g.T = T; g.Tp = 512; g.H = H; g.dh = 64; g.dhp = 64;
        }
        row(c.prec, c.with_ws(g), "%s", k.name);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// thresholds and refusals
// ---------------------------------------------------------------------------------------------------------------
static GemmParams plain(const Ctx& c, int M, int N, int K) {
    GemmParams g{};
    g.A = fake<void>(0x100000); g.a_plane = c.pln((int64_t)M * K); g.lda = K; g.rows_per_batch = M;
    g.W = fake<void>(0x200000); g.w_plane = c.pln((int64_t)N * K); g.ldw = K;
    g.M = M; g.N = N; g.K = K;
    g.scale = 1.f; g.bias = fake<float>(0x300000);
    g.residual = fake<float>(0x700000); g.ldr = N; g.out_f32 = fake<float>(0x700000); g.ldo = N;
    return c.with_ws(g);
}

static void threshold_rows(const Ctx& c) {
    for (int M : {383, 384, 767, 768, 1023, 1024, 4095, 4096})
        for (int K : {2048, 4096})
            for (int N : {64, 65, 255, 256, 1024}) row(c.prec, plain(c, M, N, K), "residual");
    // M x N beyond the split-K workspace
    row(c.prec, plain(c, 7984, 3072, 1024), "beyond-workspace");
    row(c.prec, plain(c, 31936, 4096, 1024), "beyond-workspace");
    row(c.prec, plain(c, 4608, 4096, 4096), "at-workspace");
    row(c.prec, plain(c, 4609, 4096, 4096), "beyond-workspace");
}

// one condition of pp_eligible / dma_tile_eligible / ln_eligible broken at a time, on products that otherwise take that kernel
static void refusal_rows(const Ctx& c) {
    const int NT = c.NT();
    struct Base { const char* name; int M, N, K; };
    for (const Base& b : {Base{"pp", 7984, 1024, 1024}, Base{"dma", 499, 1024, 1024}, Base{"dma-narrow", 499, 64, 1024}}) {
        auto v = [&](const char* what, auto&& change) {
            GemmParams g = plain(c, b.M, b.N, b.K);
            change(g);
            row(c.prec, g, "%s-%s", b.name, what);
        };
        v("as-is", [](GemmParams&) {});
        v("A+4", [](GemmParams& g) { g.A = fake<void>(0x100004); });
        v("W+8", [](GemmParams& g) { g.W = fake<void>(0x200008); });
        v("lda%8", [](GemmParams& g) { g.lda += 4; });
        v("lda%32", [](GemmParams& g) { g.lda += 8; });
        v("ldw%32", [](GemmParams& g) { g.ldw += 8; });
        v("a_plane%8", [](GemmParams& g) { g.a_plane += 4; });
        v("w-separate-planes", [&](GemmParams& g) { g.w_plane = (int64_t)b.N * b.K; });
        v("K%64", [](GemmParams& g) { g.K -= 32; });
        v("K%128", [](GemmParams& g) { g.K -= 64; });
        v("N%4", [](GemmParams& g) { g.N -= 2; });
        v("bias+4", [](GemmParams& g) { g.bias = fake<float>(0x300004); });
        v("out_f32+8", [](GemmParams& g) { g.out_f32 = fake<float>(0x700008); });
        v("ldo%4", [](GemmParams& g) { g.ldo += 2; });
        v("ldr%4", [](GemmParams& g) { g.ldr += 2; });
        v("residual+4", [](GemmParams& g) { g.residual = fake<float>(0x700004); });
        v("out_p+4", [&](GemmParams& g) { g.out_p = fake<void>(0x800004); g.out_plane = c.pln((int64_t)b.M * b.N); g.ldp = b.N; });
        v("ldp%4", [&](GemmParams& g) { g.out_p = fake<void>(0x800000); g.out_plane = c.pln((int64_t)b.M * b.N); g.ldp = b.N + 2; });
        v("short-batches", [](GemmParams& g) { g.rows_per_batch = 200; g.a_batch_stride = 200 * g.lda; });
        v("descending-batches", [](GemmParams& g) { g.rows_per_batch = 256; g.a_batch_stride = 128 * g.lda; });
        v("span-beyond-32-bit", [](GemmParams& g) { g.lda = (int64_t)1 << 23; });
        v("mask-without-rows_T", [](GemmParams& g) { g.row_len = fake<int>(0xD00000); g.rows_T = 0; });
        v("zout", [](GemmParams& g) { g.zout = 64; });
        v("no-bias", [](GemmParams& g) { g.bias = nullptr; });
        v("consumer", [](GemmParams& g) { g.row_coef = fake<float2>(0x900000); g.col_c = fake<float>(0xA00000); g.residual = nullptr; });
        v("consumer-col_c+4", [](GemmParams& g) { g.row_coef = fake<float2>(0x900000); g.col_c = fake<float>(0xA00004); g.residual = nullptr; });
        v("producer-no-planes", [](GemmParams& g) { g.ln_partial = fake<float2>(0xB00000); g.ln_rowps = fake<float4>(0xC00000); });
    }
    // QKV scatter
    for (int dh : {64, 62, 80}) {
        GemmParams g = plain(c, 7984, 3 * 16 * dh, 1024);
        g.residual = nullptr; g.out_f32 = nullptr;
        g.mode = 1; g.q = fake<void>(0x400000); g.k = fake<void>(0x500000); g.v = fake<void>(0x600000 + (dh == 80 ? 4 : 0));
        g.qk_plane = (int64_t)16 * 16 * 512 * 128; g.T = 499; g.Tp = 512; g.H = 16; g.dh = dh; g.dhp = dh > 64 ? 128 : 64;
        row(c.prec, g, "qkv-dh%d%s", dh, dh == 80 ? "-v+4" : "");
    }
    // fused LayerNorm: the conv2 product of 32 x 10 s and what ln_eligible refuses
    auto ln = [&](const char* what, auto&& change) {
        const int C = 512;
        GemmParams f{};
        f.A = fake<void>(0x100000); f.a_plane = c.pln((int64_t)32 * 15999 * C); f.lda = 2 * C; f.rows_per_batch = 7999; f.a_batch_stride = 15999 * C;
        f.W = fake<void>(0x200000); f.w_plane = c.pln((int64_t)C * C * 3); f.ldw = 3 * C;
        f.M = 32 * 7999; f.N = C; f.K = 3 * C;
        f.scale = 1.f; f.bias = fake<float>(0x300000);
        f.act = 1; f.ln_gamma = fake<float>(0x310000); f.ln_beta = fake<float>(0x320000); f.ln_eps = 1e-5f;
        f.out_p = fake<void>(0x800000); f.out_plane = c.pln((int64_t)f.M * C); f.ldp = C;
        f = c.with_ws(f);
        change(f);
        row(c.prec, f, "ln-%s", what);
    };
    ln("as-is", [](GemmParams&) {});
    ln("no-beta", [](GemmParams& f) { f.ln_beta = nullptr; });
    ln("no-gelu", [](GemmParams& f) { f.act = 0; });
    ln("f32-out", [](GemmParams& f) { f.out_f32 = fake<float>(0x700000); f.ldo = 512; });
    ln("N256", [](GemmParams& f) { f.N = 256; });
    ln("M1023", [](GemmParams& f) { f.M = 1023; f.rows_per_batch = 1023; });
    ln("M1024", [](GemmParams& f) { f.M = 1024; f.rows_per_batch = 1024; });
    ln("gamma+4", [](GemmParams& f) { f.ln_gamma = fake<float>(0x310004); });
    ln("out_p+8", [](GemmParams& f) { f.out_p = fake<void>(0x800008); });
    ln("short-batches", [](GemmParams& f) { f.rows_per_batch = 249; f.a_batch_stride = 499 * 512; });
    ln("K%64", [&](GemmParams& f) { f.K -= 32 * (3 - NT); });
    ln("out-separate-planes", [](GemmParams& f) { f.out_plane = (int64_t)f.M * 512; });
}

// the grid.z products of the positional convolution (launch_gemm_grouped): LDS-DMA tiles where dma_tile_shape takes the whole
// grid, else the 128 x 64 register-staged tile
static void grouped_rows(const Ctx& c) {
    for (const Encoder& e : ENCODERS)
        for (const Geo& geo : GEOS) {
            const int groups = 16, taps = 128, cg = e.D / groups, T = (int)frames((int64_t)geo.seconds * 16000, nullptr);
            const int Tpad = round_up(T + taps - 1, 8);
            GemmParams g{};
            g.A = fake<void>(0x100000); g.a_plane = (int64_t)geo.N * Tpad * e.D; g.lda = cg; g.rows_per_batch = T; g.a_batch_stride = (int64_t)Tpad * cg;
            g.za = (int64_t)geo.N * Tpad * cg;
            g.W = fake<void>(0x200000); g.w_plane = (int64_t)e.D * cg * taps; g.ldw = (int64_t)cg * taps;
            g.zw = (int64_t)cg * cg * taps;
            g.M = geo.N * T; g.N = cg; g.K = cg * taps;
            g.scale = 1.f; g.bias = fake<float>(0x300000); g.zbias = cg; g.act = 1;
            g.residual = fake<float>(0x700000); g.ldr = e.D; g.out_f32 = fake<float>(0x700000); g.ldo = e.D; g.zout = cg;
            const int shape = dma_tile_shape(c.NT(), with_vec_flag(g), groups);
            char line[200];
            snprintf(line, sizeof line, "%s %s %dx%ds %s %dx%dx%d x%d | %s %d\n", g_block.c_str(), e.name, geo.N, geo.seconds, PREC_NAME[c.prec],
                     g.M, g.N, g.K, groups, shape ? "DMA" : "TILE", shape);
            add_line(line);
        }
}

// `route_dump rows <encoder> <precision> <packed 0|1> <M> [T]`: the products of one layer at an arbitrary row count (with the
// split-K workspace, as a pass has it; padded rows: utterances of T frames), in the clear-text row format
static int rows_mode(int argc, char** argv) {
    if (argc < 6) {
        fputs("usage: route_dump rows <encoder> <precision> <packed 0|1> <M> [T]\n", stderr);
        return 2;
    }
    const Encoder* e = nullptr;
    for (const Encoder& k : ENCODERS)
        if (k.name == std::string(argv[2])) e = &k;
    int prec = -1;
    for (int i = 0; i < 4; ++i)
        if (PREC_NAME[i] == std::string(argv[3])) prec = i;
    const bool packed = atoi(argv[4]) != 0;
    const int64_t M = atoll(argv[5]);
    const int T = argc > 6 ? atoi(argv[6]) : (int)M;
    if (!e || prec < 0 || M < 1 || T < 1 || (!packed && M % T)) {
        fputs("route_dump rows: unknown encoder or precision, or M is no multiple of T\n", stderr);
        return 2;
    }
    g_full = true;
    fputs(HEADER, stdout);
    begin_block("rows", true);
    char where[64];
    snprintf(where, sizeof where, "%lldx%d%s", (long long)(packed ? 1 : M / T), packed ? (int)M : T, packed ? "-packed" : "");
    layer_rows_at(Ctx{prec, prec_planes(prec) > 1, true}, *e, M, packed, T, where);
    end_block();
    printf("%ld cases, cus %d\n", g_cases, device_cus());
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "rows") return rows_mode(argc, argv);
    g_full = argc > 1 && std::string(argv[1]) == "full";
    const int precs[] = {PREC_BF16, PREC_F16, PREC_BF16X3, PREC_F16X3};
    fputs(HEADER, stdout);
    for (int force = 0; force < 2; ++force) {
        g_force_generic_gemm = force != 0;
        const std::string suffix = force ? "-generic" : "";
        auto each = [&](auto&& fn) {  // every precision, workspace absent and present
            for (int prec : precs)
                for (int ws = 0; ws < 2; ++ws) {
                    g_ctx_clear = !force && prec == PREC_F16X3 && ws;
                    fn(Ctx{prec, prec_planes(prec) > 1, ws != 0});
                }
        };
        for (const Encoder& e : ENCODERS) {
            begin_block(std::string("layer-") + e.name + suffix, &e == &ENCODERS[0]);
            each([&](const Ctx& c) {
                for (const Geo& geo : GEOS)
                    for (int packed = 0; packed < 2; ++packed) layer_rows(c, e, geo, packed != 0);
            });
        }
        begin_block("conv" + suffix, true);
        each([](const Ctx& c) {
            for (const Geo& geo : GEOS) {
                conv_rows(c, geo);
                // two planes that are not interleaved: amx_create turns that off when the hidden or FFN width is not a multiple of 32
                const bool clear = g_ctx_clear;
                g_ctx_clear = false;
                if (c.NT() > 1) conv_rows(Ctx{c.prec, false, c.ws}, geo);
                g_ctx_clear = clear;
            }
        });
        begin_block("head" + suffix, true);
        each([](const Ctx& c) {
            for (const Geo& geo : GEOS) {
                head_rows(c, (int64_t)geo.N * frames((int64_t)geo.seconds * 16000, nullptr));
                if (geo.N == 32) head_rows(c, packed_rows(geo));
            }
        });
        begin_block("bench" + suffix, false);
        each(bench_rows);
        begin_block("threshold" + suffix, false);
        each(threshold_rows);
        begin_block("refusal" + suffix, false);
        each(refusal_rows);
        begin_block("grouped" + suffix, false);
        each([](const Ctx& c) { if (c.ws) grouped_rows(c); });
    }
    end_block();
    g_force_generic_gemm = false;
    if (!g_full)
        for (auto& kv : g_first) printf("first %s", kv.second.c_str());
    printf("%ld cases, cus %d\n", g_cases, device_cus());
    return 0;
}
