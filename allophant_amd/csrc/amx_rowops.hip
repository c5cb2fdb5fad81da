// Row-wise / bandwidth-bound kernels of the Allophant forward path on gfx950 (64-wide wavefronts):
// row LayerNorm(+GELU)(+LayerNorm) with 16-bit plane output, positional-conv input image, classifier-input concatenation (hidden | softmax(dependency logits)),
// per-head log-softmax with [T,N,C] time-major output, greedy CTC decode, and the one-off weight packers.
#include "amx_common.h"
#include <cstdlib>

namespace amx {

namespace {

// ----------------------------------------------------------------------------------------------------------------
// Row kernel: x[M, D] fp32 -> [LayerNorm(g1,b1) -> optional GELU] -> [LayerNorm(g2,b2)] -> planes / fp32.
// One wave per row, D <= 256 V, D % 4 == 0, row kept in registers (float4 x V per lane; V = 4 up to hidden 1024 -- XLS-R 300M and
// every released checkpoint --, V = 8 up to 2048: the XLS-R 1B / 2B widths 1280 / 1920, round 6).
// ----------------------------------------------------------------------------------------------------------------
template <typename T, int NT, int V = 4>
// (x and out_f32 carry no __restrict__: the post-LN encoder normalises the residual stream IN PLACE, out_f32 == x; a wave loads
// its whole row into registers before it stores any of it, and rows belong to one wave each)
__global__ __launch_bounds__(256) void rownorm_kernel(const float* x, int64_t ldx, int64_t M, int D,
                                                      const float* __restrict__ g1, const float* __restrict__ b1, int gelu,
                                                      const float* __restrict__ g2, const float* __restrict__ b2,
                                                      float eps1, float eps2, T* __restrict__ out_p, int64_t out_plane,
                                                      int64_t ldp, float* out_f32, int64_t ldo,
                                                      const int* __restrict__ row_off, const int* __restrict__ frame_len, int T_rows) {
    const int lane = threadIdx.x & 63;
    int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* src = x + row * ldx;
    if (row_off) {
        // ragged batch: input row n * T_rows + t goes to packed row row_off[n] + t; frames beyond the utterance are dropped
        const int n = (int)(row / T_rows), t = (int)(row - (int64_t)n * T_rows);
        if (t >= frame_len[n]) return;
        row = (int64_t)row_off[n] + t;
    }
    float4 v[V];
    const float invD = 1.0f / (float)D;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        int c = (i * 64 + lane) * 4;
        v[i] = c < D ? *(const float4*)(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    auto norm = [&](const float* g, const float* b, float eps, bool act) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) s += v[i].x + v[i].y + v[i].z + v[i].w;  // out-of-range entries are zero
        const float mu = wave_sum(s) * invD;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            int c = (i * 64 + lane) * 4;
            if (c < D) {
                float dx = v[i].x - mu, dy = v[i].y - mu, dz = v[i].z - mu, dw = v[i].w - mu;
                q += dx * dx + dy * dy + dz * dz + dw * dw;
            }
        }
        const float rs = 1.0f / sqrtf(wave_sum(q) * invD + eps);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            int c = (i * 64 + lane) * 4;
            if (c < D) {
                float4 gg = *(const float4*)(g + c), bb = *(const float4*)(b + c);
                float4 y;
                y.x = (v[i].x - mu) * rs * gg.x + bb.x;
                y.y = (v[i].y - mu) * rs * gg.y + bb.y;
                y.z = (v[i].z - mu) * rs * gg.z + bb.z;
                y.w = (v[i].w - mu) * rs * gg.w + bb.w;
                if (act) {
                    const f32x2 g01 = gelu_fast2(f32x2{y.x, y.y}), g23 = gelu_fast2(f32x2{y.z, y.w});
                    y.x = g01[0]; y.y = g01[1]; y.z = g23[0]; y.w = g23[1];
                }
                v[i] = y;
            }
        }
    };
    if (g1) norm(g1, b1, eps1, gelu != 0);
    if (g2) norm(g2, b2, eps2, false);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        int c = (i * 64 + lane) * 4;
        if (c < D) {
            if (out_f32) *(float4*)(out_f32 + row * ldo + c) = v[i];
            if (out_p) store_planes4<T, NT>(out_p, out_plane, row * ldp + c, v[i]);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------
// LayerNorm fold (GemmParams.ln_partial / row_coef, amx_common.h).  The power of two a row's planes are written under: 2 * rstd
// rounded down to a power of two, i.e. sigma * s in (1, 2] -- |x - mu| <= sqrt(D) sigma keeps a row itself below 64, and an element
// of the NEXT state of the row (written under this scale before its own statistics are known) may move 32 768 .. 65 504 of the
// previous sigmas before an fp16 plane overflows (which the range report of the pass then shows): a sublayer's sudden outlier
// channel stays in range.  The lo plane of a two-plane pair turns subnormal below 2^-3 / s, 0.06 .. 0.125 sigma, and keeps its
// bits down to 2^-24 / s (tests/diagnostics/emulate_ln_fold.py: no measurable cost against a scale of 16 * rstd).
// Padded frames of a ragged batch in the padded layout (frame_len, T_rows given) take 2^-6 of that scale: their sigma is 2 .. 7
// times smaller than that of the valid frames, and the same bias jump would overflow them first.  Nothing valid reads them -- the
// attention masks their keys, hidden states publish zeros there -- but a non-finite padded V row times a masked P = 0 is NaN.
// ----------------------------------------------------------------------------------------------------------------
constexpr float LN_PAD_SCALE = 0x1p-6f;
__device__ __forceinline__ float ln_plane_scale(float rstd, bool padded) {
    const float t = fminf(fmaxf(2.0f * rstd, 1.0e-12f), 1.0e12f);
    const float s = __uint_as_float(__float_as_uint(t) & 0x7F800000u);
    return padded ? s * LN_PAD_SCALE : s;
}
__device__ __forceinline__ bool ln_padded_row(int64_t row, const int* frame_len, int T_rows) {
    return frame_len && (int)(row % T_rows) >= frame_len[row / T_rows];
}

// the first norm of the stack: exact statistics from the fp32 row (the arithmetic of rownorm_kernel), planes of (x - mu) * s
template <typename T, int NT, int V = 4>
__global__ __launch_bounds__(256) void ln_rowprep_kernel(const float* __restrict__ x, int64_t ldx, int64_t M, int D, float eps,
                                                         T* __restrict__ out_p, int64_t out_plane, int64_t ldp,
                                                         float4* __restrict__ rowps, float2* __restrict__ coef,
                                                         const int* __restrict__ frame_len, int T_rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* src = x + row * ldx;
    float4 v[V];
    const float invD = 1.0f / (float)D;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = (i * 64 + lane) * 4;
        v[i] = c < D ? *(const float4*)(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) s += v[i].x + v[i].y + v[i].z + v[i].w;
    const float mu = wave_sum(s) * invD;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) {
            const float dx = v[i].x - mu, dy = v[i].y - mu, dz = v[i].z - mu, dw = v[i].w - mu;
            q += dx * dx + dy * dy + dz * dz + dw * dw;
        }
    }
    const float rs = 1.0f / sqrtf(wave_sum(q) * invD + eps);
    const float sc = ln_plane_scale(rs, ln_padded_row(row, frame_len, T_rows));
    if (lane == 0) {
        rowps[row] = make_float4(mu, sc, mu, sc);
        coef[row] = make_float2(rs / sc, 0.f);
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < D) {
            T hi[4], lo[4];
            split16<T, NT>((v[i].x - mu) * sc, hi[0], lo[0]);
            split16<T, NT>((v[i].y - mu) * sc, hi[1], lo[1]);
            split16<T, NT>((v[i].z - mu) * sc, hi[2], lo[2]);
            split16<T, NT>((v[i].w - mu) * sc, hi[3], lo[3]);
            T* dst = out_p + pidx(row * ldp + c, plane_is_il<NT>(out_plane));
            typedef typename Vec4<T>::type V4;
            V4 hv = {hi[0], hi[1], hi[2], hi[3]};
            *(V4*)dst = hv;
            if (NT > 1) {
                V4 lv = {lo[0], lo[1], lo[2], lo[3]};
                *(V4*)(dst + out_plane) = lv;
            }
        }
    }
}

// one thread per row: Chan's pairwise update over the row's 64-column blocks, in ascending order
__global__ __launch_bounds__(256) void ln_finalize_kernel(const float2* __restrict__ partial, int blocks, int64_t M, float eps,
                                                          float4* __restrict__ rowps, float2* __restrict__ coef,
                                                          const int* __restrict__ frame_len, int T_rows) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= M) return;
    const float2* pr = partial + row * blocks;
    float2 b[32];  // (hidden <= 2048)
    float s1 = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j)
        if (j < blocks) {
            b[j] = pr[j];
            s1 += b[j].x;
        }
    // the producer wrote the planes under (pivot z, scale w) and formed the statistics of u = (x - z) * w: w is a power of two, so
    // the sums are those of x - z times w (times w^2) exactly
    const float4 ps = rowps[row];
    const float inv_w = __uint_as_float(0x7F000000u - __float_as_uint(ps.w));
    const float invD = 1.0f / (float)(blocks * 64);
    const float mu = s1 * invD;  // mean of u
    float m2 = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j)
        if (j < blocks) {
            const float d = b[j].x * (1.0f / 64.0f) - mu;
            m2 += fmaf(64.0f * d, d, b[j].y);
        }
    const float m1 = mu * inv_w;  // mean of x - pivot
    const float rs = 1.0f / sqrtf(m2 * invD * inv_w * inv_w + eps);
    coef[row] = make_float2(rs * inv_w, -rs * m1);
    rowps[row] = make_float4(ps.z, ps.w, ps.z + m1, ln_plane_scale(rs, ln_padded_row(row, frame_len, T_rows)));
}

// ----------------------------------------------------------------------------------------------------------------
// positional-conv input image: h[N*T, D] fp32 -> planes [G][N][Tpad][cg], zero rows in front/behind every utterance
// ----------------------------------------------------------------------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(256) void posconv_pack_kernel(const float* __restrict__ h, int N, int Tn, int D, int G,
                                                           int pad_front, int Tpad, T* __restrict__ out, int64_t out_plane,
                                                           const int* __restrict__ row_off, const int* __restrict__ frame_len) {
    const int cg = D / G;
    const int64_t total4 = (int64_t)G * N * Tpad * cg / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        int64_t e = i * 4;
        int ci = (int)(e % cg);
        int64_t r = e / cg;
        int tp = (int)(r % Tpad);
        r /= Tpad;
        int n = (int)(r % N);
        int g = (int)(r / N);
        int t = tp - pad_front;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        // packed rows (row_off): utterance n owns rows row_off[n] .. + frame_len[n]; its other frames are the zeros the
        // feature projection's row mask leaves in the padded layout
        if (row_off) {
            if (t >= 0 && t < frame_len[n]) v = *(const float4*)(h + ((int64_t)row_off[n] + t) * D + g * cg + ci);
        } else if (t >= 0 && t < Tn) v = *(const float4*)(h + ((int64_t)n * Tn + t) * D + g * cg + ci);
        T hi[4], lo[4];
        split16<T, NT>(v.x, hi[0], lo[0]);
        split16<T, NT>(v.y, hi[1], lo[1]);
        split16<T, NT>(v.z, hi[2], lo[2]);
        split16<T, NT>(v.w, hi[3], lo[3]);
        typedef typename Vec4<T>::type V4;
        V4 hv = {hi[0], hi[1], hi[2], hi[3]};
        *(V4*)(out + e) = hv;
        if (NT > 1) {
            V4 lv = {lo[0], lo[1], lo[2], lo[3]};
            *(V4*)(out + out_plane + e) = lv;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------
// classifier input: cat([hidden | softmax(dependency logits)]) as 16-bit planes, one wave per row
// (reference acoustic_model.py:497-514)
// ----------------------------------------------------------------------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(256) void concat_kernel(const ConcatPart* __restrict__ parts, int n_parts,
                                                     const float* __restrict__ logits, int64_t ld_logits, int64_t M,
                                                     T* __restrict__ out, int64_t out_plane, int64_t ldp, int kpad) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const bool il = plane_is_il<NT>(out_plane);
    const int64_t row0 = row * ldp;  // logical offset of the row; element c lives at pidx(row0 + c)
    int kend = 0;
    for (int pi = 0; pi < n_parts; ++pi) {
        const ConcatPart pt = parts[pi];
        if (pt.type == 0) {
            const float* src = pt.src + row * pt.width;
            for (int c = lane; c < pt.width; c += 64) {
                T hi, lo;
                split16<T, NT>(src[c], hi, lo);
                T* dst = out + pidx(row0 + pt.dst_col + c, il);
                dst[0] = hi;
                if (NT > 1) dst[out_plane] = lo;
            }
        } else {
            const float* src = logits + row * ld_logits + pt.src_col;
            float m = -INFINITY;
            for (int c = lane; c < pt.width; c += 64) m = fmaxf(m, src[c]);
            m = wave_max(m);
            float s = 0.f;
            for (int c = lane; c < pt.width; c += 64) s += expf(src[c] - m);
            s = wave_sum(s);
            for (int c = lane; c < pt.width; c += 64) {
                T hi, lo;
                split16<T, NT>(expf(src[c] - m) / s, hi, lo);
                T* dst = out + pidx(row0 + pt.dst_col + c, il);
                dst[0] = hi;
                if (NT > 1) dst[out_plane] = lo;
            }
        }
        int e = pt.dst_col + pt.width;
        kend = e > kend ? e : kend;
    }
    for (int c = kend + lane; c < kpad; c += 64) {
        T* dst = out + pidx(row0 + c, il);
        dst[0] = (T)0.f;
        if (NT > 1) dst[out_plane] = (T)0.f;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// time-layer classifier heads (ProjectingMultiheadAttention, reference acoustic_model.py:237-268)
// ----------------------------------------------------------------------------------------------------------------
// LayerNorm(C) of the projected rows + sinusoidal positions (acoustic_model.py:34-69: column 2k = sin(t * base_k),
// column 2k+1 = cos(t * base_k); `pe_base` holds base per column) -> 16-bit planes [M, kpad] for the in_proj product.
// One wave per row (row = n*T + t); C is arbitrary (class sizes are small, the composed head has C = embedding_size).
template <typename T, int NT>
__global__ __launch_bounds__(256) void time_ln_pe_kernel(const float* __restrict__ x, int64_t M, int C, int T_frames,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float eps, const float* __restrict__ pe_base,
                                                         T* __restrict__ out, int64_t out_plane, int kpad) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* src = x + row * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += src[c];
    const float mu = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        float d = src[c] - mu;
        q += d * d;
    }
    const float rs = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    const float t = (float)(row % T_frames);
    const bool il = plane_is_il<NT>(out_plane);
    for (int c = lane; c < kpad; c += 64) {
        float y = 0.f;
        if (c < C) {
            y = (src[c] - mu) * rs * gamma[c] + beta[c];
            if (pe_base) {
                const float arg = t * pe_base[c];
                y += (c & 1) ? cosf(arg) : sinf(arg);
            }
        }
        T hi, lo;
        split16<T, NT>(y, hi, lo);
        T* dst = out + pidx(row * kpad + c, il);
        dst[0] = hi;
        if (NT > 1) dst[out_plane] = lo;
    }
}

// softmax(q k^T / sqrt(dh) masked to the valid keys of the utterance) v over the frames of one utterance, fp32 on the
// vector ALU: one wave per (utterance, head, query frame).  Lanes are (key group, d) pairs: DP = pow2 >= min(dh, 64)
// lanes hold the dh axis, 64 / DP groups stride over the keys.  Scores go through LDS, `kc` keys at a time (per wave: kc scores,
// the scaled query and the output accumulator): an utterance with more valid keys than that is walked in chunks with the running
// maximum / sum of the online softmax, so there is no length limit (nn.MultiheadAttention has none, acoustic_model.py:255-268);
// up to kc keys -- every utterance below ~ 3 minutes -- the arithmetic is that of the plain two-pass softmax (0 * 0 + x steps).
// Queries of padded frames are computed like upstream (only keys are masked, nn.MultiheadAttention key_padding_mask).
template <typename T, int NT>
__global__ __launch_bounds__(256) void time_attention_kernel(const float* __restrict__ qkv, const int* __restrict__ frame_len,
                                                             int T_frames, int C, int dh, int dp, int kc, T* __restrict__ out,
                                                             int64_t out_plane, int kpad) {
    extern __shared__ float time_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wave, hd = blockIdx.y, n = blockIdx.z;
    if (t >= T_frames) return;
    float* sc = time_lds + (size_t)wave * (kc + 2 * dh);
    float* qs = sc + kc;
    float* oa = qs + dh;
    const int64_t ld = 3 * (int64_t)C;
    const float* base = qkv + (int64_t)n * T_frames * ld + hd * dh;
    const float scale = 1.0f / sqrtf((float)dh);
    for (int d = lane; d < dh; d += 64) {
        qs[d] = base[(int64_t)t * ld + d] * scale;
        oa[d] = 0.f;
    }
    const int len = frame_len[n];
    const int groups = 64 / dp, kg = lane / dp, dl = lane % dp;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < len; k0 += kc) {
        const int nk = len - k0 < kc ? len - k0 : kc;
        float mc = -INFINITY;
        for (int key = lane; key < nk; key += 64) {
            const float* kr = base + (int64_t)(k0 + key) * ld + C;
            float a = 0.f;
            for (int d = 0; d < dh; ++d) a = fmaf(qs[d], kr[d], a);
            sc[key] = a;
            mc = fmaxf(mc, a);
        }
        const float mn = fmaxf(m, wave_max(mc));
        const float f = expf(m - mn);  // first chunk: exp(-inf) = 0
        float sum = 0.f;
        for (int key = lane; key < nk; key += 64) {
            float e = expf(sc[key] - mn);
            sc[key] = e;
            sum += e;
        }
        l = l * f + wave_sum(sum);
        m = mn;
        for (int d0 = 0; d0 < dh; d0 += dp) {
            const int d = d0 + dl;
            float o = 0.f;
            if (d < dh) {
                const float* vr = base + (int64_t)k0 * ld + 2 * C + d;
                for (int key = kg; key < nk; key += groups) o = fmaf(sc[key], vr[(int64_t)key * ld], o);
            }
            for (int off = dp; off < 64; off <<= 1) o += __shfl_xor(o, off);
            if (kg == 0 && d < dh) oa[d] = oa[d] * f + o;
        }
    }
    const float inv = 1.0f / l;
    const int64_t orow = ((int64_t)n * T_frames + t) * kpad;
    for (int d0 = 0; d0 < dh; d0 += dp) {
        const int d = d0 + dl;
        if (kg == 0 && d < dh) {
            T hi, lo;
            split16<T, NT>(oa[d] * inv, hi, lo);
            T* dst = out + pidx(orow + hd * dh + d, plane_is_il<NT>(out_plane));
            dst[0] = hi;
            if (NT > 1) dst[out_plane] = lo;
        }
    }
    if (hd == 0)
        for (int c = C + lane; c < kpad; c += 64) {
            T* dst = out + pidx(orow + c, plane_is_il<NT>(out_plane));
            dst[0] = (T)0.f;
            if (NT > 1) dst[out_plane] = (T)0.f;
        }
}

// ----------------------------------------------------------------------------------------------------------------
// per-head log-softmax (reference estimator.py:1041-1045), batch-major logits -> time-major [T,N,C] outputs.
// Frames t >= frame_len[n] are published as zeros: upstream leaves layout-dependent garbage there (padded queries run
// through every layer), here the padded and the packed row layouts must hand consumers of whole [T, N, C] tensors the
// same bytes (the contract: frames beyond `lengths` carry no information).
// ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void logsoftmax_out_kernel(const OutDesc* __restrict__ descs, int n_out,
                                                             const float* __restrict__ logits, int64_t ld, int N, int T,
                                                             const int* __restrict__ frame_len, int log_probs,
                                                             float* __restrict__ out, int* __restrict__ nonfinite,
                                                             const int* __restrict__ row_off) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // row = n*T + t
    if (row >= (int64_t)N * T) return;
    const int n = (int)(row / T), t = (int)(row % T);
    if (t >= frame_len[n]) {
        for (int o = 0; o < n_out; ++o) {
            const OutDesc d = descs[o];
            float* dst = out + (int64_t)T * N * d.prefix + ((int64_t)t * N + n) * d.C;
            for (int c = lane; c < d.C; c += 64) dst[c] = 0.f;
        }
        return;
    }
    const float* src_row = logits + (row_off ? (int64_t)row_off[n] + t : row) * ld;  // packed rows: utterances back to back
    if (nonfinite) {
        // range check of the 16-bit planes (fp16 overflows at 65504): whatever overflowed upstream has become an infinity or
        // a NaN in this frame's logits by now (amx_check_finite reads the counter)
        bool bad = false;
        for (int o = 0; o < n_out; ++o) {
            const OutDesc d = descs[o];
            for (int c = lane; c < d.C; c += 64) bad |= !__builtin_isfinite(src_row[d.col + c]);
        }
        if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicAdd(nonfinite, 1);
    }
    // narrow outputs (the attribute classifiers: 4 classes each): one LANE per output, everything lane-local -- a wave
    // reduction per 4-class output (36 of them per frame) made this kernel 20x slower than its 11 MB of traffic
    constexpr int NARROW = 8;
    for (int o0 = 0; o0 < n_out; o0 += 64) {
        const int o = o0 + lane;
        if (o < n_out) {
            const OutDesc d = descs[o];
            if (d.C <= NARROW) {
                const float* src = src_row + d.col;
                float* dst = out + (int64_t)T * N * d.prefix + ((int64_t)t * N + n) * d.C;
                float v[NARROW];
#pragma unroll
                for (int c = 0; c < NARROW; ++c) v[c] = c < d.C ? src[c] : -INFINITY;
                float lse = 0.f;
                if (log_probs) {
                    float m = v[0];
#pragma unroll
                    for (int c = 1; c < NARROW; ++c) m = fmaxf(m, v[c]);
                    float sum = 0.f;
#pragma unroll
                    for (int c = 0; c < NARROW; ++c) sum += c < d.C ? expf(v[c] - m) : 0.f;
                    lse = m + logf(sum);
                }
#pragma unroll
                for (int c = 0; c < NARROW; ++c)
                    if (c < d.C) dst[c] = v[c] - lse;
            }
        }
    }
    // wide outputs (phoneme / phone inventories): the whole wave per output
    for (int o = 0; o < n_out; ++o) {
        const OutDesc d = descs[o];
        if (d.C <= NARROW) continue;
        const float* src = src_row + d.col;
        float* dst = out + (int64_t)T * N * d.prefix + ((int64_t)t * N + n) * d.C;
        float lse = 0.f;
        if (log_probs) {
            float m = -INFINITY;
            for (int c = lane; c < d.C; c += 64) m = fmaxf(m, src[c]);
            m = wave_max(m);
            float s = 0.f;
            for (int c = lane; c < d.C; c += 64) s += expf(src[c] - m);
            s = wave_sum(s);
            lse = m + logf(s);
        }
        for (int c = lane; c < d.C; c += 64) dst[c] = src[c] - lse;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// greedy CTC (reference predictions.py:194-207): argmax, collapse repeats, drop blank 0, 1-based start timesteps,
// score = sum of the per-frame maxima.  One block per (output, utterance).
// ----------------------------------------------------------------------------------------------------------------
// one workgroup decodes one utterance of one output: frame t of the utterance is the C floats at base + t * stride_t.
// The argmax indices of CTC_CHUNK frames at a time live in LDS (`chunk` = min(T, CTC_CHUNK) ints); an utterance longer than that is
// walked chunk by chunk with the last index and the output position carried over, so there is no length limit (the reference's
// decoder has none, predictions.py:194-207).  A thread adds the maxima of frames tid, tid + 256, ... in ascending order whatever
// the chunking (CTC_CHUNK % 256 == 0) and the block total is one fixed tree: scores do not depend on T's relation to the chunk.
constexpr int CTC_CHUNK = 8192;
__device__ __forceinline__ void greedy_ctc_block(const float* __restrict__ base, int64_t stride_t, int C, int len, int chunk,
                                                 int blank, int64_t* __restrict__ tok, int64_t* __restrict__ ts, int* __restrict__ count,
                                                 float* __restrict__ score_out, unsigned char* smem) {
    int* idx = (int*)smem;          // [chunk]
    int* scan = idx + chunk;        // [256]
    float* fred = (float*)(scan + 256);  // [256]
    float score = 0.f;
    int pos_base = 0, prev = -1;
    for (int b = 0; b < len; b += chunk) {
        const int n = len - b < chunk ? len - b : chunk;
        for (int t = threadIdx.x; t < n; t += 256) {
            const float* p = base + (int64_t)(b + t) * stride_t;
            float best = p[0];
            int bi = 0;
            for (int c = 1; c < C; ++c) {
                float v = p[c];
                if (v > best) { best = v; bi = c; }
            }
            idx[t] = bi;
            score += best;
        }
        __syncthreads();
        // contiguous segment per thread
        const int seg = (n + 255) / 256;
        const int lo = threadIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
        int cnt = 0;
        for (int t = lo; t < hi; ++t) {
            const bool start = b + t == 0 || idx[t] != (t > 0 ? idx[t - 1] : prev);
            cnt += (start && idx[t] != blank) ? 1 : 0;
        }
        scan[threadIdx.x] = cnt;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            int v = threadIdx.x >= off ? scan[threadIdx.x - off] : 0;
            __syncthreads();
            scan[threadIdx.x] += v;
            __syncthreads();
        }
        int pos = pos_base + scan[threadIdx.x] - cnt;  // exclusive prefix
        for (int t = lo; t < hi; ++t) {
            const bool start = b + t == 0 || idx[t] != (t > 0 ? idx[t - 1] : prev);
            if (start && idx[t] != blank) {
                tok[pos] = idx[t];
                ts[pos] = b + t + 1;
                ++pos;
            }
        }
        const int total = scan[255], last = idx[n - 1];
        __syncthreads();  // every thread has read idx / scan of this chunk before the next one overwrites them
        pos_base += total;
        prev = last;
    }
    fred[threadIdx.x] = score;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        float f = threadIdx.x + off < 256 ? fred[threadIdx.x + off] : 0.f;
        __syncthreads();
        if ((threadIdx.x & (2 * off - 1)) == 0) fred[threadIdx.x] += f;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *count = pos_base;
        *score_out = fred[0];
    }
}

__global__ __launch_bounds__(256) void greedy_ctc_kernel(const OutDesc* __restrict__ descs, const float* __restrict__ out,
                                                         const int* __restrict__ frame_len, int N, int T,
                                                         int64_t* __restrict__ tokens, int64_t* __restrict__ timesteps,
                                                         int* __restrict__ counts, float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int o = blockIdx.y, n = blockIdx.x;
    const OutDesc d = descs[o];
    const int len = frame_len[n] < T ? frame_len[n] : T;
    const float* base = out + (int64_t)T * N * d.prefix + (int64_t)n * d.C;
    greedy_ctc_block(base, (int64_t)N * d.C, d.C, len, T < CTC_CHUNK ? T : CTC_CHUNK, 0, tokens + ((int64_t)o * N + n) * T, timesteps + ((int64_t)o * N + n) * T,
                     counts + o * N + n, scores + o * N + n, smem);
}

// the reference decoder's own signature (predictions.py:194): one [N, T, C] emission tensor with arbitrary strides
__global__ __launch_bounds__(256) void greedy_ctc_emissions_kernel(const float* __restrict__ emissions, int64_t stride_n,
                                                                   int64_t stride_t, const int* __restrict__ frame_len, int T,
                                                                   int C, int blank, int64_t* __restrict__ tokens,
                                                                   int64_t* __restrict__ timesteps, int* __restrict__ counts,
                                                                   float* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = blockIdx.x;
    const int len = frame_len[n] < T ? frame_len[n] : T;
    greedy_ctc_block(emissions + (int64_t)n * stride_n, stride_t, C, len < 0 ? 0 : len, T < CTC_CHUNK ? T : CTC_CHUNK, blank, tokens + (int64_t)n * T,
                     timesteps + (int64_t)n * T, counts + n, scores + n, smem);
}

// ----------------------------------------------------------------------------------------------------------------
// weight packers
// ----------------------------------------------------------------------------------------------------------------
template <typename T, int NT>
__global__ void pack_matrix_kernel(const float* __restrict__ src, int rows, int cols, int64_t srs, int64_t scs, float scale,
                                   T* __restrict__ dst, int64_t dst_plane, int64_t ldd, int cols_pad) {
    int64_t total = (int64_t)rows * cols_pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int r = (int)(i / cols_pad), c = (int)(i % cols_pad);
        float v = c < cols ? src[r * srs + c * scs] * scale : 0.f;
        T hi, lo;
        split16<T, NT>(v, hi, lo);
        T* d = dst + pidx((int64_t)r * ldd + c, plane_is_il<NT>(dst_plane));
        d[0] = hi;
        if (NT > 1) d[dst_plane] = lo;
    }
}

template <typename T, int NT>
__global__ void pack_conv_w_kernel(const float* __restrict__ src, int Co, int Ci, int k, float scale, T* __restrict__ dst,
                                   int64_t dst_plane, int tap_minor_slice) {
    // dst[co][j*Ci + ci] = src[co][ci][j]; tap-minor (slice S): dst[co][((ci / S) * k + pos) * S + ci % S] = src[co][ci][(k - pos) % k]
    int64_t total = (int64_t)Co * Ci * k;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int ci, j, co;
        if (tap_minor_slice > 0) {
            const int S = tap_minor_slice;
            const int within = (int)(i % S);
            int64_t r = i / S;
            j = (int)(r % k);
            j = (k - j) % k;  // position 0, 1, 2 of a channel slice holds tap 0, 2, 1 (GemmParams.a_taps: shared rows back to back)
            r /= k;
            ci = (int)(r % (Ci / S)) * S + within;
            co = (int)(r / (Ci / S));
        } else {
            ci = (int)(i % Ci);
            int64_t r = i / Ci;
            j = (int)(r % k);
            co = (int)(r / k);
        }
        T hi, lo;
        split16<T, NT>(src[((int64_t)co * Ci + ci) * k + j] * scale, hi, lo);
        T* d = dst + pidx(i, plane_is_il<NT>(dst_plane));  // rows of Ci * k elements
        d[0] = hi;
        if (NT > 1) d[dst_plane] = lo;
    }
}

__global__ __launch_bounds__(256) void posconv_norm_kernel(const float* __restrict__ v, int64_t rows /*D*cg*/, int k,
                                                           float* __restrict__ norm) {
    // weight_norm(dim=2): one norm per kernel tap over dims (0,1)
    const int tap = blockIdx.x;
    double s = 0;
    for (int64_t r = threadIdx.x; r < rows; r += 256) {
        double x = v[r * k + tap];
        s += x * x;
    }
    __shared__ double red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) norm[tap] = (float)sqrt(red[0] + red[1] + red[2] + red[3]);
}

template <typename T, int NT>
__global__ void pack_posconv_w_kernel(const float* __restrict__ g, const float* __restrict__ v, const float* __restrict__ norm,
                                      int D, int cg, int k, float scale, T* __restrict__ dst, int64_t dst_plane) {
    // dst[grp][co][tap*cg + ci] = v[grp*cg + co][ci][tap] * (g[tap] / norm[tap])
    int64_t total = (int64_t)D * cg * k;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int ci = (int)(i % cg);
        int64_t r = i / cg;
        int tap = (int)(r % k);
        int co_all = (int)(r / k);  // grp*cg + co
        float w = v[((int64_t)co_all * cg + ci) * k + tap] * (g[tap] / norm[tap]) * scale;
        T hi, lo;
        split16<T, NT>(w, hi, lo);
        dst[i] = hi;
        if (NT > 1) dst[dst_plane + i] = lo;
    }
}

template <typename T, int NT>
__global__ void compose_kernel(const float* __restrict__ emb, int E, const int64_t* __restrict__ idx, int P1, int F, float scale,
                               float* __restrict__ composed, T* __restrict__ dst, int64_t dst_plane, int64_t ldd) {
    // EmbeddingBag(mode="sum") per phone (reference acoustic_model.py:219-232); negative index = unused slot
    int64_t total = (int64_t)P1 * E;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int e = (int)(i % E), p = (int)(i / E);
        float s = 0.f;
        for (int f = 0; f < F; ++f) {
            int64_t r = idx[(int64_t)p * F + f];
            if (r >= 0) s += emb[r * E + e];
        }
        composed[i] = s;
        T hi, lo;
        split16<T, NT>(s * scale, hi, lo);
        T* d = dst + pidx((int64_t)p * ldd + e, plane_is_il<NT>(dst_plane));
        d[0] = hi;
        if (NT > 1) d[dst_plane] = lo;
    }
}

__global__ void scale_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t n, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i] * scale;
}

inline int grid_for(int64_t n, int block = 256, int cap = 8192) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    return (int)(g < cap ? g : cap);
}

}  // namespace

void launch_rownorm(int prec, const float* x, int64_t ldx, int64_t M, int D, const float* gamma1, const float* beta1,
                    int gelu, const float* gamma2, const float* beta2, float eps1, float eps2, void* out_p,
                    int64_t out_plane, int64_t ldp, float* out_f32, int64_t ldo, hipStream_t s) {
    dim3 grid((unsigned)((M + 3) / 4));
    if (D <= 1024) {
        AMX_DISPATCH(prec, hipLaunchKernelGGL((rownorm_kernel<T16, NT, 4>), grid, dim3(256), 0, s, x, ldx, M, D, gamma1, beta1, gelu,
                                              gamma2, beta2, eps1, eps2, (T16*)out_p, out_plane, ldp, out_f32, ldo, nullptr, nullptr, 1));
    } else {
        AMX_DISPATCH(prec, hipLaunchKernelGGL((rownorm_kernel<T16, NT, 8>), grid, dim3(256), 0, s, x, ldx, M, D, gamma1, beta1, gelu,
                                              gamma2, beta2, eps1, eps2, (T16*)out_p, out_plane, ldp, out_f32, ldo, nullptr, nullptr, 1));
    }
}

void launch_ln_rowprep(int prec, const float* x, int64_t ldx, int64_t M, int D, float eps, void* out_p, int64_t out_plane, int64_t ldp,
                       float4* rowps, float2* coef, const int* frame_len, int T_rows, hipStream_t s) {
    dim3 grid((unsigned)((M + 3) / 4));
    if (D <= 1024) {
        AMX_DISPATCH(prec, hipLaunchKernelGGL((ln_rowprep_kernel<T16, NT, 4>), grid, dim3(256), 0, s, x, ldx, M, D, eps, (T16*)out_p, out_plane,
                                              ldp, rowps, coef, frame_len, T_rows));
    } else {
        AMX_DISPATCH(prec, hipLaunchKernelGGL((ln_rowprep_kernel<T16, NT, 8>), grid, dim3(256), 0, s, x, ldx, M, D, eps, (T16*)out_p, out_plane,
                                              ldp, rowps, coef, frame_len, T_rows));
    }
}

void launch_ln_finalize(const float2* partial, int blocks, int64_t M, float eps, float4* rowps, float2* coef, const int* frame_len,
                        int T_rows, hipStream_t s) {
    hipLaunchKernelGGL(ln_finalize_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, partial, blocks, M, eps, rowps, coef,
                       frame_len, T_rows);
}

void launch_rownorm_to_packed(int prec, const float* x, int64_t ldx, int64_t M, int D, const float* gamma1, const float* beta1,
                              int gelu, const float* gamma2, const float* beta2, float eps1, float eps2, void* out_p,
                              int64_t out_plane, int64_t ldp, const int* row_off, const int* frame_len, int T_rows, hipStream_t s) {
    dim3 grid((unsigned)((M + 3) / 4));
    AMX_DISPATCH(prec, hipLaunchKernelGGL((rownorm_kernel<T16, NT>), grid, dim3(256), 0, s, x, ldx, M, D, gamma1, beta1, gelu,
                                          gamma2, beta2, eps1, eps2, (T16*)out_p, out_plane, ldp, nullptr, 0, row_off, frame_len, T_rows));
}

void launch_posconv_pack(int prec, const float* h, int N, int T, int D, int G, int pad_front, int Tpad, void* out,
                         int64_t out_plane, const int* row_off, const int* frame_len, hipStream_t s) {
    int64_t total4 = (int64_t)N * Tpad * D / 4;
    AMX_DISPATCH(prec, hipLaunchKernelGGL((posconv_pack_kernel<T16, NT>), dim3(grid_for(total4)), dim3(256), 0, s, h, N, T, D,
                                          G, pad_front, Tpad, (T16*)out, out_plane, row_off, frame_len));
}

void launch_concat(int prec, const ConcatPart* parts_dev, int n_parts, const float* logits, int64_t ld_logits, int64_t M,
                   void* out, int64_t out_plane, int64_t ldp, int kpad, hipStream_t s) {
    dim3 grid((unsigned)((M + 3) / 4));
    AMX_DISPATCH(prec, hipLaunchKernelGGL((concat_kernel<T16, NT>), grid, dim3(256), 0, s, parts_dev, n_parts, logits,
                                          ld_logits, M, (T16*)out, out_plane, ldp, kpad));
}

void launch_time_ln_pe(int prec, const float* x, int64_t M, int C, int T, const float* gamma, const float* beta, float eps,
                       const float* pe_base, void* out, int64_t out_plane, int kpad, hipStream_t s) {
    dim3 grid((unsigned)((M + 3) / 4));
    AMX_DISPATCH(prec, hipLaunchKernelGGL((time_ln_pe_kernel<T16, NT>), grid, dim3(256), 0, s, x, M, C, T, gamma, beta, eps,
                                          pe_base, (T16*)out, out_plane, kpad));
}

// keys per chunk of the time-layer attention: the whole utterance when 4 waves x (T + 2 dh) floats fit the 160 KiB of a CU
static int time_attention_chunk(int T, int dh) {
    const int room = 160 * 1024 / 16 - 2 * dh;
    return T < room ? T : room;
}
size_t time_attention_lds_bytes(int T, int dh) { return (size_t)4 * (time_attention_chunk(T, dh) + 2 * dh) * sizeof(float); }

template <typename T, int NT>
static void time_attention_launch(const float* qkv, const int* frame_len, int N, int T_frames, int C, int heads, void* out,
                                  int64_t out_plane, int kpad, hipStream_t s) {
    const int dh = C / heads;
    int dp = 1;
    while (dp < dh && dp < 64) dp <<= 1;
    const size_t lds = time_attention_lds_bytes(T_frames, dh);
    auto kernel = time_attention_kernel<T, NT>;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((T_frames + 3) / 4), heads, N), dim3(256), lds, s, qkv, frame_len, T_frames, C,
                       dh, dp, time_attention_chunk(T_frames, dh), (T*)out, out_plane, kpad);
}

void launch_time_attention(int prec, const float* qkv, const int* frame_len, int N, int T, int C, int heads, void* out,
                           int64_t out_plane, int kpad, hipStream_t s) {
    AMX_DISPATCH(prec, (time_attention_launch<T16, NT>(qkv, frame_len, N, T, C, heads, out, out_plane, kpad, s)));
}

void launch_logsoftmax_out(const OutDesc* descs_dev, int n_out, const float* logits, int64_t ld, int N, int T,
                           const int* frame_len, int log_probs, float* out, int* nonfinite, const int* row_off, hipStream_t s) {
    int64_t M = (int64_t)N * T;
    hipLaunchKernelGGL(logsoftmax_out_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, descs_dev, n_out, logits, ld,
                       N, T, frame_len, log_probs, out, nonfinite, row_off);
}

void launch_greedy_ctc(const OutDesc* descs_dev, int n_out, const float* out, const int* frame_len, int N, int T,
                       int64_t* tokens, int64_t* timesteps, int* counts, float* scores, hipStream_t s) {
    size_t lds = (size_t)(T < CTC_CHUNK ? T : CTC_CHUNK) * sizeof(int) + 256 * sizeof(int) + 256 * sizeof(float);
    hipLaunchKernelGGL(greedy_ctc_kernel, dim3(N, n_out), dim3(256), lds, s, descs_dev, out, frame_len, N, T, tokens,
                       timesteps, counts, scores);
}

void launch_greedy_ctc_emissions(const float* emissions, int64_t stride_n, int64_t stride_t, const int* frame_len, int N, int T,
                                 int C, int blank, int64_t* tokens, int64_t* timesteps, int* counts, float* scores, hipStream_t s) {
    size_t lds = (size_t)(T < CTC_CHUNK ? T : CTC_CHUNK) * sizeof(int) + 256 * sizeof(int) + 256 * sizeof(float);
    hipLaunchKernelGGL(greedy_ctc_emissions_kernel, dim3(N), dim3(256), lds, s, emissions, stride_n, stride_t, frame_len, T, C,
                       blank, tokens, timesteps, counts, scores);
}

void launch_pack_matrix(int prec, const float* src, int rows, int cols, int64_t src_row_stride, int64_t src_col_stride,
                        float scale, void* dst, int64_t dst_plane, int64_t ldd, int cols_pad, hipStream_t s) {
    int64_t total = (int64_t)rows * cols_pad;
    AMX_DISPATCH(prec, hipLaunchKernelGGL((pack_matrix_kernel<T16, NT>), dim3(grid_for(total)), dim3(256), 0, s, src, rows,
                                          cols, src_row_stride, src_col_stride, scale, (T16*)dst, dst_plane, ldd, cols_pad));
}

void launch_pack_conv_w(int prec, const float* src, int Co, int Ci, int k, float scale, void* dst, int64_t dst_plane, hipStream_t s,
                        int tap_minor_slice) {
    int64_t total = (int64_t)Co * Ci * k;
    AMX_DISPATCH(prec, hipLaunchKernelGGL((pack_conv_w_kernel<T16, NT>), dim3(grid_for(total)), dim3(256), 0, s, src, Co, Ci, k,
                                          scale, (T16*)dst, dst_plane, tap_minor_slice));
}

void launch_pack_posconv_w(int prec, const float* g, const float* v, int D, int cg, int k, float scale, float* norm_scratch, void* dst,
                           int64_t dst_plane, hipStream_t s) {
    hipLaunchKernelGGL(posconv_norm_kernel, dim3(k), dim3(256), 0, s, v, (int64_t)D * cg, k, norm_scratch);
    int64_t total = (int64_t)D * cg * k;
    AMX_DISPATCH(prec, hipLaunchKernelGGL((pack_posconv_w_kernel<T16, NT>), dim3(grid_for(total)), dim3(256), 0, s, g, v,
                                          norm_scratch, D, cg, k, scale, (T16*)dst, dst_plane));
}

void launch_compose(int prec, const float* emb, int E, const int64_t* idx, int P1, int F, float scale, float* composed_f32, void* dst,
                    int64_t dst_plane, int64_t ldd, hipStream_t s) {
    int64_t total = (int64_t)P1 * E;
    AMX_DISPATCH(prec, hipLaunchKernelGGL((compose_kernel<T16, NT>), dim3(grid_for(total)), dim3(256), 0, s, emb, E, idx, P1, F,
                                          scale, composed_f32, (T16*)dst, dst_plane, ldd));
}

// Zero fills and device copies of a forward pass as KERNELS: a pass holds no hipMemset / hipMemcpy.  A pass may be recorded into
// a HIP graph, and on this runtime (ROCm 7.2) replays of a recorded pass -- once eager passes had run between them -- left
// 0x01010101 in the non-finite frame counter that the pass's memset node zeroes (every other replay: one of the two recordings
// of a caller that alternates between two output buffers; tools/debug_range2.py, profiles/r05_memset_node_replay.log).  Found by
// the range report itself.  Two changes removed it, not separated: no memset / memcpy node in a pass (kernel nodes carry their
// arguments by value), and the graph template now lives as long as its instance (amx_api.hip).  Sizes are multiples of 4 bytes,
// pointers 4-byte aligned (callers: fp16 plane rows of 128 bytes, fp32 rows, one int counter).
namespace {
__global__ __launch_bounds__(256) void zero_fill_kernel(uint32_t* __restrict__ p, size_t words) {
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool aligned = ((uintptr_t)p & 15) == 0;
    const size_t quads = aligned ? words / 4 : 0;
    for (size_t q = i; q < quads; q += stride) ((uint4*)p)[q] = make_uint4(0, 0, 0, 0);
    for (size_t w = quads * 4 + i; w < words; w += stride) p[w] = 0;
}
__global__ __launch_bounds__(256) void copy_words_kernel(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, size_t words) {
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool aligned = (((uintptr_t)dst | (uintptr_t)src) & 15) == 0;
    const size_t quads = aligned ? words / 4 : 0;
    for (size_t q = i; q < quads; q += stride) ((uint4*)dst)[q] = ((const uint4*)src)[q];
    for (size_t w = quads * 4 + i; w < words; w += stride) dst[w] = src[w];
}
__global__ __launch_bounds__(256) void zero_fill_2d_kernel(unsigned char* __restrict__ base, size_t pitch, size_t width_words) {
    uint32_t* row = (uint32_t*)(base + (size_t)blockIdx.y * pitch);
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < width_words; w += (size_t)gridDim.x * 256) row[w] = 0;
}
// (amx_debug_scribble) `pattern` over `words` 32-bit words, then the `tail` < 4 bytes behind them from its low bytes
__global__ __launch_bounds__(256) void fill_words_kernel(uint32_t* __restrict__ p, size_t words, uint32_t pattern, int tail) {
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool aligned = ((uintptr_t)p & 15) == 0;
    const size_t quads = aligned ? words / 4 : 0;
    for (size_t q = i; q < quads; q += stride) ((uint4*)p)[q] = make_uint4(pattern, pattern, pattern, pattern);
    for (size_t w = quads * 4 + i; w < words; w += stride) p[w] = pattern;
    if (i < (size_t)tail) ((unsigned char*)(p + words))[i] = (unsigned char)(pattern >> (8 * i));
}
}  // namespace

void launch_zero(void* p, size_t bytes, hipStream_t s) {
    if (bytes == 0) return;
    const size_t words = bytes / 4;
    size_t blocks = (words / 4 + 255) / 256 + 1;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (uint32_t*)p, words);
}

// device-to-device copy of a pass as a kernel, for the same reason (bytes a multiple of 4)
void launch_copy(void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return;
    const size_t words = bytes / 4;
    size_t blocks = (words / 4 + 255) / 256 + 1;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(copy_words_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (uint32_t*)dst, (const uint32_t*)src, words);
}

void launch_zero_2d(void* base, size_t pitch, size_t width_bytes, size_t rows, hipStream_t s) {
    if (width_bytes == 0 || rows == 0) return;
    const size_t words = width_bytes / 4;
    size_t bx = (words + 255) / 256;
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(zero_fill_2d_kernel, dim3((unsigned)bx, (unsigned)rows), dim3(256), 0, s, (unsigned char*)base, pitch, words);
}

void launch_fill16(void* p, size_t bytes, uint32_t word16, hipStream_t s) {
    if (bytes == 0) return;
    const size_t words = bytes / 4;
    size_t blocks = (words / 4 + 255) / 256 + 1;
    if (blocks > 4096) blocks = 4096;
    const uint32_t pattern = (word16 & 0xffffu) | (word16 << 16);
    hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (uint32_t*)p, words, pattern, (int)(bytes - words * 4));
}

void launch_scale_copy(const float* src, float* dst, int64_t n, float scale, hipStream_t s) {
    hipLaunchKernelGGL(scale_copy_kernel, dim3(grid_for(n)), dim3(256), 0, s, src, dst, n, scale);
}

// ---------------------------------------------------------------------------------------------------------------
// packed rows: the encoder layers of a ragged batch run on the valid frames only
// ---------------------------------------------------------------------------------------------------------------
namespace {
template <bool UNPACK>
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ row_off,
                                                        const int* __restrict__ frame_len, int T, int D) {
    const int n = blockIdx.y, t = blockIdx.x;
    if (t >= frame_len[n]) return;
    const int64_t padded_row = (int64_t)n * T + t, packed_row = (int64_t)row_off[n] + t;
    const float4* s4 = (const float4*)(src + (UNPACK ? packed_row : padded_row) * D);
    float4* d4 = (float4*)(dst + (UNPACK ? padded_row : packed_row) * D);
    for (int c = threadIdx.x; c < D / 4; c += 256) d4[c] = s4[c];
}
}  // namespace

void launch_pack_rows(const float* padded, float* packed, const int* row_off, const int* frame_len, int N, int T, int D, bool unpack,
                      hipStream_t s) {
    dim3 grid(T, N);
    if (unpack) hipLaunchKernelGGL(pack_rows_kernel<true>, grid, dim3(256), 0, s, packed, const_cast<float*>(padded), row_off, frame_len, T, D);
    else hipLaunchKernelGGL(pack_rows_kernel<false>, grid, dim3(256), 0, s, padded, packed, row_off, frame_len, T, D);
}

}  // namespace amx
