// Conv layer 0 of the Allophant forward path on gfx950 (64-wide wavefronts): input normalisation statistics, the fused
// first layer (C_in = 1: conv + LayerNorm over channels or GroupNorm over time + GELU -> 16-bit planes) in its scalar and
// matrix-pipe forms, the GroupNorm statistics passes, and the one function that routes a shape to them (conv0_route).
#include "amx_common.h"

namespace amx {

namespace {

// ----------------------------------------------------------------------------------------------------------------
// input normalisation (reference acoustic_model.py:762-767): statistics only; applied on the fly by conv layer 0
// ----------------------------------------------------------------------------------------------------------------
constexpr int STAT_CHUNKS = 64;

__global__ __launch_bounds__(256) void audio_stats_kernel(const float* __restrict__ audio, const int64_t* __restrict__ lengths,
                                                          int64_t L, double* __restrict__ partial) {
    const int n = blockIdx.y, c = blockIdx.x;
    int64_t per = (L + STAT_CHUNKS - 1) / STAT_CHUNKS;
    per = (per + 3) & ~(int64_t)3;
    int64_t lo = c * per, hi = lo + per < L ? lo + per : L;
    const int64_t len = lengths[n];
    const float* row = audio + (int64_t)n * L;
    double s_all = 0, s_val = 0, q_val = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        double x = row[i];
        s_all += x;
        if (i < len) { s_val += x; q_val += x * x; }
    }
    __shared__ double red[3][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s_all += __shfl_xor(s_all, o);
        s_val += __shfl_xor(s_val, o);
        q_val += __shfl_xor(q_val, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s_all;
        red[1][threadIdx.x >> 6] = s_val;
        red[2][threadIdx.x >> 6] = q_val;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        partial[((int64_t)n * STAT_CHUNKS + c) * 3 + threadIdx.x] = v;
    }
}

__global__ void audio_stats_final_kernel(const double* __restrict__ partial, const int64_t* __restrict__ lengths, int N,
                                         float* __restrict__ mean_rstd, int do_normalize) {
    int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    if (!do_normalize) { mean_rstd[2 * n] = 0.f; mean_rstd[2 * n + 1] = 1.f; return; }
    double s_all = 0, s_val = 0, q_val = 0;
    for (int c = 0; c < STAT_CHUNKS; ++c) {
        s_all += partial[((int64_t)n * STAT_CHUNKS + c) * 3 + 0];
        s_val += partial[((int64_t)n * STAT_CHUNKS + c) * 3 + 1];
        q_val += partial[((int64_t)n * STAT_CHUNKS + c) * 3 + 2];
    }
    double len = (double)lengths[n];
    double mean = s_all / len;  // the reference sums the whole padded row (zero padding contract)
    double var = (q_val - 2.0 * mean * s_val + len * mean * mean) / len;
    if (var < 0) var = 0;
    mean_rstd[2 * n] = (float)mean;
    mean_rstd[2 * n + 1] = (float)(1.0 / sqrt(var + 1e-7));
}

// ----------------------------------------------------------------------------------------------------------------
// conv layer 0 (C_in = 1, kernel KW, stride s) + LayerNorm over channels + exact GELU  ->  16-bit planes [N*T1, C]
// One wave per output frame, lane owns CPL consecutive channels (weights in registers), window staged in LDS.
// HBM-bound: reads 4 B/sample once, writes 2*NT bytes per output element.
// ----------------------------------------------------------------------------------------------------------------
constexpr int C0_FRAMES = 128;  // frames per workgroup: amortises the per-lane weight loads

// GN (the group-norm feature extractor, `feat_extract_norm="group"`: GroupNorm(C groups of one channel) over TIME behind conv
// layer 0 instead of a LayerNorm over channels): the statistics come from conv0_gn_stats_kernel, and `gamma` / `beta` are the
// per-(utterance, channel) scale and shift [N, C] that conv0_gn_final_kernel folded them into -- y = acc * scale + shift, no
// cross-lane reduction.
template <typename T, int NT, int CPL, int KW, bool GN>
__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ audio, const int64_t* __restrict__ lengths,
                                                    const float* __restrict__ mean_rstd, int64_t L, int T1, int C, int k,
                                                    int stride, const float* __restrict__ w, const float* __restrict__ b,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, int do_normalize, T* __restrict__ out, int64_t out_plane,
                                                    int skip_padding) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* win = (float*)smem;
    const int n = blockIdx.y;
    const int f0 = blockIdx.x * C0_FRAMES;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwin = C0_FRAMES * stride + k;
    const int64_t len = lengths[n];
    // ragged batch: frames past the utterance's own (len - k) / stride + 1 feed no valid frame of any later layer
    if (skip_padding && (int64_t)f0 * stride + k > len && f0 > 0) return;
    const float mean = mean_rstd[2 * n], rstd = mean_rstd[2 * n + 1];
    const int64_t s0 = (int64_t)f0 * stride;
    for (int i = threadIdx.x; i < nwin; i += 256) {
        int64_t pos = s0 + i;
        float x = 0.f;
        if (pos < L) {
            x = audio[(int64_t)n * L + pos];
            if (do_normalize) x = pos < len ? (x - mean) * rstd : 0.f;
        }
        win[i] = x;
    }
    const int c0 = lane * CPL;
    const bool active = c0 < C;
    if (GN) { gamma += (int64_t)n * C; beta += (int64_t)n * C; }
    float wr[CPL][KW], br[CPL], gr[CPL], be[CPL];
    if ((CPL * KW) % 4 == 0 && k == KW && c0 + CPL <= C) {
        // this lane's CPL x KW weights are contiguous and 16-byte aligned: branch-free vector loads (the per-element
        // predicated loads of the general path cost as much as the block's arithmetic)
        float flat[CPL * KW];
        const float4* src = (const float4*)(w + (int64_t)c0 * KW);
#pragma unroll
        for (int q = 0; q < CPL * KW / 4; ++q) {
            const float4 v = src[q];
            flat[4 * q] = v.x; flat[4 * q + 1] = v.y; flat[4 * q + 2] = v.z; flat[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
#pragma unroll
            for (int j = 0; j < KW; ++j) wr[i][j] = flat[i * KW + j];
            br[i] = b[c0 + i];
            gr[i] = gamma[c0 + i];
            be[i] = beta[c0 + i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            int c = c0 + i;
            bool ok = c < C;
#pragma unroll
            for (int j = 0; j < KW; ++j) wr[i][j] = (ok && j < k) ? w[c * k + j] : 0.f;
            br[i] = ok ? b[c] : 0.f;
            gr[i] = ok ? gamma[c] : 0.f;
            be[i] = ok ? beta[c] : 0.f;
        }
    }
    __syncthreads();
    const float invC = 1.0f / (float)C;
    // two frames per wave iteration: the two dependent chains (conv -> mean -> variance -> GELU) interleave
    constexpr int FPI = 2;
    if constexpr (CPL % 2 == 0) {
        // channel pairs on the packed fp32 pipe (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32, packed 16-bit converts): the
        // kernel is VALU-bound, and this halves the instructions of the convolution, the normalisation and the split
        typedef typename Vec2<T>::type V2;
        constexpr int CP = CPL / 2;
        f32x2 w2[CP][KW], b2[CP], g2[CP], be2[CP];
#pragma unroll
        for (int i = 0; i < CP; ++i) {
#pragma unroll
            for (int j = 0; j < KW; ++j) w2[i][j] = f32x2{wr[2 * i][j], wr[2 * i + 1][j]};
            b2[i] = f32x2{br[2 * i], br[2 * i + 1]};
            g2[i] = f32x2{gr[2 * i], gr[2 * i + 1]};
            be2[i] = f32x2{be[2 * i], be[2 * i + 1]};
        }
        for (int f = wave * FPI; f < C0_FRAMES; f += 4 * FPI) {
            f32x2 acc[FPI][CP];
#pragma unroll
            for (int u = 0; u < FPI; ++u)
#pragma unroll
                for (int i = 0; i < CP; ++i) acc[u][i] = b2[i];
#pragma unroll
            for (int j = 0; j < KW; ++j) {
#pragma unroll
                for (int u = 0; u < FPI; ++u) {
                    const float x = j < k ? win[(f + u) * stride + j] : 0.f;  // f + u < C0_FRAMES: inside the staged window
                    const f32x2 xx = {x, x};
#pragma unroll
                    for (int i = 0; i < CP; ++i) acc[u][i] = w2[i][j] * xx + acc[u][i];
                }
            }
            // channels beyond C carry zero weights and bias, so they add nothing to the sums (c0 + CPL <= C or lane idle)
            float mu[FPI], rs[FPI];
            if constexpr (!GN) {
#pragma unroll
                for (int u = 0; u < FPI; ++u) {
                    f32x2 s2 = acc[u][0];
#pragma unroll
                    for (int i = 1; i < CP; ++i) s2 += acc[u][i];
                    mu[u] = wave_sum(active ? s2[0] + s2[1] : 0.f) * invC;
                }
#pragma unroll
                for (int u = 0; u < FPI; ++u) {
                    const f32x2 m2 = {mu[u], mu[u]};
                    f32x2 q2 = {0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < CP; ++i) {
                        const f32x2 d = acc[u][i] - m2;
                        q2 = d * d + q2;
                    }
                    rs[u] = 1.0f / sqrtf(wave_sum(active ? q2[0] + q2[1] : 0.f) * invC + eps);
                }
            } else {
#pragma unroll
                for (int u = 0; u < FPI; ++u) { mu[u] = 0.f; rs[u] = 1.f; }
            }
#pragma unroll
            for (int u = 0; u < FPI; ++u) {
                const int t = f0 + f + u;
                V2 hi[CP], lo[CP];
                const f32x2 r2 = {rs[u], rs[u]}, m2 = {mu[u], mu[u]};
#pragma unroll
                for (int i = 0; i < CP; ++i) {
                    const f32x2 v = GN ? acc[u][i] * g2[i] + be2[i] : (acc[u][i] - m2) * r2 * g2[i] + be2[i];
                    f32x2 y = gelu_fast2(v);
                    // one register pair for y: its 16-bit image and the residual are taken from the same value (see split16)
                    asm volatile("" : "+v"(y));
                    hi[i] = __builtin_convertvector(y, V2);
                    if (NT > 1) {
                        asm volatile("" : "+v"(hi[i]));
                        const f32x2 back = {(float)hi[i][0], (float)hi[i][1]};
                        lo[i] = __builtin_convertvector(y - back, V2);
                    }
                }
                if (active && t < T1) {
                    T* dst = out + pidx(((int64_t)n * T1 + t) * C + c0, plane_is_il<NT>(out_plane));
                    if constexpr (CPL == 8) {
                        union { V2 h[4]; typename Vec8<T>::type v; } hv, lv;
#pragma unroll
                        for (int i = 0; i < 4; ++i) { hv.h[i] = hi[i]; if (NT > 1) lv.h[i] = lo[i]; }
                        *(typename Vec8<T>::type*)dst = hv.v;
                        if (NT > 1) *(typename Vec8<T>::type*)(dst + out_plane) = lv.v;
                    } else {
#pragma unroll
                        for (int i = 0; i < CP; ++i) {
                            *(V2*)(dst + 2 * i) = hi[i];
                            if (NT > 1) *(V2*)(dst + out_plane + 2 * i) = lo[i];
                        }
                    }
                }
            }
        }
        return;
    }
    for (int f = wave * FPI; f < C0_FRAMES; f += 4 * FPI) {
        float acc[FPI][CPL];
#pragma unroll
        for (int u = 0; u < FPI; ++u)
#pragma unroll
            for (int i = 0; i < CPL; ++i) acc[u][i] = br[i];
#pragma unroll
        for (int j = 0; j < KW; ++j) {
#pragma unroll
            for (int u = 0; u < FPI; ++u) {
                const float x = j < k ? win[(f + u) * stride + j] : 0.f;  // f + u < C0_FRAMES: inside the staged window
#pragma unroll
                for (int i = 0; i < CPL; ++i) acc[u][i] = fmaf(wr[i][j], x, acc[u][i]);
            }
        }
        float mu[FPI], rs[FPI];
        if constexpr (!GN) {
#pragma unroll
            for (int u = 0; u < FPI; ++u) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < CPL; ++i) s += (c0 + i < C) ? acc[u][i] : 0.f;
                mu[u] = wave_sum(s) * invC;
            }
#pragma unroll
            for (int u = 0; u < FPI; ++u) {
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    float d = acc[u][i] - mu[u];
                    q += (c0 + i < C) ? d * d : 0.f;
                }
                rs[u] = 1.0f / sqrtf(wave_sum(q) * invC + eps);
            }
        } else {
#pragma unroll
            for (int u = 0; u < FPI; ++u) { mu[u] = 0.f; rs[u] = 1.f; }
        }
#pragma unroll
        for (int u = 0; u < FPI; ++u) {
            const int t = f0 + f + u;
            T hi[CPL], lo[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                float y = gelu_fast((acc[u][i] - mu[u]) * rs[u] * gr[i] + be[i]);
                split16<T, NT>(y, hi[i], lo[i]);
            }
            if (active && t < T1) {
                T* dst = out + pidx(((int64_t)n * T1 + t) * C + c0, plane_is_il<NT>(out_plane));
#pragma unroll
                for (int i = 0; i < CPL; ++i)
                    if (c0 + i < C) {
                        dst[i] = hi[i];
                        if (NT > 1) dst[out_plane + i] = lo[i];
                    }
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------
// conv layer 0 on the matrix pipe (round 5; k = 10, C = 512, LayerNorm variant -- every released wav2vec 2.0 / XLS-R shape).
//
// conv0_kernel above is VALU-bound (0.45 ms of its 0.57 ms per config-2 step without its stores): ~390 VALU instructions per
// frame pair, of which the k-tap contraction is 28 % (measured: with ONE tap the kernel takes 0.41 ms, profiles/r05_conv0_*)
// and the two 64-lane LayerNorm reductions another 20 %.  Here
//   * the taps run as ONE v_mfma_f32_16x16x32_f16 per (16 channels x 16 frames): K = 32 holds the three split-precision terms of
//     the 10-tap product side by side -- A row (channel) [w_hi(10) | w_lo(10) | w_hi(10) | 0 0], B column (frame)
//     [x_hi(10) | x_hi(10) | x_lo(10) | 0 0] -- so hi.hi + lo.hi + hi.lo (2^-22 relative, fp32 accumulate) is a single MFMA on
//     a pipe that idles in this kernel.  Both operands are fp16 planes whatever the handle's mode: the samples of a frame are
//     scaled by an exact power of two (largest |x| of the frame into [512, 1024)) and the weights by one per tensor, so the lo
//     planes stay normal numbers and silence is as accurate as speech (LayerNorm makes the result scale-free per frame);
//   * the LayerNorm statistics need no pass over the channels: mean_c(w_c . x + b_c) = wbar . x + bbar and
//     var_c(...) = x~^T G x~ with x~ = [x; 1] and G the 11 x 11 covariance of the rows [w_c, b_c] over the channels -- exact
//     identities, evaluated per frame in fp64 from tables amx_create computes in fp64 (`stats`: 11 + 121 doubles), i.e. more
//     accurate than the fp32 two-pass sums they replace, and 132 FMAs per frame instead of 2 x 512 + two butterflies;
//   * a lane owns ONE frame and 4 consecutive channels per tile (MFMA output layout), so the normalisation is two packed FMAs
//     with lane-constant factors; outputs go through a per-wave LDS patch and leave as whole 128-byte lines.
// Workgroup = 128 frames (8 frame tiles) x 512 channels; wave w owns channels [128 w, 128 w + 128) with its weight fragments in
// registers; the frame operands (8 KiB), scales and statistics of the 128 frames are built once per workgroup.
// ----------------------------------------------------------------------------------------------------------------
constexpr int C0M_FRAMES = 128, C0M_K = 10, C0M_C = 512;
static_assert(CONV0_MFMA_STATS == 11 + 121, "stats table: mean of [w_c, b_c] over c (11 doubles), covariance G (11 x 11, row-major)");

template <int NT>
constexpr int c0m_rowb() { return (NT == 2 ? 512 : 256) + 16; }  // bytes of a staged frame row of one wave (+ 16: bank skew)
inline size_t conv0_mfma_lds_bytes(int NT, int stride) {
    const size_t win = ((size_t)(C0M_FRAMES * stride + C0M_K) * 4 + 15) & ~(size_t)15;
    const size_t stage = (size_t)4 * 16 * (NT == 2 ? c0m_rowb<2>() : c0m_rowb<1>());
    const size_t image = (size_t)C0M_C * 64;  // fp16 weight image [512][32], aliased with the staging patches
    return win + 4 * C0M_FRAMES * 4 + (size_t)C0M_FRAMES * 64 + (stage > image ? stage : image);
}

// GN (the group-norm feature extractor): `gamma` / `beta` are the per-(utterance, channel) scale and shift [N, C] of the GroupNorm
// over time (conv0_gn_cov_final_kernel), y = (conv + b) * scale + shift: no per-frame statistics, `stats` unused.
template <typename T, int NT, bool GN>
__global__ __launch_bounds__(256, 2) void conv0_mfma_kernel(const float* __restrict__ audio, const int64_t* __restrict__ lengths,
                                                            const float* __restrict__ mean_rstd, int64_t L, int T1, int stride,
                                                            const float* __restrict__ w /*[512][10]*/, const float* __restrict__ b,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const double* __restrict__ stats, float w_scale, float eps,
                                                            int do_normalize, T* __restrict__ out, int64_t out_plane,
                                                            int skip_padding) {
    typedef _Float16 h16;
    typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
    typedef typename Vec2<T>::type V2;
    constexpr int ROWB = c0m_rowb<NT>();
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n = blockIdx.y;
    const int f0 = blockIdx.x * C0M_FRAMES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwin = C0M_FRAMES * stride + C0M_K;
    const int64_t len = lengths[n];
    if (skip_padding && (int64_t)f0 * stride + C0M_K > len && f0 > 0) return;  // (see conv0_kernel)
    if (GN) { gamma += (int64_t)n * C0M_C; beta += (int64_t)n * C0M_C; }
    float* win = (float*)smem;
    const int win_bytes = (nwin * 4 + 15) & ~15;
    float* fr_a = (float*)(smem + win_bytes);          // per frame: acc -> conv value / sigma:  rstd / (2^s * w_scale)
    float* fr_c = fr_a + C0M_FRAMES;                    //            - mean * rstd
    float* fr_r = fr_c + C0M_FRAMES;                    //            rstd
    unsigned char* bplanes = (unsigned char*)(fr_r + 2 * C0M_FRAMES);  // [8 frame tiles][64 MFMA lanes][16 B]
    unsigned char* stage = bplanes + C0M_FRAMES * 64;   // per-wave output patches; first: the fp16 weight image [512][32]

    // ---- the window of this workgroup's frames, input normalisation applied on load ----
    const float mean = mean_rstd[2 * n], rstd_in = mean_rstd[2 * n + 1];
    const int64_t s0 = (int64_t)f0 * stride;
    for (int i = tid; i < nwin; i += 256) {
        const int64_t pos = s0 + i;
        float x = 0.f;
        if (pos < L) {
            x = audio[(int64_t)n * L + pos];
            if (do_normalize) x = pos < len ? (x - mean) * rstd_in : 0.f;
        }
        win[i] = x;
    }
    // ---- weight image: row c = [w_hi(10) | w_lo(10) | w_hi(10) | 0 0] of w_c * w_scale as fp16 (two channels per thread) ----
#pragma unroll
    for (int rep = 0; rep < 2; ++rep) {
        const int c = tid + 256 * rep;
        h16 hi[C0M_K], lo[C0M_K];
#pragma unroll
        for (int j = 0; j < C0M_K; ++j) {
            float v = w[c * C0M_K + j] * w_scale;
            asm volatile("" : "+v"(v));
            hi[j] = (h16)v;
            asm volatile("" : "+v"(hi[j]));
            lo[j] = (h16)(v - (float)hi[j]);
        }
        h16 row[32];
#pragma unroll
        for (int j = 0; j < C0M_K; ++j) { row[j] = hi[j]; row[10 + j] = lo[j]; row[20 + j] = hi[j]; }
        row[30] = (h16)0.f; row[31] = (h16)0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            h16x8 v8;
#pragma unroll
            for (int e = 0; e < 8; ++e) v8[e] = row[8 * q + e];
            *(h16x8*)(stage + c * 64 + q * 16) = v8;
        }
    }
    __syncthreads();
    // ---- per frame (threads 0..127): power-of-two scale, fp64 LayerNorm statistics, the frame's B column ----
    if (tid < C0M_FRAMES) {
        const int f = tid;
        float x[C0M_K];
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < C0M_K; ++j) { x[j] = win[f * stride + j]; amax = fmaxf(amax, fabsf(x[j])); }
        // exact power of two that puts the largest sample of the frame into [512, 1024) (1 for an all-zero / non-finite frame)
        int e = 0;
        if (amax > 0.f && amax < INFINITY) e = 9 - (((__builtin_bit_cast(int, amax) >> 23) & 255) - 127);
        e = e < -100 ? -100 : (e > 120 ? 120 : e);
        const float sc = __builtin_bit_cast(float, (127 + e) << 23), inv_sc = __builtin_bit_cast(float, (127 - e) << 23);
        if constexpr (GN) {
            fr_r[f] = 1.f;
            fr_c[f] = 0.f;
            fr_a[f] = inv_sc / w_scale;  // (both exact powers of two)
        } else {
            double xt[11];
#pragma unroll
            for (int j = 0; j < C0M_K; ++j) xt[j] = (double)x[j];
            xt[10] = 1.0;
            double mu = 0.0, var = 0.0;
#pragma unroll
            for (int a = 0; a < 11; ++a) {
                mu = fma(stats[a], xt[a], mu);
                double rowsum = 0.0;
#pragma unroll
                for (int c2 = 0; c2 < 11; ++c2) rowsum = fma(stats[11 + a * 11 + c2], xt[c2], rowsum);
                var = fma(rowsum, xt[a], var);
            }
            if (!(var > 0.0)) var = 0.0;
            const double rs = 1.0 / sqrt(var + (double)eps);
            fr_r[f] = (float)rs;
            fr_c[f] = (float)(-mu * rs);
            fr_a[f] = (float)(rs * (double)inv_sc / (double)w_scale);
        }
        h16 hi[C0M_K], lo[C0M_K];
#pragma unroll
        for (int j = 0; j < C0M_K; ++j) {
            float v = x[j] * sc;
            asm volatile("" : "+v"(v));
            hi[j] = (h16)v;
            asm volatile("" : "+v"(hi[j]));
            lo[j] = (h16)(v - (float)hi[j]);
        }
        h16 row[32];
#pragma unroll
        for (int j = 0; j < C0M_K; ++j) { row[j] = hi[j]; row[10 + j] = hi[j]; row[20 + j] = lo[j]; }
        row[30] = (h16)0.f; row[31] = (h16)0.f;
        const int ft = f >> 4, jj = f & 15;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // chunk q = the 8 K values MFMA lane (jj, group q) feeds
            h16x8 v8;
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) v8[e2] = row[8 * q + e2];
            *(h16x8*)(bplanes + ((ft * 4 + q) * 16 + jj) * 16) = v8;
        }
    }
    // ---- this wave's weight fragments (A operand: lane (i, g) = channel i of the tile, K 8g .. 8g + 7) and channel constants ----
    const int li = lane & 15, g = lane >> 4;
    h16x8 wf[8];
    f32x2 b2[8][2], g2[8][2], be2[8][2];
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
        wf[tt] = *(const h16x8*)(stage + ((wave * 8 + tt) * 16 + li) * 64 + g * 16);
        const int c = wave * 128 + tt * 16 + 4 * g;
        const float4 bb = *(const float4*)(b + c), gg = *(const float4*)(gamma + c), ee = *(const float4*)(beta + c);
        b2[tt][0] = f32x2{bb.x, bb.y}; b2[tt][1] = f32x2{bb.z, bb.w};
        g2[tt][0] = f32x2{gg.x, gg.y}; g2[tt][1] = f32x2{gg.z, gg.w};
        be2[tt][0] = f32x2{ee.x, ee.y}; be2[tt][1] = f32x2{ee.z, ee.w};
        if constexpr (GN) {  // (conv + b) * scale + shift = conv * scale + (b * scale + shift)
            be2[tt][0] = b2[tt][0] * g2[tt][0] + be2[tt][0];
            be2[tt][1] = b2[tt][1] * g2[tt][1] + be2[tt][1];
        }
    }
    __syncthreads();  // frame columns and statistics are complete; the weight image is dead (its LDS becomes the patches)
    unsigned char* patch = stage + wave * (16 * ROWB);
    const bool o_il = plane_is_il<NT>(out_plane);
    for (int ft = 0; ft < C0M_FRAMES / 16; ++ft) {
        if (f0 + ft * 16 >= T1) break;  // (wave-uniform) nothing of this tile exists
        const h16x8 xf = *(const h16x8*)(bplanes + (ft * 64 + lane) * 16);
        const int f = ft * 16 + li;
        const float a = fr_a[f], cc = fr_c[f], rr = fr_r[f];
        const f32x2 a2 = {a, a}, c2 = {cc, cc}, r2 = {rr, rr};
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[tt], xf, acc, 0, 0, 0);
            V2 hi[2], lo[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x2 v = {acc[2 * q], acc[2 * q + 1]};
                // LayerNorm((v * inv_scale + b) ; mu, rstd) * gamma + beta with the per-frame factors folded: a = rstd * inv_scale
                const f32x2 u = GN ? v * a2 : v * a2 + (b2[tt][q] * r2 + c2);
                const f32x2 y = gelu_fast2(u * g2[tt][q] + be2[tt][q]);
                lo[q] = V2{(T)0.f, (T)0.f};
                split16x2<T, NT>(y, hi[q], lo[q]);
            }
            // channels co .. co + 3 of the wave's 128: the frame row as it lies in HBM (interleaved planes: [hi x 32 | lo x 32])
            const int co = tt * 16 + 4 * g;
            unsigned char* dst = patch + li * ROWB + (NT == 2 ? (co >> 5) * 128 + (co & 31) * 2 : co * 2);
            union { V2 h[2]; uint64_t u; } ph, pl;
            ph.h[0] = hi[0]; ph.h[1] = hi[1];
            *(uint64_t*)dst = ph.u;
            if (NT == 2) {
                pl.h[0] = lo[0]; pl.h[1] = lo[1];
                *(uint64_t*)(dst + 64) = pl.u;
            }
        }
        // the wave's 16 x (128 channels) patch leaves as 16-byte pieces of whole lines (LDS operations of one wave complete in
        // order: these reads see the writes above, and the next tile's writes follow them)
        constexpr int CHUNKS_PER_ROW = (ROWB - 16) / 16, ROUNDS = 16 * CHUNKS_PER_ROW / 64;
#pragma unroll
        for (int q = 0; q < ROUNDS; ++q) {
            const int id = q * 64 + lane, row = id / CHUNKS_PER_ROW, chunk = id - row * CHUNKS_PER_ROW;
            const uint4 v = *(const uint4*)(patch + row * ROWB + chunk * 16);
            const int t = f0 + ft * 16 + row;
            if (t < T1) {
                T* base = out + pidx(((int64_t)n * T1 + t) * C0M_C + wave * 128, o_il);
                *(uint4*)((unsigned char*)base + chunk * 16) = v;
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------
// Group-norm feature extractor (transformers Wav2Vec2GroupNormConvLayer: conv -> GroupNorm(num_groups = C) -> GELU): the
// statistics of conv layer 0's raw output per (utterance, channel) over ALL T1 frames of the padded length -- upstream
// normalises the padded batch tensor, so frames of an utterance's padding count (their conv output is the bias).  The conv
// (k taps per output) is recomputed rather than stored: pass 1 here, pass 2 = conv0_kernel<GN>.  fp64 sums of the fp32 conv
// values, fixed order (block partials, then a serial combine): deterministic.
// ----------------------------------------------------------------------------------------------------------------
constexpr int GN_FRAMES = 1024;  // frames per workgroup of the statistics pass

template <int KW>
__global__ __launch_bounds__(256) void conv0_gn_stats_kernel(const float* __restrict__ audio, const int64_t* __restrict__ lengths,
                                                             const float* __restrict__ mean_rstd, int64_t L, int T1, int C, int k,
                                                             int stride, const float* __restrict__ w, const float* __restrict__ b,
                                                             int do_normalize, double* __restrict__ partial /*[N][blocks][C][2]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* win = (float*)smem;
    const int n = blockIdx.y, blk = blockIdx.x;
    const int f0 = blk * GN_FRAMES;
    const int frames = min(GN_FRAMES, T1 - f0);
    const int nwin = (frames - 1) * stride + k;
    const int64_t len = lengths[n];
    const float mean = mean_rstd[2 * n], rstd = mean_rstd[2 * n + 1];
    const int64_t s0 = (int64_t)f0 * stride;
    for (int i = threadIdx.x; i < nwin; i += 256) {
        const int64_t pos = s0 + i;
        float x = 0.f;
        if (pos < L) {
            x = audio[(int64_t)n * L + pos];
            if (do_normalize) x = pos < len ? (x - mean) * rstd : 0.f;
        }
        win[i] = x;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float wr[KW];
#pragma unroll
        for (int j = 0; j < KW; ++j) wr[j] = j < k ? w[c * k + j] : 0.f;
        const float bias = b[c];
        double s = 0.0, q = 0.0;
        for (int f = 0; f < frames; f += 8) {
            // eight frames in fp32, then one fp64 step: the fp32 partial sums stay short (8 terms)
            float s8 = 0.f, q8 = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (f + u < frames) {
                    float acc = bias;
#pragma unroll
                    for (int j = 0; j < KW; ++j) acc = fmaf(wr[j], j < k ? win[(f + u) * stride + j] : 0.f, acc);
                    s8 += acc;
                    q8 = fmaf(acc, acc, q8);
                }
            }
            s += (double)s8;
            q += (double)q8;
        }
        double* dst = partial + (((int64_t)n * gridDim.x + blk) * C + c) * 2;
        dst[0] = s;
        dst[1] = q;
    }
}

// The same statistics with the register blocking of conv0_kernel (C == 512, k == KW): a lane owns 8 consecutive channels with
// their taps in registers, a wave walks the frames of its block two at a time on the packed fp32 pipe (one LDS broadcast read
// per tap feeds 8 channels; the general kernel above reads LDS once per multiply), eight frames in fp32 between fp64 steps, and
// the four waves of the workgroup are summed through LDS in wave order.  0.60 -> 0.2 ms at 32 x 10 s.
template <int KW>
__global__ __launch_bounds__(256) void conv0_gn_stats8_kernel(const float* __restrict__ audio, const int64_t* __restrict__ lengths,
                                                              const float* __restrict__ mean_rstd, int64_t L, int T1, int C, int stride,
                                                              const float* __restrict__ w, const float* __restrict__ b, int do_normalize,
                                                              double* __restrict__ partial /*[N][blocks][C][2]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* win = (float*)smem;
    constexpr int CP = 4;  // channel pairs per lane
    const int n = blockIdx.y, blk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f0 = blk * GN_FRAMES;
    const int frames = min(GN_FRAMES, T1 - f0);
    const int nwin = (frames - 1) * stride + KW;
    const int64_t len = lengths[n];
    const float mean = mean_rstd[2 * n], rstd = mean_rstd[2 * n + 1];
    const int64_t s0 = (int64_t)f0 * stride;
    for (int i = threadIdx.x; i < nwin; i += 256) {
        const int64_t pos = s0 + i;
        float x = 0.f;
        if (pos < L) {
            x = audio[(int64_t)n * L + pos];
            if (do_normalize) x = pos < len ? (x - mean) * rstd : 0.f;
        }
        win[i] = x;
    }
    const int c0 = lane * 8;
    f32x2 w2[CP][KW], b2[CP];
#pragma unroll
    for (int i = 0; i < CP; ++i) {
#pragma unroll
        for (int j = 0; j < KW; ++j) w2[i][j] = f32x2{w[(c0 + 2 * i) * KW + j], w[(c0 + 2 * i + 1) * KW + j]};
        b2[i] = f32x2{b[c0 + 2 * i], b[c0 + 2 * i + 1]};
    }
    __syncthreads();
    double sd[2 * CP], qd[2 * CP];
#pragma unroll
    for (int i = 0; i < 2 * CP; ++i) { sd[i] = 0.0; qd[i] = 0.0; }
    // the wave's frames: wave, wave + 4, ... in groups of 8 (two at a time), fp32 inside a group
    for (int g = wave * 8; g < frames; g += 32) {
        f32x2 s8[CP], q8[CP];
#pragma unroll
        for (int i = 0; i < CP; ++i) { s8[i] = f32x2{0.f, 0.f}; q8[i] = f32x2{0.f, 0.f}; }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            f32x2 acc[2][CP];
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int i = 0; i < CP; ++i) acc[v][i] = b2[i];
#pragma unroll
            for (int j = 0; j < KW; ++j)
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const int f = g + u + v;
                    const float x = f < frames ? win[f * stride + j] : 0.f;
                    const f32x2 xx = {x, x};
#pragma unroll
                    for (int i = 0; i < CP; ++i) acc[v][i] = w2[i][j] * xx + acc[v][i];
                }
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                if (g + u + v < frames) {
#pragma unroll
                    for (int i = 0; i < CP; ++i) {
                        s8[i] += acc[v][i];
                        q8[i] = acc[v][i] * acc[v][i] + q8[i];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < CP; ++i) {
            sd[2 * i] += (double)s8[i][0]; sd[2 * i + 1] += (double)s8[i][1];
            qd[2 * i] += (double)q8[i][0]; qd[2 * i + 1] += (double)q8[i][1];
        }
    }
    // the four waves of the block, summed in wave order (the window is dead: its LDS holds the partials)
    __syncthreads();
    double* red = (double*)smem;  // [4 waves][512 channels][2]
#pragma unroll
    for (int i = 0; i < 2 * CP; ++i) {
        red[((size_t)wave * 512 + c0 + i) * 2] = sd[i];
        red[((size_t)wave * 512 + c0 + i) * 2 + 1] = qd[i];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) { s += red[((size_t)wv * 512 + c) * 2]; q += red[((size_t)wv * 512 + c) * 2 + 1]; }
        double* dst = partial + (((int64_t)n * gridDim.x + blk) * C + c) * 2;
        dst[0] = s;
        dst[1] = q;
    }
}

// mean / variance over the T1 frames -> scale = gamma * rstd, shift = beta - mean * scale per (utterance, channel)
__global__ void conv0_gn_final_kernel(const double* __restrict__ partial, int blocks, int N, int C, int T1,
                                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                      float* __restrict__ scale, float* __restrict__ shift) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * C) return;
    const int n = (int)(i / C), c = (int)(i - (int64_t)n * C);
    double s = 0.0, q = 0.0;
    for (int blk = 0; blk < blocks; ++blk) {
        const double* src = partial + (((int64_t)n * blocks + blk) * C + c) * 2;
        s += src[0];
        q += src[1];
    }
    const double mean = s / (double)T1;
    double var = q / (double)T1 - mean * mean;  // biased variance, like torch.nn.GroupNorm
    if (var < 0) var = 0;
    const double rs = 1.0 / sqrt(var + (double)eps);
    const double sc = (double)gamma[c] * rs;
    scale[i] = (float)sc;
    shift[i] = (float)((double)beta[c] - mean * sc);
}

// ----------------------------------------------------------------------------------------------------------------
// GroupNorm statistics without recomputing the convolution (round 5; k = 10, the conv0_mfma_kernel shapes).  The conv output of
// channel c at frame t is w_c . x_t + b_c with x_t the frame's 10 (normalised) samples, so over the T1 frames of the padded length
//   mean_t = w_c . xbar + b_c,    var_t = w_c^T Cov w_c,    xbar = mean_t x_t,  Cov = mean_t x_t x_t^T - xbar xbar^T  (10 x 10)
// -- one pass over the audio for 10 + 55 sums in fp64 (conv0_gn_cov_kernel), then 110 fp64 FMAs per (utterance, channel)
// (conv0_gn_cov_final_kernel) instead of a second evaluation of every conv output.  Deterministic: block partials in fixed
// order, tree reductions of fixed shape.
// ----------------------------------------------------------------------------------------------------------------
constexpr int GNC_FRAMES = 2048;   // frames per workgroup
constexpr int GNC_SUMS = 10 + 55;  // S1[j], S2[a <= b]

__global__ __launch_bounds__(256) void conv0_gn_cov_kernel(const float* __restrict__ audio, const int64_t* __restrict__ lengths,
                                                           const float* __restrict__ mean_rstd, int64_t L, int T1, int stride,
                                                           int do_normalize, double* __restrict__ partial /*[N][blocks][65]*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* win = (float*)smem;
    const int n = blockIdx.y, blk = blockIdx.x;
    const int f0 = blk * GNC_FRAMES;
    const int frames = min(GNC_FRAMES, T1 - f0);
    const int nwin = (frames - 1) * stride + C0M_K;
    const int64_t len = lengths[n];
    const float mean = mean_rstd[2 * n], rstd = mean_rstd[2 * n + 1];
    const int64_t s0 = (int64_t)f0 * stride;
    for (int i = threadIdx.x; i < nwin; i += 256) {
        const int64_t pos = s0 + i;
        float x = 0.f;
        if (pos < L) {
            x = audio[(int64_t)n * L + pos];
            if (do_normalize) x = pos < len ? (x - mean) * rstd : 0.f;
        }
        win[i] = x;
    }
    __syncthreads();
    double acc[GNC_SUMS];
#pragma unroll
    for (int i = 0; i < GNC_SUMS; ++i) acc[i] = 0.0;
    for (int f = threadIdx.x; f < frames; f += 256) {
        double x[C0M_K];
#pragma unroll
        for (int j = 0; j < C0M_K; ++j) x[j] = (double)win[f * stride + j];
        int p = C0M_K;
#pragma unroll
        for (int a = 0; a < C0M_K; ++a) {
            acc[a] += x[a];
#pragma unroll
            for (int b2 = a; b2 < C0M_K; ++b2) { acc[p] = fma(x[a], x[b2], acc[p]); ++p; }
        }
    }
    // wave totals (xor tree), then the four waves in order
#pragma unroll
    for (int i = 0; i < GNC_SUMS; ++i) {
        double v = acc[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        acc[i] = v;
    }
    __syncthreads();  // the window is dead: its LDS takes the wave totals
    double* red = (double*)smem;  // [4][65]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < GNC_SUMS; ++i) red[wave * GNC_SUMS + i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < GNC_SUMS) {
        const double v = ((red[threadIdx.x] + red[GNC_SUMS + threadIdx.x]) + red[2 * GNC_SUMS + threadIdx.x]) + red[3 * GNC_SUMS + threadIdx.x];
        partial[((int64_t)n * gridDim.x + blk) * GNC_SUMS + threadIdx.x] = v;
    }
}

// one workgroup of 512 threads per utterance: totals of the block partials -> xbar, Cov; thread c -> scale / shift of channel c
__global__ __launch_bounds__(512) void conv0_gn_cov_final_kernel(const double* __restrict__ partial, int blocks, int T1,
                                                                 const float* __restrict__ w /*[512][10]*/, const float* __restrict__ b,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                 float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ double tot[GNC_SUMS], xbar[C0M_K], cov[C0M_K][C0M_K];
    const int n = blockIdx.x, c = threadIdx.x;
    if (c < GNC_SUMS) {
        double v = 0.0;
        for (int blk = 0; blk < blocks; ++blk) v += partial[((int64_t)n * blocks + blk) * GNC_SUMS + c];
        tot[c] = v;
    }
    __syncthreads();
    if (c < C0M_K) xbar[c] = tot[c] / (double)T1;
    __syncthreads();
    if (c < C0M_K * C0M_K) {
        const int a = c / C0M_K, b2 = c % C0M_K, lo = a < b2 ? a : b2, hi = a < b2 ? b2 : a;
        // index of (lo, hi) in the upper-triangular order of conv0_gn_cov_kernel
        const int p = C0M_K + lo * C0M_K - lo * (lo - 1) / 2 + (hi - lo);
        cov[a][b2] = tot[p] / (double)T1 - xbar[a] * xbar[b2];
    }
    __syncthreads();
    double wr[C0M_K];
#pragma unroll
    for (int j = 0; j < C0M_K; ++j) wr[j] = (double)w[c * C0M_K + j];
    double mean = (double)b[c], var = 0.0;
#pragma unroll
    for (int a = 0; a < C0M_K; ++a) {
        mean = fma(wr[a], xbar[a], mean);
        double rowsum = 0.0;
#pragma unroll
        for (int b2 = 0; b2 < C0M_K; ++b2) rowsum = fma(cov[a][b2], wr[b2], rowsum);
        var = fma(rowsum, wr[a], var);
    }
    if (!(var > 0.0)) var = 0.0;  // biased variance, like torch.nn.GroupNorm
    const double rs = 1.0 / sqrt(var + (double)eps);
    const double sc = (double)gamma[c] * rs;
    scale[(int64_t)n * C0M_C + c] = (float)sc;
    shift[(int64_t)n * C0M_C + c] = (float)((double)beta[c] - mean * sc);
}

}  // namespace

void launch_audio_stats(const float* audio, const int64_t* lengths, int N, int64_t L, double* partial, float* mean_rstd,
                        int do_normalize, hipStream_t s) {
    if (do_normalize) hipLaunchKernelGGL(audio_stats_kernel, dim3(STAT_CHUNKS, N), dim3(256), 0, s, audio, lengths, L, partial);
    hipLaunchKernelGGL(audio_stats_final_kernel, dim3((N + 63) / 64), dim3(64), 0, s, partial, lengths, N, mean_rstd,
                       do_normalize);
}

// Every condition that decides which first-layer kernels run, in one place.  A form is taken only if its dynamic LDS -- the
// staged audio window of a workgroup plus what the kernel keeps beside it -- stays within the 64 KiB a kernel may ask for
// without raising its limit: a launch over it would fail and leave stale outputs.
Conv0Route conv0_route(int prec, bool il, int C, int k, int stride, bool group_norm) {
    constexpr size_t LDS_MAX = 64 * 1024;
    Conv0Route r{};
    r.prec = prec;
    r.group_norm = group_norm;
    if (C < 1 || k < 1 || k > 16 || stride < 1) {
        r.refusal = "first conv layer: kernel 1 .. 16, positive stride and width";
        return r;
    }
    // Matrix pipe: conv0_mfma_kernel is written for C = 512, k = 10 (every released wav2vec 2.0 / XLS-R shape).  Its LDS is
    // judged at two planes whatever the mode, so that the four modes of one model take the same form (stride <= 41).  In the
    // two-plane modes its output patches are images of interleaved rows, so the handle's planes must be interleaved.
    r.mfma = C == C0M_C && k == C0M_K && conv0_mfma_lds_bytes(2, stride) <= LDS_MAX && (prec_planes(prec) == 1 || il);
    // Group norm: the matrix-pipe apply goes with the covariance statistics (both use the k = 10 frame as a vector), whose
    // workgroup stages 2048 frames (stride <= 7); past that the shape takes the recomputed statistics AND the scalar apply.
    const size_t cov_lds = (size_t)((GNC_FRAMES - 1) * stride + C0M_K) * sizeof(float);
    if (group_norm && cov_lds > LDS_MAX) r.mfma = false;
    if (r.mfma) {
        r.apply_lds = conv0_mfma_lds_bytes(prec_planes(prec), stride);
        r.stats = group_norm ? CONV0_STATS_COVARIANCE : CONV0_STATS_TABLE;
        if (group_norm) {
            r.stats_lds = cov_lds;
            r.stats_frames = GNC_FRAMES;
            r.stats_block_bytes = GNC_SUMS * sizeof(double);
        }
        return r;
    }
    // Scalar apply: lane l of a wave owns channels [l * CPL, l * CPL + CPL), so a row is 64 * CPL channels wide (or narrower
    // than 64 with idle lanes at CPL = 1); CPL is instantiated for 1, 2, 4 and 8 only.  Taps: KW = 10 or, padded, 16.
    if (C >= 64 && C != 64 && C != 128 && C != 256 && C != 512) {
        r.refusal = "conv_dim must be below 64 or one of 64, 128, 256, 512 (the widths the first-layer kernel is built for)";
        return r;
    }
    r.cpl = C >= 64 ? C / 64 : 1;
    r.kw = k == 10 ? 10 : 16;
    r.apply_lds = (size_t)(C0_FRAMES * stride + k) * sizeof(float);
    if (group_norm) {
        // the conv is evaluated a second time for its statistics, 1024 frames per workgroup; the register-blocked form also
        // keeps the 4 x 512 x 2 fp64 partials of its waves in that LDS
        const bool blocked = C == 512 && k == 10;
        r.stats = blocked ? CONV0_STATS_RECOMPUTE8 : CONV0_STATS_RECOMPUTE;
        r.stats_lds = (size_t)((GN_FRAMES - 1) * stride + k) * sizeof(float);
        if (blocked) r.stats_lds = std::max(r.stats_lds, (size_t)4 * 512 * 2 * sizeof(double));
        r.stats_frames = GN_FRAMES;
        r.stats_block_bytes = (size_t)C * 2 * sizeof(double);
    }
    if (r.apply_lds > LDS_MAX || r.stats_lds > LDS_MAX)
        r.refusal = "first conv stride too large for the LDS window of the conv-0 kernels (stride <= 16 with the group-norm "
                    "extractor, <= 127 otherwise)";
    return r;
}

template <typename T, int NT, int KW, bool GN>
static void conv0_launch_scalar(const Conv0Route& r, const Conv0Args& a, const float* gamma, const float* beta, hipStream_t s) {
    const dim3 grid((a.T1 + C0_FRAMES - 1) / C0_FRAMES, a.N);
#define C0_GO(CPL)                                                                                                          \
    hipLaunchKernelGGL((conv0_kernel<T, NT, CPL, KW, GN>), grid, dim3(256), r.apply_lds, s, a.audio, a.lengths, a.mean_rstd, a.L, \
                       a.T1, a.C, a.k, a.stride, a.w, a.b, gamma, beta, a.eps, a.do_normalize, (T*)a.out, a.out_plane,      \
                       a.skip_padding)
    switch (r.cpl) {
        case 8: C0_GO(8); break;
        case 4: C0_GO(4); break;
        case 2: C0_GO(2); break;
        case 1: C0_GO(1); break;
    }
#undef C0_GO
}

template <typename T, int NT, bool GN>
static void conv0_launch_mfma(const Conv0Route& r, const Conv0Args& a, const float* gamma, const float* beta, hipStream_t s) {
    const dim3 grid((a.T1 + C0M_FRAMES - 1) / C0M_FRAMES, a.N);
    hipLaunchKernelGGL((conv0_mfma_kernel<T, NT, GN>), grid, dim3(256), r.apply_lds, s, a.audio, a.lengths, a.mean_rstd, a.L, a.T1,
                       a.stride, a.w, a.b, gamma, beta, GN ? nullptr : a.table, a.w_scale, a.eps, a.do_normalize, (T*)a.out,
                       a.out_plane, a.skip_padding);
}

// the apply pass; under group norm it takes the per-(utterance, channel) scale / shift in place of the norm's own gamma / beta
template <bool GN>
static void conv0_launch_apply(const Conv0Route& r, const Conv0Args& a, hipStream_t s) {
    const float *gamma = GN ? a.gn_scale : a.gamma, *beta = GN ? a.gn_shift : a.beta;
    if (r.mfma) {
        AMX_DISPATCH(r.prec, (conv0_launch_mfma<T16, NT, GN>(r, a, gamma, beta, s)));
    } else if (r.kw == 10) {
        AMX_DISPATCH(r.prec, (conv0_launch_scalar<T16, NT, 10, GN>(r, a, gamma, beta, s)));
    } else {
        AMX_DISPATCH(r.prec, (conv0_launch_scalar<T16, NT, 16, GN>(r, a, gamma, beta, s)));
    }
}

void launch_conv0(const Conv0Route& r, const Conv0Args& a, hipStream_t s) {
    // group norm: first the statistics over ALL T1 frames of the padded length, folded into scale / shift [N, C]
    const int blocks = r.stats_frames ? (a.T1 + r.stats_frames - 1) / r.stats_frames : 0;
    const dim3 sgrid(blocks, a.N);
    switch (r.stats) {
        case CONV0_STATS_NONE:
        case CONV0_STATS_TABLE: break;
        case CONV0_STATS_COVARIANCE:
            hipLaunchKernelGGL(conv0_gn_cov_kernel, sgrid, dim3(256), r.stats_lds, s, a.audio, a.lengths, a.mean_rstd, a.L, a.T1, a.stride,
                               a.do_normalize, a.gn_partial);
            hipLaunchKernelGGL(conv0_gn_cov_final_kernel, dim3(a.N), dim3(512), 0, s, a.gn_partial, blocks, a.T1, a.w, a.b, a.gamma, a.beta,
                               a.eps, a.gn_scale, a.gn_shift);
            break;
        case CONV0_STATS_RECOMPUTE8:
            hipLaunchKernelGGL(conv0_gn_stats8_kernel<10>, sgrid, dim3(256), r.stats_lds, s, a.audio, a.lengths, a.mean_rstd, a.L, a.T1, a.C,
                               a.stride, a.w, a.b, a.do_normalize, a.gn_partial);
            break;
        case CONV0_STATS_RECOMPUTE:
            if (r.kw == 10)
                hipLaunchKernelGGL(conv0_gn_stats_kernel<10>, sgrid, dim3(256), r.stats_lds, s, a.audio, a.lengths, a.mean_rstd, a.L, a.T1,
                                   a.C, a.k, a.stride, a.w, a.b, a.do_normalize, a.gn_partial);
            else
                hipLaunchKernelGGL(conv0_gn_stats_kernel<16>, sgrid, dim3(256), r.stats_lds, s, a.audio, a.lengths, a.mean_rstd, a.L, a.T1,
                                   a.C, a.k, a.stride, a.w, a.b, a.do_normalize, a.gn_partial);
            break;
    }
    if (r.stats == CONV0_STATS_RECOMPUTE8 || r.stats == CONV0_STATS_RECOMPUTE) {
        const int64_t nc = (int64_t)a.N * a.C;
        hipLaunchKernelGGL(conv0_gn_final_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, a.gn_partial, blocks, a.N, a.C, a.T1,
                           a.gamma, a.beta, a.eps, a.gn_scale, a.gn_shift);
    }
    if (r.group_norm) conv0_launch_apply<true>(r, a, s);
    else conv0_launch_apply<false>(r, a, s);
}

}  // namespace amx
