// Language-specific phoneme outputs through the allophone layer: `AllophoneMapping.map_allophones` (reference
// network/acoustic_model.py:142-159 with _multiply_allophone_matrix :76-87) as one sparse gather-max pass.
//
//   out[t, n, q] = max_p( masked(x[t, n, p] * W[l, p, q]) ),   l = language_ids[n]
//
// Upstream builds the dense [T, P+1, Q+1] product per utterance, fills the masked positions with finfo(float32).min AFTER
// the multiply and max-reduces over p.  Here each (language, q) column keeps only its unmasked entries (p, W[l, p, q]) and
// starts its accumulator at finfo.min when the column has any masked entry (those entries would all contribute exactly
// that value), else at -inf (the identity of the max).  Every product is one fp32 multiply of the same operands as
// upstream's, and the max propagates NaN like torch.max, so each output value is bitwise the reference's.  No atomics, one
// launch for the batch.
#include "amx_common.h"

namespace amx {

namespace {

constexpr int AL_THREADS = 256;
constexpr int AL_FRAMES = 8;  // frames a workgroup stages at most (accumulators per lane)
constexpr int64_t AL_LDS_TARGET = 32 * 1024;

// torch.max semantics: NaN wins, otherwise the larger value.  fmaxf would drop the NaN.
__device__ __forceinline__ float nan_max(float acc, float v) { return (v > acc || v != v) ? v : acc; }

// grid (ceil(T / frames), N): one workgroup = one utterance (so one language) and `frames` consecutive frames of it.
// LDS holds those frames' phone rows (frames x P1 floats) because the gather by p is random; lanes own output columns q,
// so every store of a frame is one contiguous run of Q1 floats.
__global__ void __launch_bounds__(AL_THREADS) allophone_map_kernel(
    const float* __restrict__ phone, int64_t stride_t, int64_t stride_n, const int* __restrict__ language_ids, int n_lang,
    int N, int64_t T, int P1, int Q1, int frames, const int* __restrict__ col_ptr, const int* __restrict__ ent_p,
    const float* __restrict__ ent_w, const float* __restrict__ col_init, float* __restrict__ out) {
    extern __shared__ float xs[];  // [frames][P1]
    const int n = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * frames;
    const int nf = (int)min((int64_t)frames, T - t0);
    const int tid = threadIdx.x;
    const int l = language_ids[n];

    const float* src = phone + (int64_t)n * stride_n + t0 * stride_t;
    const int staged = nf * P1;
    for (int i = tid; i < staged; i += AL_THREADS) {
        const int f = i / P1;
        const int p = i - f * P1;
        xs[i] = src[(int64_t)f * stride_t + p];
    }
    __syncthreads();

    float* dst = out + (t0 * N + n) * (int64_t)Q1;
    const int64_t frame_stride = (int64_t)N * Q1;
    if (l < 0 || l >= n_lang) {  // outside the ABI contract (the binding normalises and checks the ids): mark, do not read
        for (int q = tid; q < Q1; q += AL_THREADS)
            for (int f = 0; f < nf; ++f) dst[f * frame_stride + q] = __builtin_nanf("");
        return;
    }
    const int* cp = col_ptr + (int64_t)l * Q1;
    const float* ci = col_init + (int64_t)l * Q1;
    for (int q = tid; q < Q1; q += AL_THREADS) {
        const float init = ci[q];
        float acc[AL_FRAMES];
#pragma unroll
        for (int f = 0; f < AL_FRAMES; ++f) acc[f] = init;
        const int e1 = cp[q + 1];
        for (int e = cp[q]; e < e1; ++e) {
            const int p = ent_p[e];
            const float w = ent_w[e];
#pragma unroll
            for (int f = 0; f < AL_FRAMES; ++f)
                if (f < nf) acc[f] = nan_max(acc[f], __fmul_rn(xs[f * P1 + p], w));
        }
#pragma unroll
        for (int f = 0; f < AL_FRAMES; ++f)
            if (f < nf) dst[f * frame_stride + q] = acc[f];
    }
}

}  // namespace

int allophone_frames(int P1) {
    // ~32 KB of LDS per workgroup keeps four to five of them resident per CU; one frame at the widest inventories
    int f = (int)(AL_LDS_TARGET / ((int64_t)P1 * (int64_t)sizeof(float)));
    return f < 1 ? 1 : (f > AL_FRAMES ? AL_FRAMES : f);
}

void launch_allophone_map(const float* phone, int64_t stride_t, int64_t stride_n, const int* language_ids, int n_lang, int N,
                          int64_t T, int P1, int Q1, const int* col_ptr, const int* ent_p, const float* ent_w,
                          const float* col_init, float* out, hipStream_t s) {
    const int frames = allophone_frames(P1);
    const size_t lds = (size_t)frames * P1 * sizeof(float);
    dim3 grid((unsigned)((T + frames - 1) / frames), (unsigned)N);
    hipLaunchKernelGGL(allophone_map_kernel, grid, dim3(AL_THREADS), lds, s, phone, stride_t, stride_n, language_ids, n_lang, N,
                       T, P1, Q1, frames, col_ptr, ent_p, ent_w, col_init, out);
}

}  // namespace amx
