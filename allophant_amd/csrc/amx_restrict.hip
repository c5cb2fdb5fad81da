// Restriction of a union-inventory output to each utterance's own language; contract in include/allophant_amx_restrict.h.
//
// One WAVE per (t, n) row, four rows per workgroup; consecutive waves take consecutive utterances of one frame, which lie side
// by side in a [T, N, C] block.  Lane l owns the columns l, l + 64, ...: a strip of 64 columns is read and written as whole
// coalesced lines, and its membership is ONE 8-byte word, loaded wave-uniformly, of which the lane tests bit l.  Rows of up
// to RESIDENT strips (512 classes) are read once and kept in registers; wider rows are streamed three times (maximum, sum,
// write), the second and third reading from cache.  Either way a lane re-reads only columns that it alone writes, so `out`
// may be `src`.  The maximum and the sum are the DPP reductions of amx_common.h: no LDS, no barrier, no atomic, and the
// summation order depends on C alone.
#include "amx_common.h"
#include "../../include/allophant_amx_restrict.h"

#include <cmath>

namespace amx {

namespace {

constexpr int RW = 64;             // wave size, columns per strip
constexpr int RESTRICT_WAVES = 4;  // rows per workgroup
constexpr int RESIDENT = 8;        // strips a row may have to stay in registers

__device__ __forceinline__ bool is_member(uint64_t word, int lane) { return (word >> lane) & 1; }

// what a member becomes: `x - lse` (one fp32 subtraction; -inf where lse is -inf) or `x` itself
__device__ __forceinline__ float member_value(float x, float lse, bool normalize) {
    if (!normalize) return x;
    return lse == -INFINITY ? -INFINITY : x - lse;
}

__device__ __forceinline__ float log_sum_exp(float m, float s) { return m == -INFINITY ? -INFINITY : m + logf(s); }

// C <= RESIDENT * 64: the row in registers
__device__ __forceinline__ void restrict_row_resident(const float* src, float* out, const uint64_t* bits, int C, bool normalize, int lane) {
    float v[RESIDENT];
    bool member[RESIDENT];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < RESIDENT; ++k) {
        const int c = k * RW + lane;
        const uint64_t word = k * RW < C ? bits[k] : 0;  // (wave-uniform)
        member[k] = c < C && is_member(word, lane);
        v[k] = c < C ? src[c] : -INFINITY;
        if (!member[k]) v[k] = -INFINITY;
        m = fmaxf(m, v[k]);
    }
    m = wave_max(m);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < RESIDENT; ++k) s += member[k] ? expf(v[k] - m) : 0.0f;  // (a sum nobody reads where m is -inf)
    const float lse = log_sum_exp(m, wave_sum(s));
#pragma unroll
    for (int k = 0; k < RESIDENT; ++k) {
        const int c = k * RW + lane;
        if (c < C) out[c] = member[k] ? member_value(v[k], lse, normalize) : -INFINITY;
    }
}

// any C: three sweeps over the row
__device__ __forceinline__ void restrict_row_streamed(const float* src, float* out, const uint64_t* bits, int C, bool normalize, int lane) {
    float m = -INFINITY;
    for (int c = lane; c < C; c += RW)
        if (is_member(bits[c / RW], lane)) m = fmaxf(m, src[c]);
    m = wave_max(m);
    float s = 0.0f;
    for (int c = lane; c < C; c += RW)
        if (is_member(bits[c / RW], lane)) s += expf(src[c] - m);
    const float lse = log_sum_exp(m, wave_sum(s));
    for (int c = lane; c < C; c += RW) out[c] = is_member(bits[c / RW], lane) ? member_value(src[c], lse, normalize) : -INFINITY;
}

__global__ __launch_bounds__(RESTRICT_WAVES * RW) void restrict_kernel(RestrictArgs a) {
    const int lane = threadIdx.x & (RW - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / RW));
    const int64_t row = (int64_t)blockIdx.x * RESTRICT_WAVES + wave;  // t * N + n, wave-uniform
    if (row >= (int64_t)a.N * a.T) return;
    const int n = (int)(row % a.N);
    const int64_t t = row / a.N;
    const int len = a.frame_lengths[n], language = a.language_ids[n];
    if (language < 0 || language >= a.n_lang || len < 0 || len > a.T) {
        if (t == 0 && lane == 0) a.status[n] = -2;
        return;
    }
    if (t == 0 && lane == 0) a.status[n] = 0;
    float* out = a.out + t * a.out_stride_t + n * a.out_stride_n;
    if (t >= len) {
        for (int c = lane; c < a.C; c += RW) out[c] = 0.0f;
        return;
    }
    const float* src = a.src + t * a.stride_t + n * a.stride_n;
    const uint64_t* bits = a.member_bits + (int64_t)language * ((a.C + RW - 1) / RW);
    if (a.C <= RESIDENT * RW)
        restrict_row_resident(src, out, bits, a.C, a.normalize, lane);
    else
        restrict_row_streamed(src, out, bits, a.C, a.normalize, lane);
}

}  // namespace

void launch_restrict(RestrictArgs a, hipStream_t s) {
    const int64_t rows = (int64_t)a.N * a.T;
    hipLaunchKernelGGL(restrict_kernel, dim3((unsigned)((rows + RESTRICT_WAVES - 1) / RESTRICT_WAVES)), dim3(RESTRICT_WAVES * RW), 0, s, a);
}

}  // namespace amx
