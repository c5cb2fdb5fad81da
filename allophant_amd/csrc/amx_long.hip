// Long recordings as windows of utterance size: the plan (host), the gather of the windows' audio into one padded batch and
// the stitch of the windows' kept output frames into the recordings' outputs; contract in include/allophant_amx_long.h.
//
// Both kernels are copies bound by HBM: no LDS, no atomics, a workgroup of 256 lanes per work item, the grid capped and
// strided over the items.  A gather item is GATHER_CHUNK consecutive samples of one row of the batch.  A stitch item is
// STITCH_CHUNK consecutive units of the flattened (frame, class) range that one window keeps of one block, a unit being 4
// floats where the block allows 16-byte moves and 1 float otherwise: lanes run over classes AND frames, so that a block of 3
// classes coalesces like one of 641.  A lane divides once per item and then steps (frame, class) by the remainder.
#include "amx_common.h"
#include "../../include/allophant_amx_long.h"

#include <algorithm>

namespace amx {

namespace {

constexpr int LT = 256;                 // lanes per workgroup
constexpr int GATHER_CHUNK = LT * 4 * 2;  // samples per gather item: two 16-byte moves per lane
constexpr int STITCH_STEPS = 8;         // moves per lane and stitch item
constexpr int STITCH_CHUNK = LT * STITCH_STEPS;
constexpr int64_t MAX_GRID = 4096;      // workgroups per launch; the rest is strided

struct GatherArgs {
    const float* audio;
    const int64_t* lengths;
    const amx_long_window* windows;
    float* batch;
    int32_t* status;
    int64_t stride, hop, L_out, chunks;  // chunks: items per row, at least 1 (the status of a row of no samples)
    int R, n;
};

template <bool VEC>
__global__ __launch_bounds__(LT) void long_gather_kernel(GatherArgs a) {
    const int64_t items = (int64_t)a.n * a.chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int w = (int)(item / a.chunks);
        const int64_t s0 = (item % a.chunks) * GATHER_CHUNK;
        const amx_long_window win = a.windows[w];
        bool ok = win.recording >= 0 && win.recording < a.R && win.start >= 0 && win.samples >= 0 && win.samples <= a.L_out;
        int64_t first = 0;
        if (ok) {
            first = (int64_t)win.start * a.hop;  // (below 2^62: hop < 2^31)
            ok = first + win.samples <= a.lengths[win.recording];
        }
        if (s0 == 0 && threadIdx.x == 0) a.status[w] = ok ? 0 : -2;
        const int64_t samples = ok ? win.samples : 0;  // a malformed row reads nothing
        const float* __restrict__ src = ok ? a.audio + (int64_t)win.recording * a.stride + first : a.audio;
        float* __restrict__ dst = a.batch + (int64_t)w * a.L_out;
        const int64_t end = min(s0 + GATHER_CHUNK, a.L_out);
        if (VEC) {  // L_out is a multiple of 4: a move never passes `end`
            for (int64_t s = s0 + threadIdx.x * 4; s < end; s += LT * 4) {
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (s + 4 <= samples) {
                    v = *(const f32x4*)(src + s);
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (s + j < samples) v[j] = src[s + j];
                }
                *(f32x4*)(dst + s) = v;
            }
        } else {
            for (int64_t s = s0 + threadIdx.x; s < end; s += LT) dst[s] = s < samples ? src[s] : 0.0f;
        }
    }
}

struct StitchArgs {
    const float* src;
    float* dst;
    const amx_long_window* windows;
    int32_t* status;
    int64_t src_T, dst_T;
    int n, R;
    int base_aligned;  // src and dst both 16-byte aligned
    amx_long_block blocks[AMX_LONG_MAX_BLOCKS];
};

// units per frame of a block and whether a unit is 4 floats
__host__ __device__ inline bool stitch_vec(const amx_long_block& b, int base_aligned) {
    return base_aligned && !(((int64_t)b.classes | b.src_offset | b.dst_offset) & 3);
}
// items per window of a block: an upper bound, a window keeps at most src_T frames (src_T * classes < 2^31)
__host__ __device__ inline uint32_t stitch_chunks(int64_t src_T, uint32_t units) {
    return (uint32_t)((src_T * units + STITCH_CHUNK - 1) / STITCH_CHUNK);
}

__global__ __launch_bounds__(LT) void long_stitch_kernel(StitchArgs a) {
    const amx_long_block blk = a.blocks[blockIdx.y];
    const bool vec = stitch_vec(blk, a.base_aligned);
    const uint32_t units = vec ? blk.classes / 4 : blk.classes;  // per frame
    const uint32_t chunks = stitch_chunks(a.src_T, units);
    const uint32_t step_f = LT / units, step_c = LT % units;
    const int64_t src_frame = (int64_t)a.n * blk.classes, dst_frame = (int64_t)a.R * blk.classes;  // frame strides in floats
    const int64_t items = (int64_t)a.n * chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int w = (int)(item / chunks);
        const uint32_t u0 = (uint32_t)(item % chunks) * STITCH_CHUNK;
        const amx_long_window win = a.windows[w];
        const bool ok = win.recording >= 0 && win.recording < a.R && win.keep_lo >= 0 && win.keep_lo <= win.keep_hi &&
                        win.keep_lo >= win.start && win.keep_hi <= win.start + a.src_T && win.keep_hi <= a.dst_T;
        if (blockIdx.y == 0 && u0 == 0 && threadIdx.x == 0) a.status[w] = ok ? 0 : -2;
        if (!ok) continue;
        const uint32_t total = (uint32_t)(win.keep_hi - win.keep_lo) * units;  // (at most src_T * classes)
        const float* __restrict__ src = a.src + blk.src_offset + ((int64_t)(win.keep_lo - win.start) * a.n + w) * blk.classes;
        float* __restrict__ dst = a.dst + blk.dst_offset + ((int64_t)win.keep_lo * a.R + win.recording) * blk.classes;
        uint32_t u = u0 + threadIdx.x;
        uint32_t f = u / units, c = u % units;
#pragma unroll
        for (int k = 0; k < STITCH_STEPS; ++k, u += LT) {
            if (u < total) {
                if (vec)
                    *(f32x4*)(dst + f * dst_frame + c * 4) = *(const f32x4*)(src + f * src_frame + c * 4);
                else
                    dst[f * dst_frame + c] = src[f * src_frame + c];
            }
            f += step_f, c += step_c;
            if (c >= units) c -= units, ++f;
        }
    }
}

}  // namespace

void launch_long_gather(const float* audio, int64_t stride, const int64_t* lengths, int R, const amx_long_window* windows, int n,
                        int64_t hop, int64_t L_out, float* batch, int32_t* status, hipStream_t s) {
    GatherArgs a{};
    a.audio = audio, a.lengths = lengths, a.windows = windows, a.batch = batch, a.status = status;
    a.stride = stride, a.hop = hop, a.L_out = L_out, a.R = R, a.n = n;
    a.chunks = std::max<int64_t>(1, (L_out + GATHER_CHUNK - 1) / GATHER_CHUNK);
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)n * a.chunks, MAX_GRID));
    const bool vec = !((((uintptr_t)audio | (uintptr_t)batch) & 15) || ((stride | L_out | hop) & 3));
    if (vec)
        hipLaunchKernelGGL(long_gather_kernel<true>, grid, dim3(LT), 0, s, a);
    else
        hipLaunchKernelGGL(long_gather_kernel<false>, grid, dim3(LT), 0, s, a);
}

void launch_long_stitch(const float* src, int64_t src_T, int n, const amx_long_window* windows, const amx_long_block* blocks,
                        int n_blocks, float* dst, int R, int64_t dst_T, int32_t* status, hipStream_t s) {
    StitchArgs a{};
    a.src = src, a.dst = dst, a.windows = windows, a.status = status;
    a.src_T = src_T, a.dst_T = dst_T, a.n = n, a.R = R;
    a.base_aligned = !(((uintptr_t)src | (uintptr_t)dst) & 15);
    int64_t most = 1;  // items of the largest block
    for (int b = 0; b < n_blocks; ++b) {
        a.blocks[b] = blocks[b];
        const uint32_t units = stitch_vec(blocks[b], a.base_aligned) ? blocks[b].classes / 4 : blocks[b].classes;
        most = std::max(most, (int64_t)n * stitch_chunks(src_T, units));
    }
    const dim3 grid((unsigned)std::min(most, std::max<int64_t>(1, MAX_GRID / n_blocks)), (unsigned)n_blocks);
    hipLaunchKernelGGL(long_stitch_kernel, grid, dim3(LT), 0, s, a);
}

// -- the plan (host) -------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t FRAME_LIMIT = (int64_t)1 << 31;

int64_t long_frames(int64_t L, int64_t RF, int64_t S) { return L < RF ? 0 : (L - RF) / S + 1; }
}  // namespace

std::string long_plan(const int64_t* lengths, int R, int64_t window, int32_t context, const int32_t* conv_kernel,
                      const int32_t* conv_stride, int n_conv, amx_long_window* windows, int64_t capacity, int64_t* n_windows,
                      int64_t* frames) {
    if (!n_windows) return "null n_windows pointer";
    *n_windows = 0;
    if (n_conv < 1 || n_conv > AMX_MAX_CONV) return "n_conv must be 1 to " + std::to_string(AMX_MAX_CONV);
    if (!conv_kernel || !conv_stride) return "null conv geometry";
    if (R < 0 || (R > 0 && !lengths)) return R < 0 ? "negative number of recordings" : "null lengths";
    int64_t S = 1, RF = 1;
    for (int i = 0; i < n_conv; ++i) {
        if (conv_kernel[i] < 1 || conv_stride[i] < 1) return "conv kernels and strides must be at least 1";
        int64_t reach = 0;
        if (__builtin_mul_overflow((int64_t)conv_kernel[i] - 1, S, &reach) || __builtin_add_overflow(RF, reach, &RF) ||
            __builtin_mul_overflow(S, (int64_t)conv_stride[i], &S))
            return "conv stack too large";
    }
    if (context < 0) return "context must be at least 0 frames, got " + std::to_string(context);
    if (window < RF)
        return "a window of " + std::to_string(window) + " samples is shorter than the receptive field of the feature extractor (" +
               std::to_string(RF) + ")";
    if (window >= FRAME_LIMIT) return "a window must hold fewer than 2^31 samples";  // (and so fewer frames)
    const int64_t Wf = long_frames(window, RF, S);
    const int64_t K = Wf - 2 * (int64_t)context;
    if (K < 1)
        return "a window of " + std::to_string(Wf) + " frames keeps none with " + std::to_string(context) + " frames of context on each side";
    for (int r = 0; r < R; ++r) {
        if (lengths[r] < 0) return "negative length";
        if (long_frames(lengths[r], RF, S) >= FRAME_LIMIT) return "a recording must hold fewer than 2^31 frames";
    }
    int64_t total = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t T = long_frames(lengths[r], RF, S);
        if (frames) frames[r] = T;
        total += T == 0 ? 0 : T <= Wf ? 1 : (T - Wf + K - 1) / K + 1;
    }
    *n_windows = total;
    if (!windows) return "";
    if (capacity < total) return "room for " + std::to_string(capacity) + " windows, the plan has " + std::to_string(total);
    for (int r = 0; r < R; ++r) {
        const int64_t T = long_frames(lengths[r], RF, S);
        const int64_t n = T == 0 ? 0 : T <= Wf ? 1 : (T - Wf + K - 1) / K + 1;
        for (int64_t i = 0; i < n; ++i) {
            const int64_t start = std::min(i * K, std::max<int64_t>(0, T - Wf));
            amx_long_window& w = *windows++;
            w.recording = r, w.index = (int32_t)i, w.start = (int32_t)start;
            w.keep_lo = (int32_t)(i == 0 ? 0 : i * K + context);
            w.keep_hi = (int32_t)(i == n - 1 ? T : (i + 1) * K + context);
            w.samples = (int32_t)std::min(window, lengths[r] - start * S);
        }
    }
    return "";
}

}  // namespace amx
