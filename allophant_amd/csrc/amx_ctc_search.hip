// CTC search for short label sequences within utterances (start and end free); contract in include/allophant_amx_search.h.
//
// A pre-pass reduces every frame's C emissions to its maximum m[n][t] (one wave per frame, the DPP max reduction), which
// every query of the utterance reuses.  The search kernel gives one WAVE to one (utterance, query) row; the four waves of a
// workgroup hold four consecutive queries of one utterance, so they share lines of lp and m.  State i lives in lane i % 64 of
// strip i / 64; a lane keeps d, the start frame b and the label of each state it owns in registers.  The strip count K (1, 2,
// 4, 8) is a template parameter of the row's sweep and is chosen per row, wave-uniformly, from the row's own L: a long query
// in the launch does not lengthen the sweep of the short ones.  There is no LDS, no barrier and no atomic.
//
// Per frame the strips are updated from the highest down, so that the strip below still holds the previous frame: states
// i - 1 and i - 2 arrive by a DPP wave shift, and the lanes at a strip's lower edge take lanes 63 / 62 of the strip below
// with readlane.  Each cell is one compare-select chain, one fp32 subtraction (the emission against the frame's maximum) and
// one fp32 addition.  lp[t][label] is gathered PF frames ahead of its use; m is loaded 64 frames at a time, one per lane, and
// read per frame with readlane.  The end state's (d, b) is read wave-uniformly each frame: it updates the running best in
// scalars and, when the curves are wanted, is staged in lane t % 64 and stored 64 frames at a time.
#include "amx_common.h"
#include "../../include/allophant_amx_search.h"

#include <cmath>

namespace amx {

namespace {

constexpr int SW = CTC_WAVE;     // wave size, states per strip
constexpr int SEARCH_WAVES = 4;  // rows (consecutive queries of one utterance) per workgroup

// wave_shr:1 -- lane l receives lane l - 1's `v`, lane 0 receives `lane0`
__device__ __forceinline__ int shift_in(int lane0, int v) { return __builtin_amdgcn_update_dpp(lane0, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ float shift_in(float lane0, float v) {
    return __builtin_bit_cast(float, shift_in(__builtin_bit_cast(int, lane0), __builtin_bit_cast(int, v)));
}

__global__ __launch_bounds__(SEARCH_WAVES * SW) void ctc_search_frame_max_kernel(SearchArgs a) {
    const int lane = threadIdx.x & (SW - 1);
    const int64_t frame = (int64_t)blockIdx.x * SEARCH_WAVES + threadIdx.x / SW;  // wave-uniform
    if (frame >= (int64_t)a.N * a.T) return;
    const int n = (int)(frame / a.T), t = (int)(frame % a.T);
    const int len = a.frame_lengths[n];
    if (len > a.T || t >= len) return;  // (no row reads it)
    const float* lp = a.emissions + n * a.stride_n + t * a.stride_t;
    float v = -INFINITY;
    for (int c = lane; c < a.C; c += SW) v = fmaxf(v, lp[c]);
    v = wave_max(v);
    if (lane == 0) a.frame_max[frame] = v;
}

// One row on one wave: `lp` the utterance's emissions (lp[t * st + c]), `m` its frame maxima, `y` the L ids of the query
// (validated), 2L - 1 <= K * 64.
template <int K, int PF>
__device__ __forceinline__ void search_row(const SearchArgs& a, const float* lp, int64_t st, const float* m, int len, const int32_t* y,
                                           int L, int blank, int64_t row, int lane) {
    static_assert(SW % PF == 0, "a block of 64 frames holds whole prefetch groups");
    const float neg_inf = -INFINITY;
    const int S = 2 * L - 1;
    const int end_strip = (S - 1) / SW, end_lane = (S - 1) % SW;  // wave-uniform
    const bool curves = a.end_scores != nullptr;
    float* end_scores = curves ? a.end_scores + row * a.T : nullptr;
    int32_t* end_starts = curves ? a.end_starts + row * a.T : nullptr;

    int lab[K], b[K];
    bool skip[K];
    float d[K], ahead[K][PF];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = k * SW + lane;
        lab[k] = blank, skip[k] = false, d[k] = neg_inf, b[k] = -1;
        if (i < S && !(i & 1)) {  // (the lanes past S compute cells nobody reads)
            lab[k] = y[i >> 1];
            skip[k] = i >= 2 && lab[k] != y[(i >> 1) - 1];
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) ahead[k][j] = j < len ? lp[j * st + lab[k]] : 0.0f;
    }

    float best = neg_inf, frame_max = 0.0f, staged_score = neg_inf;
    int best_start = -1, best_end = -1, staged_start = -1;
    for (int t0 = 0; t0 < len; t0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = t0 + j;
            if (t < len) {
                const int c = t & (SW - 1);
                if (c == 0) frame_max = t + lane < len ? m[t + lane] : 0.0f;
                const float mt = lane_value(frame_max, c);
#pragma unroll
                for (int k = K - 1; k >= 0; --k) {  // downwards: strip k - 1 still holds frame t - 1
                    if (k > end_strip) continue;    // (wave-uniform: a strip past the row's states)
                    const float below1_d = k ? lane_value(d[k - 1], SW - 1) : neg_inf;
                    const float below2_d = k ? lane_value(d[k - 1], SW - 2) : neg_inf;
                    const int below1_b = k ? __builtin_amdgcn_readlane(b[k - 1], SW - 1) : -1;
                    const int below2_b = k ? __builtin_amdgcn_readlane(b[k - 1], SW - 2) : -1;
                    const float x1 = shift_in(below1_d, d[k]), x2 = shift_in(below2_d, x1);
                    const int s1 = shift_in(below1_b, b[k]), s2 = shift_in(below2_b, s1);
                    float r = d[k];
                    int s = b[k];
                    if (x1 > r) r = x1, s = s1;  // (state 0 receives -inf)
                    if (skip[k] && x2 > r) r = x2, s = s2;
                    if (k == 0 && lane == 0 && 0.0f > r) r = 0.0f, s = t;  // a fresh start
                    const float x = ahead[k][j];
                    const float e = x == neg_inf ? neg_inf : x - mt;
                    d[k] = r + e;
                    b[k] = s;
                    if (t + PF < len) ahead[k][j] = lp[(int64_t)(t + PF) * st + lab[k]];
                }
                float end_d = neg_inf;
                int end_b = -1;
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (k == end_strip) end_d = lane_value(d[k], end_lane), end_b = __builtin_amdgcn_readlane(b[k], end_lane);
                const bool reached = end_d > neg_inf;
                if (reached && end_d >= best) best = end_d, best_start = end_b, best_end = t + 1;
                if (curves) {
                    if (lane == c) staged_score = end_d, staged_start = reached ? end_b : -1;
                    if ((c == SW - 1 || t == len - 1) && lane <= c) {
                        end_scores[t - c + lane] = staged_score;
                        end_starts[t - c + lane] = staged_start;
                    }
                }
            }
        }
    }
    if (lane == 0) {
        if (best_end >= 0) {
            a.best_scores[row] = best;
            a.best_spans[2 * row] = best_start;
            a.best_spans[2 * row + 1] = best_end;
        }
        a.status[row] = best_end >= 0 ? 0 : -1;
    }
}

__global__ __launch_bounds__(SEARCH_WAVES * SW) void ctc_search_kernel(SearchArgs a) {
    const int lane = threadIdx.x & (SW - 1);
    const int groups = a.Q / SEARCH_WAVES + (a.Q % SEARCH_WAVES != 0);
    const int n = (int)(blockIdx.x / groups);
    const int q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % groups) * SEARCH_WAVES + (int)(threadIdx.x / SW));
    if (q >= a.Q) return;
    const int64_t row = (int64_t)n * a.Q + q;
    const int len = a.frame_lengths[n];
    const int lb = a.query_offsets[q], le = a.query_offsets[q + 1], id_count = a.query_offsets[a.Q];
    const bool malformed = len < 0 || len > a.T || lb < 0 || le <= lb || le > id_count || le - lb > a.max_query;
    const int L = __builtin_amdgcn_readfirstlane(malformed ? 0 : le - lb);
    const int32_t* y = a.query_ids + lb;
    bool wrong = false;
    for (int l = lane; l < L; l += SW) {
        const int v = y[l];
        wrong |= v < 0 || v >= a.C || v == a.blank;
    }
    if (malformed || __any(wrong)) {
        if (lane == 0) a.status[row] = -2;
        return;
    }
    const float* lp = a.emissions + n * a.stride_n;
    const float* m = a.frame_max + (int64_t)n * a.T;
    const int strips = (2 * L - 1 + SW - 1) / SW;
    if (strips <= 1)
        search_row<1, 8>(a, lp, a.stride_t, m, len, y, L, a.blank, row, lane);
    else if (strips <= 2)
        search_row<2, 8>(a, lp, a.stride_t, m, len, y, L, a.blank, row, lane);
    else if (strips <= 4)
        search_row<4, 4>(a, lp, a.stride_t, m, len, y, L, a.blank, row, lane);
    else
        search_row<8, 2>(a, lp, a.stride_t, m, len, y, L, a.blank, row, lane);
}

}  // namespace

bool ctc_search_workspace_bytes(int64_t N, int64_t T, size_t* bytes) {
    size_t total = 0;
    if (__builtin_mul_overflow((size_t)N, (size_t)T, &total) || __builtin_mul_overflow(total, sizeof(float), &total)) return false;
    *bytes = total;
    return true;
}

void launch_ctc_search(SearchArgs a, hipStream_t s) {
    const int64_t frames = (int64_t)a.N * a.T;
    if (frames > 0)
        hipLaunchKernelGGL(ctc_search_frame_max_kernel, dim3((unsigned)((frames + SEARCH_WAVES - 1) / SEARCH_WAVES)),
                           dim3(SEARCH_WAVES * SW), 0, s, a);
    const int64_t groups = ((int64_t)a.Q + SEARCH_WAVES - 1) / SEARCH_WAVES;
    hipLaunchKernelGGL(ctc_search_kernel, dim3((unsigned)(a.N * groups)), dim3(SEARCH_WAVES * SW), 0, s, a);
}

}  // namespace amx
