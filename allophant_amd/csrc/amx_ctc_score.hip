// CTC forward-backward scoring of known label sequences (the sum over every path); contract in
// include/allophant_amx_score.h.
//
// The shape is that of amx_ctc_align.hip: one workgroup per row, the S = 2L + 1 states cut into strips of 64, wave w of the
// block owning strips w, w + waves, ... (SPW of them at most, a template parameter so that everything a lane keeps per strip
// stays in registers), one state per lane.  Both sweeps are sequential in t: a lane keeps its own previous value in a
// register and reads its two neighbours from the previous frame's row, double-buffered in LDS (one barrier per frame), and it
// gathers lp[t][label] PF frames before the frame that adds it.  Each cell is a 3-way log-sum-exp on the hardware's base-2
// exp and log (__expf / __logf), chosen over the library forms by measurement of both time and error.
//
// Each sweep starts from a virtual frame that holds 0 in its one entry state and -inf elsewhere, which yields the
// contract's first row exactly (lse of {0} is 0, and 0 + e is e).  The forward sweep stores a[t][i] to the workspace, states
// contiguous, so a strip stores one 256-byte line per frame.  The backward sweep follows in the same workgroup: a lane
// reads back the forward values of its own state (written by itself, so program order makes them visible) PF frames ahead,
// forms g[t][i], writes it to `posteriors` when asked and, for an odd state, adds the three sums of its target to registers:
// one lane per target adding frame by frame, so there are no atomics and the result is the same on every run.
#include "amx_common.h"
#include "../../include/allophant_amx_score.h"

#include <cmath>

namespace amx {

namespace {

#include "amx_ctc_row.inc"

// log(exp(x0) + exp(x1) + exp(x2)); -inf when all three are (the maximum is replaced by 0, so nothing subtracts -inf from -inf)
__device__ __forceinline__ float lse3(float x0, float x1, float x2) {
    const float m = fmaxf(fmaxf(x0, x1), x2);
    const float shift = m == -INFINITY ? 0.0f : m;
    return shift + __logf(__expf(x0 - shift) + __expf(x1 - shift) + __expf(x2 - shift));
}

template <int SPW, int PF>
__global__ __launch_bounds__(ALIGN_MAX_WAVES * CTC_WAVE) void ctc_score_kernel(ScoreArgs a) {
    extern __shared__ float state_rows[];  // two rows of a.strips * 64 states
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (CTC_WAVE - 1), wave = tid / CTC_WAVE, waves = blockDim.x / CTC_WAVE;
    const float neg_inf = -INFINITY;

    CtcRow row;  // row (o * N + n) * G + g over the output blocks, or n * G + g over one tensor
    if (!ctc_open_row(a, r, (int)((r / a.candidates) % a.N), r / ((int64_t)a.N * a.candidates), row)) {
        if (tid == 0) a.status[r] = -2;
        return;
    }
    const float* lp = row.lp;
    const int64_t st = row.st;
    const int len = row.len, L = row.L;
    const int32_t* y = row.y;
    if (len == 0) {
        if (tid == 0) {
            a.log_likelihood[r] = L ? neg_inf : 0.0f;
            a.status[r] = L ? -1 : 0;
        }
        return;
    }

    const int S = 2 * L + 1, W = a.strips * CTC_WAVE;
    float* row0 = state_rows;
    float* row1 = state_rows + W;
    float* forward = a.workspace + r * a.T * W;  // a[t][i] at forward[t * W + i]

    bool live[SPW], mine[SPW], skip[SPW];
    int lab[SPW];
    float own[SPW], ahead[SPW][PF];
#pragma unroll
    for (int k = 0; k < SPW; ++k) {
        const int strip = k * waves + wave, i = strip * CTC_WAVE + lane;
        live[k] = strip * CTC_WAVE < S;  // wave-uniform
        mine[k] = i < S;                 // the lanes past S compute cells nobody reads
        lab[k] = row.blank, skip[k] = false, own[k] = i == 0 ? 0.0f : neg_inf;
#pragma unroll
        for (int j = 0; j < PF; ++j) ahead[k][j] = 0.0f;
        if (live[k]) {
            if (mine[k] && (i & 1)) {
                lab[k] = y[i >> 1];
                skip[k] = i >= 3 && lab[k] != y[(i >> 1) - 1];
            }
            row0[i] = own[k];  // the virtual frame before the first
#pragma unroll
            for (int j = 0; j < PF; ++j)
                if (j < len) ahead[k][j] = lp[j * st + lab[k]];
        }
    }
    __syncthreads();

    for (int t0 = 0; t0 < len; t0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = t0 + j;
            if (t < len) {
                const float* prev = (t & 1) ? row1 : row0;
                float* cur = (t & 1) ? row0 : row1;
#pragma unroll
                for (int k = 0; k < SPW; ++k) {
                    if (live[k]) {
                        const int i = (k * waves + wave) * CTC_WAVE + lane;
                        const float x1 = i >= 1 ? prev[i - 1] : neg_inf;
                        const float x2 = skip[k] ? prev[i - 2] : neg_inf;
                        own[k] = lse3(own[k], x1, x2) + ahead[k][j];
                        cur[i] = own[k];
                        forward[(int64_t)t * W + i] = own[k];
                        if (t + PF < len) ahead[k][j] = lp[(int64_t)(t + PF) * st + lab[k]];
                    }
                }
                __syncthreads();  // the row is complete
            }
        }
    }

    const float* last = (len & 1) ? row1 : row0;
    const float ll = lse3(last[S - 1], S > 1 ? last[S - 2] : neg_inf, neg_inf);
    if (ll == neg_inf) {
        if (tid == 0) {
            a.log_likelihood[r] = neg_inf;
            a.status[r] = -1;
        }
        return;
    }
    __syncthreads();  // every wave has read the end states: the rows now serve the backward sweep

    float* posteriors = a.posteriors ? a.posteriors + r * a.T * (2 * (int64_t)a.max_target + 1) : nullptr;
    const int P = 2 * a.max_target + 1;
    float before[SPW][PF];  // the lane's own forward values, read back PF frames ahead
    float occupancy[SPW], position[SPW], score[SPW];
#pragma unroll
    for (int k = 0; k < SPW; ++k) {
        const int i = (k * waves + wave) * CTC_WAVE + lane;
        own[k] = i == S - 1 ? 0.0f : neg_inf;
        occupancy[k] = position[k] = score[k] = 0.0f;
        // from here `skip` is the backward skip, to state i + 2
        skip[k] = live[k] && (i & 1) && i + 2 < S && y[(i >> 1) + 1] != lab[k];
#pragma unroll
        for (int j = 0; j < PF; ++j) ahead[k][j] = before[k][j] = 0.0f;
        if (live[k]) {
            row0[i] = own[k];  // the virtual frame after the last
#pragma unroll
            for (int j = 0; j < PF; ++j)
                if (len - 1 - j >= 0) {
                    ahead[k][j] = lp[(int64_t)(len - 1 - j) * st + lab[k]];
                    before[k][j] = forward[(int64_t)(len - 1 - j) * W + i];
                }
        }
    }
    __syncthreads();

    for (int u0 = 0; u0 < len; u0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int u = u0 + j, t = len - 1 - u;
            if (u < len) {
                const float* next = (u & 1) ? row1 : row0;
                float* cur = (u & 1) ? row0 : row1;
#pragma unroll
                for (int k = 0; k < SPW; ++k) {
                    if (live[k]) {
                        const int i = (k * waves + wave) * CTC_WAVE + lane;
                        const float x1 = i + 1 < S ? next[i + 1] : neg_inf;
                        const float x2 = skip[k] ? next[i + 2] : neg_inf;
                        const float e = ahead[k][j], av = before[k][j];
                        own[k] = lse3(own[k], x1, x2) + e;
                        cur[i] = own[k];
                        const float g = (av == neg_inf || own[k] == neg_inf) ? 0.0f : __expf(av + own[k] - e - ll);
                        if (mine[k]) {
                            if (posteriors) posteriors[(int64_t)t * P + i] = g;
                            if (i & 1) {
                                occupancy[k] = occupancy[k] + g;
                                position[k] = position[k] + (float)t * g;
                                score[k] = score[k] + (g != 0.0f ? g * e : 0.0f);
                            }
                        }
                        if (t - PF >= 0) {
                            ahead[k][j] = lp[(int64_t)(t - PF) * st + lab[k]];
                            before[k][j] = forward[(int64_t)(t - PF) * W + i];
                        }
                    }
                }
                __syncthreads();
            }
        }
    }

#pragma unroll
    for (int k = 0; k < SPW; ++k) {
        const int i = (k * waves + wave) * CTC_WAVE + lane;
        if (mine[k] && (i & 1)) {
            const int64_t at = r * a.max_target + (i >> 1);
            a.occupancy[at] = occupancy[k];
            a.position_sums[at] = position[k];
            a.score_sums[at] = score[k];
        }
    }
    if (tid == 0) {
        a.log_likelihood[r] = ll;
        a.status[r] = 0;
    }
}

}  // namespace

bool ctc_score_workspace_bytes(int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    const size_t states = (size_t)(ctc_strips(max_target) * CTC_WAVE);
    size_t total = 0;
    if (__builtin_mul_overflow((size_t)rows, (size_t)T, &total) || __builtin_mul_overflow(total, states, &total) ||
        __builtin_mul_overflow(total, sizeof(float), &total))
        return false;
    *bytes = total;
    return true;
}

void launch_ctc_score(ScoreArgs a, hipStream_t s) {
    a.strips = (int)ctc_strips(a.max_target);
    ctc_launch_rows(a, s, ctc_score_kernel<1, 4>, ctc_score_kernel<2, 4>, ctc_score_kernel<4, 2>, ctc_score_kernel<8, 1>);
}

}  // namespace amx
