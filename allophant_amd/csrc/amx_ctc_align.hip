// CTC forced alignment of known label sequences to frames (Viterbi); contract in include/allophant_amx_align.h.
//
// One workgroup per row.  The S = 2L + 1 states are cut into strips of 64; wave w of the block owns strips w, w + waves,
// ... (SPW of them at most, a template parameter so that everything a lane keeps per strip stays in registers), one state per
// lane.  The sweep is sequential in t: a lane keeps its own a[t-1][i] in a register and reads a[t-1][i-1] and a[t-1][i-2]
// from the previous frame's row, which is double-buffered in LDS (one barrier per frame).  A lane's label never changes, so
// it gathers lp[t][label] PF frames before the frame that adds it.  Each cell is one compare-and-select maximum and one
// fp32 addition, as the contract states them.
//
// The moves are recorded as two ballots per (frame, strip) -- (move == 1, move == 2) over the strip's 64 states -- staged
// one frame per lane and stored 64 frames at a time as 16-byte words at workspace[strip][frame] (with 8 strips per wave, i.e.
// past 2047 targets, the staging registers would spill, so there each word is stored as it is made).  Wave 0 then walks back
// from the end state: the walk is wave-uniform, loads the 64 words of the current (strip, 64 frames) at once and reads one
// per frame with readlane.  It stages one state per lane and writes paths, frame_scores and the span bounds 64 frames at a
// time; the bounds also go to LDS (the state rows are dead by then), from which one thread per target adds its frames' scores
// in frame order.
#include "amx_common.h"
#include "../../include/allophant_amx_align.h"

#include <cmath>

namespace amx {

namespace {

#include "amx_ctc_row.inc"

template <int SPW, int PF, bool STAGED>
__global__ __launch_bounds__(ALIGN_MAX_WAVES * CTC_WAVE) void ctc_align_kernel(AlignArgs a) {
    extern __shared__ float state_rows[];  // two rows of a.strips * 64 states; later the span bounds
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (CTC_WAVE - 1), wave = tid / CTC_WAVE, waves = blockDim.x / CTC_WAVE;
    const float neg_inf = -INFINITY;

    int64_t n = r, block = 0;  // utterance r of one tensor, or row o * N + n over the output blocks
    if (a.descs) n = (int)(r % a.N), block = r / a.N;
    CtcRow row;
    if (!ctc_open_row(a, r, n, block, row)) {
        if (tid == 0) a.status[r] = -2;
        return;
    }
    const float* lp = row.lp;
    const int64_t st = row.st;
    const int blank = row.blank, len = row.len, L = row.L;
    const int32_t* y = row.y;
    int32_t* paths = a.paths + r * a.T;
    if (len == 0) {
        if (L == 0)
            for (int t = tid; t < a.T; t += blockDim.x) paths[t] = -1;
        if (tid == 0) {
            if (L == 0) a.totals[r] = 0.0f;
            a.status[r] = L ? -1 : 0;
        }
        return;
    }

    const int S = 2 * L + 1;
    float* row0 = state_rows;
    float* row1 = state_rows + a.strips * CTC_WAVE;
    uint4* moves = a.workspace + r * a.strips * a.t_pad;

    bool live[SPW], skip[SPW];
    int lab[SPW];
    float x0[SPW], ahead[SPW][PF];
    uint4 word[STAGED ? SPW : 1];  // STAGED: lane c holds the strip's moves of frame 64 q + c until 64 frames are stored at once
#pragma unroll
    for (int k = 0; k < SPW; ++k) {
        const int strip = k * waves + wave, i = strip * CTC_WAVE + lane;
        live[k] = strip * CTC_WAVE < S;  // wave-uniform
        const bool mine = i < S;         // the lanes past S compute cells nobody reads
        lab[k] = blank, skip[k] = false, x0[k] = neg_inf;
        if (STAGED) word[k] = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < PF; ++j) ahead[k][j] = 0.0f;
        if (live[k]) {
            if (mine && (i & 1)) {
                lab[k] = y[i >> 1];
                skip[k] = i >= 3 && lab[k] != y[(i >> 1) - 1];
            }
            if (mine && i < 2) x0[k] = lp[lab[k]];
            row0[i] = x0[k];
#pragma unroll
            for (int j = 0; j < PF; ++j)
                if (1 + j < len) ahead[k][j] = lp[(1 + j) * st + lab[k]];
        }
    }
    __syncthreads();

    for (int t0 = 1; t0 < len; t0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = t0 + j;
            if (t < len) {
                const float* prev = (t & 1) ? row0 : row1;
                float* cur = (t & 1) ? row1 : row0;
                const int c = t & (CTC_WAVE - 1);
#pragma unroll
                for (int k = 0; k < SPW; ++k) {
                    if (live[k]) {
                        const int strip = k * waves + wave, i = strip * CTC_WAVE + lane;
                        const float x1 = i >= 1 ? prev[i - 1] : neg_inf;
                        const float x2 = skip[k] ? prev[i - 2] : neg_inf;
                        float best = x0[k];
                        int m = 0;
                        if (x1 > best) best = x1, m = 1;
                        if (x2 > best) best = x2, m = 2;
                        x0[k] = best + ahead[k][j];
                        cur[i] = x0[k];
                        if (t + PF < len) ahead[k][j] = lp[(int64_t)(t + PF) * st + lab[k]];
                        const unsigned long long b1 = __ballot(m == 1), b2 = __ballot(m == 2);
                        const uint4 both = make_uint4((uint32_t)b1, (uint32_t)(b1 >> 32), (uint32_t)b2, (uint32_t)(b2 >> 32));
                        if (STAGED) {
                            if (lane == c) word[k] = both;
                            if ((c == CTC_WAVE - 1 || t == len - 1) && lane <= c)
                                moves[strip * a.t_pad + (t - c) + lane] = word[k];
                        } else if (lane == c) {
                            moves[strip * a.t_pad + t] = both;
                        }
                    }
                }
                __syncthreads();  // the row is complete (and, after the last frame, the moves are visible to wave 0)
            }
        }
    }

    const float* last = ((len - 1) & 1) ? row1 : row0;
    const float end1 = last[S - 1], end2 = S > 1 ? last[S - 2] : neg_inf;
    int e = (S == 1 || end1 > end2) ? S - 1 : S - 2;
    const float total = e == S - 1 ? end1 : end2;
    if (total == neg_inf) {
        if (tid == 0) a.status[r] = -1;
        return;
    }
    __syncthreads();  // every wave has read the end states: the rows now hold the span bounds

    int* first = reinterpret_cast<int*>(state_rows);  // [L], then the ends [L]
    int* past = first + L;
    float* frame_scores = a.frame_scores + r * a.T;
    int32_t* spans = a.spans + r * a.max_target * 2;
    // an empty span for every target: on a NaN-ridden row the walk can stay on one state and visit none of the lower targets
    for (int l = tid; l < 2 * L; l += blockDim.x) first[l] = 0;
    __syncthreads();
    if (wave == 0) {
        int after_block = -1;  // the state of the frame after the 64 being walked
        for (int tb = (len - 1) & ~(CTC_WAVE - 1); tb >= 0; tb -= CTC_WAVE) {
            const int hi = min(len - 1, tb + CTC_WAVE - 1);
            int mine = -1, loaded = -1;
            uint4 w = make_uint4(0, 0, 0, 0);
            for (int t = hi; t >= tb; --t) {
                if (lane == t - tb) mine = e;
                if (t > 0) {
                    const int strip = e >> 6, bit = e & 63;
                    if (strip != loaded) {
                        w = moves[strip * a.t_pad + tb + lane];
                        loaded = strip;
                    }
                    const uint32_t m1 = __builtin_amdgcn_readlane(bit < 32 ? w.x : w.y, t - tb);
                    const uint32_t m2 = __builtin_amdgcn_readlane(bit < 32 ? w.z : w.w, t - tb);
                    e -= ((m1 >> (bit & 31)) & 1) + 2 * ((m2 >> (bit & 31)) & 1);
                    e = max(e, 0);  // (only NaN-ridden rows could get here)
                }
            }
            // frame tb + lane has state `mine`; e is now the state of frame tb - 1
            const int t = tb + lane;
            const int up = __shfl_up(mine, 1), down = __shfl_down(mine, 1);
            const int before = lane > 0 ? up : (tb > 0 ? e : -1);
            const int after = t < hi ? down : after_block;
            if (t <= hi) {
                const int label = (mine & 1) ? y[mine >> 1] : blank;
                paths[t] = label;
                frame_scores[t] = lp[(int64_t)t * st + label];
                if (mine & 1) {
                    const int l = mine >> 1;
                    if (before != mine) spans[2 * l] = t, first[l] = t;
                    if (after != mine) spans[2 * l + 1] = t + 1, past[l] = t + 1;
                }
            }
            after_block = __builtin_amdgcn_readfirstlane(mine);
        }
    }
    for (int t = len + tid; t < a.T; t += blockDim.x) paths[t] = -1;
    __syncthreads();

    for (int l = tid; l < L; l += blockDim.x) {
        const float* column = lp + y[l];
        float sum = 0.0f;
        for (int t = first[l]; t < past[l]; ++t) sum = sum + column[(int64_t)t * st];  // the values frame_scores holds
        a.span_scores[r * a.max_target + l] = sum;
    }
    if (tid == 0) {
        a.totals[r] = total;
        a.status[r] = 0;
    }
}

}  // namespace

bool ctc_align_workspace_bytes(int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    const size_t strips = (size_t)ctc_strips(max_target), t_pad = (size_t)((T + CTC_WAVE - 1) / CTC_WAVE * CTC_WAVE);
    size_t total = 0;
    if (__builtin_mul_overflow((size_t)rows, strips, &total) || __builtin_mul_overflow(total, t_pad, &total) ||
        __builtin_mul_overflow(total, sizeof(uint4), &total))
        return false;
    *bytes = total;
    return true;
}

void launch_ctc_align(AlignArgs a, hipStream_t s) {
    a.strips = (int)ctc_strips(a.max_target);
    a.t_pad = ((int64_t)a.T + CTC_WAVE - 1) / CTC_WAVE * CTC_WAVE;
    ctc_launch_rows(a, s, ctc_align_kernel<1, 4, true>, ctc_align_kernel<2, 4, true>, ctc_align_kernel<4, 2, true>,
                    ctc_align_kernel<8, 1, false>);
}

}  // namespace amx
