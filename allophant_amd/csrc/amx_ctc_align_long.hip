// CTC forced alignment of whole transcripts (up to AMX_ALIGN_LONG_MAX_TARGET targets per row): the contract of
// include/allophant_amx_align.h, cell for cell the recurrence of amx_ctc_align.hip, with the trellis cut so that a row's
// states are spread over the device and no workgroup ever waits for another.
//
//   prepare   one workgroup per row: validates the row once (ctc_open_row), reports refused rows (-2, or a row of no frames),
//             writes the row's live flag and frame 0's state row.
//   sweep     one launch per block of ALIGN_LONG_FRAMES = 64 frames, grid (state tiles, rows).  A tile owns ALIGN_LONG_OWNED
//             = 832 states (13 strips of 64, one strip per wave, one state per lane) and computes them together with a left
//             halo of ALIGN_LONG_HALO = 128 states, which it reads -- like its own -- from the state row the previous launch
//             left in the workspace.  A halo cell at the left edge lacks its predecessors and is wrong; the error moves right
//             by at most two states per frame, so after 64 frames it has reached the first owned state and not entered it.
//             (832 is no multiple of 128: a path that advances two states every frame from frame 0 crosses every other tile
//             edge in the middle of a frame block, where a halo too short loses it -- the tests' steepest row.)
//             Inside the launch the scheme is the old kernel's: the previous frame's row double-buffered in LDS, one barrier
//             per frame, emissions gathered PF frames ahead, the moves of (frame, strip) as two ballots staged one frame per
//             lane and stored as one coalesced line of 64 16-byte words -- for owned strips only.  The state row between
//             launches is ping-ponged by block parity: a neighbour reads its halo from the old row while the owner writes the
//             new one.  The only ordering between frame blocks is the stream's kernel boundary: no flags, no atomics, no
//             grid barrier.
//   finish    one workgroup per row: end state from the row's last state row, the wave-uniform walk of the old kernel
//             (wave 0), paths / frame_scores / spans, -1 past the length, then one thread per target adds its span's scores
//             in frame order.  The span bounds live in the workspace, preset to empty spans.
//
// The number of launches depends on the geometry only (2 + ceil(T / 64) per chunk of 65535 rows), so a call can be captured in
// a graph.
#include "amx_common.h"
#include "../../include/allophant_amx_align.h"

#include <algorithm>
#include <cmath>

namespace amx {

static_assert(ALIGN_LONG_FRAMES == CTC_WAVE, "one move word per lane makes a frame block one line");
static_assert(ALIGN_LONG_HALO == 2 * ALIGN_LONG_FRAMES, "the halo's error advances two states per frame");
static_assert(ALIGN_LONG_OWNED % CTC_WAVE == 0 && ALIGN_LONG_HALO % CTC_WAVE == 0, "tiles are whole strips");
static_assert(ALIGN_LONG_OWNED == AMX_ALIGN_LONG_TILE_STATES && ALIGN_LONG_FRAMES == AMX_ALIGN_LONG_FRAME_BLOCK, "header constants");

namespace {

#include "amx_ctc_row.inc"

constexpr int LONG_TILE = ALIGN_LONG_OWNED + ALIGN_LONG_HALO;  // states a tile computes = threads of a sweep workgroup
constexpr int LONG_THREADS = LONG_TILE;
constexpr int LONG_PF = 4;
static_assert(LONG_THREADS <= 1024, "one state per thread");

// Row r as ctc_open_row opens it, without the checks (the prepare launch made them: only live rows get here).
__device__ __forceinline__ CtcRow long_row(const AlignLongArgs& a, int64_t r) {
    CtcRow row;
    int64_t n = r;
    if (a.descs) {
        n = r % a.N;
        const OutDesc d = a.descs[r / a.N];
        row.lp = a.emissions + (int64_t)a.T * a.N * d.prefix + n * d.C;
        row.st = (int64_t)a.N * d.C, row.C = d.C, row.blank = 0;
    } else {
        row.lp = a.emissions + n * a.stride_n;
        row.st = a.stride_t, row.C = a.C, row.blank = a.blank;
    }
    row.len = a.frame_lengths[n];
    const int lb = a.target_offsets[r];
    row.L = a.target_offsets[r + 1] - lb;
    row.y = a.target_ids + lb;
    return row;
}

// state row `parity` of row r: strips * 64 floats
__device__ __forceinline__ float* long_states(const AlignLongArgs& a, int64_t r, int parity) {
    return a.states + (2 * r + parity) * ((int64_t)a.strips * CTC_WAVE);
}

__global__ __launch_bounds__(LONG_THREADS) void ctc_align_long_prepare(AlignLongArgs a) {
    const int64_t r = a.row_base + blockIdx.x;
    const int tid = threadIdx.x;
    int64_t n = r, block = 0;
    if (a.descs) n = (int)(r % a.N), block = r / a.N;
    CtcRow row;
    if (!ctc_open_row(a, r, n, block, row)) {
        if (tid == 0) a.status[r] = -2, a.live[r] = 0;
        return;
    }
    if (row.len == 0) {
        if (row.L == 0)
            for (int t = tid; t < a.T; t += blockDim.x) a.paths[r * a.T + t] = -1;
        if (tid == 0) {
            if (row.L == 0) a.totals[r] = 0.0f;
            a.status[r] = row.L ? -1 : 0;
            a.live[r] = 0;
        }
        return;
    }
    // frame 0, as the state row "before block 0" (parity 1); whole strips, so that every lane of a live strip reads a value
    const int S = 2 * row.L + 1, padded = (S + CTC_WAVE - 1) / CTC_WAVE * CTC_WAVE;
    float* first = long_states(a, r, 1);
    for (int i = tid; i < padded; i += blockDim.x) {
        float v = -INFINITY;
        if (i == 0) v = row.lp[row.blank];
        if (i == 1 && S > 1) v = row.lp[row.y[0]];
        first[i] = v;
    }
    if (tid == 0) a.live[r] = 1;
}

// Frames [64 b, 64 b + 64) of row blockIdx.y (frame 0 is the prepare launch's), states of tile blockIdx.x.
__global__ __launch_bounds__(LONG_THREADS) void ctc_align_long_sweep(AlignLongArgs a, int b) {
    __shared__ float row0[LONG_TILE], row1[LONG_TILE];
    const int64_t r = a.row_base + blockIdx.y;
    if (!a.live[r]) return;
    const CtcRow row = long_row(a, r);
    const int len = row.len, S = 2 * row.L + 1;
    const int t_block = b * ALIGN_LONG_FRAMES;
    const int own0 = blockIdx.x * ALIGN_LONG_OWNED;
    if (t_block >= len || own0 >= S) return;  // (block-uniform)

    const int tid = threadIdx.x, lane = tid & (CTC_WAVE - 1), wave = tid / CTC_WAVE;
    const float neg_inf = -INFINITY;
    const float* lp = row.lp;
    const int64_t st = row.st;
    const int li = tid, gi = own0 - ALIGN_LONG_HALO + li;  // state in the tile, state in the row
    const int strip0 = gi - lane;                           // the strip's first state (wave-uniform)
    const bool live = strip0 >= 0 && strip0 < S;            // tile 0 has no halo; strips past S compute nothing
    const bool owned = live && wave >= ALIGN_LONG_HALO / CTC_WAVE;
    const bool mine = live && gi < S;  // the lanes past S compute cells nobody reads
    const int t_first = max(1, t_block), t_last = min(len - 1, t_block + ALIGN_LONG_FRAMES - 1);

    int lab = row.blank;
    bool skip = false;
    if (mine && (gi & 1)) {
        lab = row.y[gi >> 1];
        skip = gi >= 3 && li >= 2 && lab != row.y[(gi >> 1) - 1];
    }
    const bool step = gi >= 1 && li >= 1;
    float x0 = live ? long_states(a, r, (b + 1) & 1)[gi] : neg_inf;
    float ahead[LONG_PF];
#pragma unroll
    for (int j = 0; j < LONG_PF; ++j) ahead[j] = (live && t_first + j <= t_last) ? lp[(int64_t)(t_first + j) * st + lab] : 0.0f;
    ((t_first & 1) ? row0 : row1)[li] = x0;
    uint4 word = make_uint4(0, 0, 0, 0);  // lane c holds the strip's moves of frame 64 b + c
    __syncthreads();

    for (int t0 = t_first; t0 <= t_last; t0 += LONG_PF) {
#pragma unroll
        for (int j = 0; j < LONG_PF; ++j) {
            const int t = t0 + j;
            if (t <= t_last) {
                const float* prev = (t & 1) ? row0 : row1;
                float* cur = (t & 1) ? row1 : row0;
                if (live) {
                    const float x1 = step ? prev[li - 1] : neg_inf;
                    const float x2 = skip ? prev[li - 2] : neg_inf;
                    float best = x0;
                    int m = 0;
                    if (x1 > best) best = x1, m = 1;
                    if (x2 > best) best = x2, m = 2;
                    x0 = best + ahead[j];
                    cur[li] = x0;
                    if (t + LONG_PF <= t_last) ahead[j] = lp[(int64_t)(t + LONG_PF) * st + lab];
                    const unsigned long long b1 = __ballot(m == 1), b2 = __ballot(m == 2);
                    if (lane == (t & (CTC_WAVE - 1)))
                        word = make_uint4((uint32_t)b1, (uint32_t)(b1 >> 32), (uint32_t)b2, (uint32_t)(b2 >> 32));
                }
                __syncthreads();
            }
        }
    }

    if (owned) {
        long_states(a, r, b & 1)[gi] = x0;
        if (lane <= t_last - t_block)  // (a block of no frames -- a row of one frame -- stores frame 0's empty word)
            a.workspace[((int64_t)r * a.strips + (strip0 >> 6)) * a.t_pad + t_block + lane] = word;
    }
}

__global__ __launch_bounds__(LONG_THREADS) void ctc_align_long_finish(AlignLongArgs a) {
    const int64_t r = a.row_base + blockIdx.x;
    if (!a.live[r]) return;
    const CtcRow row = long_row(a, r);
    const int tid = threadIdx.x, lane = tid & (CTC_WAVE - 1), wave = tid / CTC_WAVE;
    const float neg_inf = -INFINITY;
    const float* lp = row.lp;
    const int64_t st = row.st;
    const int blank = row.blank, len = row.len, L = row.L, S = 2 * L + 1;
    const int32_t* y = row.y;

    const float* last = long_states(a, r, ((len - 1) / ALIGN_LONG_FRAMES) & 1);
    const float end1 = last[S - 1], end2 = S > 1 ? last[S - 2] : neg_inf;
    int e = (S == 1 || end1 > end2) ? S - 1 : S - 2;
    const float total = e == S - 1 ? end1 : end2;
    if (total == neg_inf) {
        if (tid == 0) a.status[r] = -1;
        return;
    }

    int* first = a.bounds + r * a.max_target * 2;  // [L], then the ends [L]
    int* past = first + L;
    const uint4* moves = a.workspace + r * a.strips * a.t_pad;
    int32_t* paths = a.paths + r * a.T;
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
                        w = moves[(int64_t)strip * a.t_pad + tb + lane];
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
    } else {
        for (int t = len + tid - CTC_WAVE; t < a.T; t += blockDim.x - CTC_WAVE) paths[t] = -1;
    }
    __syncthreads();  // the bounds are visible to the block

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

constexpr size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

// moves | two state rows per row | span bounds | live flags, each section a multiple of 16 bytes
bool ctc_align_long_layout(int64_t rows, int64_t T, int64_t max_target, AlignLongLayout* out) {
    const size_t strips = (size_t)ctc_strips(max_target), t_pad = (size_t)((T + CTC_WAVE - 1) / CTC_WAVE * CTC_WAVE);
    size_t moves = 0, states = 0, bounds = 0, live = 0, total = 0;
    if (__builtin_mul_overflow((size_t)rows, strips, &moves) || __builtin_mul_overflow(moves, t_pad, &moves) ||
        __builtin_mul_overflow(moves, sizeof(uint4), &moves))
        return false;
    if (__builtin_mul_overflow((size_t)rows, strips, &states) ||
        __builtin_mul_overflow(states, (size_t)(2 * CTC_WAVE * sizeof(float)), &states))
        return false;
    if (__builtin_mul_overflow((size_t)rows, (size_t)max_target, &bounds) ||
        __builtin_mul_overflow(bounds, 2 * sizeof(int32_t), &bounds) || bounds > SIZE_MAX - 15)
        return false;
    bounds = round16(bounds);
    if (__builtin_mul_overflow((size_t)rows, sizeof(int32_t), &live) || live > SIZE_MAX - 15) return false;
    live = round16(live);
    if (__builtin_add_overflow(moves, states, &total) || __builtin_add_overflow(total, bounds, &total) ||
        __builtin_add_overflow(total, live, &total))
        return false;
    out->states = moves, out->bounds = moves + states, out->live = moves + states + bounds, out->bytes = total;
    return true;
}

void launch_ctc_align_long(AlignLongArgs a, hipStream_t s) {
    AlignLongLayout at;
    if (!ctc_align_long_layout(a.rows, a.T, a.max_target, &at)) return;  // (the caller has sized the workspace with it)
    char* base = reinterpret_cast<char*>(a.workspace);
    a.states = reinterpret_cast<float*>(base + at.states);
    a.bounds = reinterpret_cast<int32_t*>(base + at.bounds);
    a.live = reinterpret_cast<int32_t*>(base + at.live);
    a.strips = (int)ctc_strips(a.max_target);
    a.t_pad = ((int64_t)a.T + CTC_WAVE - 1) / CTC_WAVE * CTC_WAVE;
    const int64_t tiles = (2 * (int64_t)a.max_target + 1 + ALIGN_LONG_OWNED - 1) / ALIGN_LONG_OWNED;
    const int blocks = (int)(a.t_pad / ALIGN_LONG_FRAMES);
    // rows in chunks that fit a grid: 65535 in y, and below 2^32 threads in all
    const int64_t chunk = std::min<int64_t>(65535, ((int64_t)1 << 22) / tiles - 1);
    for (a.row_base = 0; a.row_base < a.rows; a.row_base += chunk) {
        const unsigned rows = (unsigned)std::min<int64_t>(chunk, a.rows - a.row_base);
        hipLaunchKernelGGL(ctc_align_long_prepare, dim3(rows), dim3(LONG_THREADS), 0, s, a);
        for (int b = 0; b < blocks; ++b)
            hipLaunchKernelGGL(ctc_align_long_sweep, dim3((unsigned)tiles, rows), dim3(LONG_THREADS), 0, s, a, b);
        hipLaunchKernelGGL(ctc_align_long_finish, dim3(rows), dim3(LONG_THREADS), 0, s, a);
    }
}

}  // namespace amx
