// CTC scoring of every one-edit variant of a transcript (each substitution, deletion and insertion); contract in
// include/allophant_amx_variants.h.
//
// Two launches.  The lattice kernel is the forward and backward sweep of amx_ctc_score.hip in its layout (one workgroup per
// row, strips of 64 states, SPW strips per wave, two LDS rows, the emission gathered PF frames ahead) and stores both
// a[t][i] and b[t][i] to the workspace, states contiguous; it writes ll and the status.  Unlike the scoring kernel it goes on
// when ll is -inf, because a transcript without a path can still have feasible deletions.
//
// An edit at position l leaves a left of it and b right of it unchanged, so a variant is a recursion of one or two states
// over the frames that bridges them.  The variants kernel runs one wave per (row, slot, strip of 64 classes): slot 2l + 1 is
// the substitution row l, slot 2p the insertion row p, and the lane is the class, so lp[t][c .. c + 63] is one coalesced
// 256-byte read per frame, taken PF frames ahead.  Both kinds of slot enter the bridging state from a[t-1][2k] and
// a[t-1][2k-1] (k = slot / 2); they differ in how they leave it.  The lattice values a frame needs are the same for every
// lane.  The wave reads them 64 frames at a time, a frame per lane (a gather down the [t][state] rows, one block ahead of
// its use), forms there whatever does not depend on the class -- lse(a0, a1), lse(b0, b1) -- and the frame loop broadcasts
// lane t of the block to the wave (v_readlane).  That leaves two lse per frame and class to a substitution slot and three to
// an insertion slot, the running one in the linear domain.  A lane carries v (or u, w) and the running sum in registers;
// there is no LDS, no barrier and no atomic.  The lane whose class is the blank takes the deletion (or ll) by select.
#include "amx_common.h"
#include "../../include/allophant_amx_variants.h"

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
__device__ __forceinline__ float lse2(float x0, float x1) {
    const float m = fmaxf(x0, x1);
    const float shift = m == -INFINITY ? 0.0f : m;
    return shift + __logf(__expf(x0 - shift) + __expf(x1 - shift));
}

// Where a[t][i] (or b[t][i]) of one row lies in its T x W floats of the workspace: states contiguous, so that a strip of the
// lattice kernel stores one 256-byte line per frame.
__device__ __forceinline__ int64_t lattice_at(int64_t t, int64_t i, int64_t W) { return t * W + i; }

template <int SPW, int PF>
__global__ __launch_bounds__(ALIGN_MAX_WAVES * CTC_WAVE) void ctc_lattice_kernel(VariantsArgs a) {
    extern __shared__ float state_rows[];  // two rows of a.strips * 64 states
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (CTC_WAVE - 1), wave = tid / CTC_WAVE, waves = blockDim.x / CTC_WAVE;
    const float neg_inf = -INFINITY;

    CtcRow row;
    if (!ctc_open_row(a, r, r, 0, row)) {
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
    float* forward = a.forward + r * a.T * W;    // a[t][i] at forward[lattice_at(t, i, ...)]
    float* backward = a.backward + r * a.T * W;  // b[t][i] likewise

    bool live[SPW], skip[SPW];
    int lab[SPW];
    float own[SPW], ahead[SPW][PF];
#pragma unroll
    for (int k = 0; k < SPW; ++k) {
        const int strip = k * waves + wave, i = strip * CTC_WAVE + lane;
        live[k] = strip * CTC_WAVE < S;  // wave-uniform; the lanes past S compute cells nobody reads
        lab[k] = row.blank, skip[k] = false, own[k] = i == 0 ? 0.0f : neg_inf;
#pragma unroll
        for (int j = 0; j < PF; ++j) ahead[k][j] = 0.0f;
        if (live[k]) {
            if (i < S && (i & 1)) {
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
                        forward[lattice_at(t, i, W)] = own[k];
                        if (t + PF < len) ahead[k][j] = lp[(int64_t)(t + PF) * st + lab[k]];
                    }
                }
                __syncthreads();  // the row is complete
            }
        }
    }

    const float* last = (len & 1) ? row1 : row0;
    const float ll = lse3(last[S - 1], S > 1 ? last[S - 2] : neg_inf, neg_inf);
    __syncthreads();  // every wave has read the end states: the rows now serve the backward sweep

#pragma unroll
    for (int k = 0; k < SPW; ++k) {
        const int i = (k * waves + wave) * CTC_WAVE + lane;
        own[k] = i == S - 1 ? 0.0f : neg_inf;
        // from here `skip` is the backward skip, to state i + 2
        skip[k] = live[k] && (i & 1) && i + 2 < S && y[(i >> 1) + 1] != lab[k];
#pragma unroll
        for (int j = 0; j < PF; ++j) ahead[k][j] = 0.0f;
        if (live[k]) {
            row0[i] = own[k];  // the virtual frame after the last
#pragma unroll
            for (int j = 0; j < PF; ++j)
                if (len - 1 - j >= 0) ahead[k][j] = lp[(int64_t)(len - 1 - j) * st + lab[k]];
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
                        own[k] = lse3(own[k], x1, x2) + ahead[k][j];
                        cur[i] = own[k];
                        backward[lattice_at(t, i, W)] = own[k];
                        if (t - PF >= 0) ahead[k][j] = lp[(int64_t)(t - PF) * st + lab[k]];
                    }
                }
                __syncthreads();
            }
        }
    }

    if (tid == 0) {
        a.log_likelihood[r] = ll;
        a.status[r] = 0;
    }
}

// The running lse over the frames, kept as a maximum and a sum in the linear domain: two exp per term and one log at the end,
// where an lse per term costs a log each (measured: DESIGN.md).  An empty or all -inf sum is -inf.
struct RunningLse {
    float m = -INFINITY, s = 0.0f;
    __device__ __forceinline__ void add(float term) {
        const float top = fmaxf(m, term), shift = top == -INFINITY ? 0.0f : top;
        s = s * __expf(m - shift) + __expf(term - shift);
        m = top;
    }
    __device__ __forceinline__ float value() const { return m == -INFINITY ? m : m + __logf(s); }
};

template <int PF>
__global__ __launch_bounds__(CTC_WAVE) void ctc_variants_kernel(VariantsArgs a) {
    static_assert(CTC_WAVE % PF == 0, "a block of frames holds whole turns of the emission ring");
    const int64_t r = a.row_base + blockIdx.y;
    if (a.status[r] != 0) return;  // (written by the lattice kernel, which has validated the row)
    const int class_strips = (a.C + CTC_WAVE - 1) / CTC_WAVE;
    const int slot = blockIdx.x / class_strips, lane = threadIdx.x;
    const int c = (blockIdx.x % class_strips) * CTC_WAVE + lane;
    const int lb = a.target_offsets[r], L = a.target_offsets[r + 1] - lb;
    if (slot > 2 * L) return;
    const int len = a.frame_lengths[r], S = 2 * L + 1, W = a.strips * CTC_WAVE, blank = a.blank;
    const int32_t* y = a.target_ids + lb;
    const float* lp = a.emissions + r * a.stride_n;
    const int64_t st = a.stride_t;
    const float* forward = a.forward + r * a.T * W;
    const float* backward = a.backward + r * a.T * W;
    const float neg_inf = -INFINITY;

    const bool substitution = slot & 1;  // wave-uniform, like everything that is not named after the lane's class
    const int k = slot >> 1;             // the position l or the gap p; the bridging state is entered from 2k and 2k - 1
    const int cl = min(c, a.C - 1);      // the lanes past C read the last class and store nothing
    const int left = k >= 1 ? y[k - 1] : -1, here = k < L ? y[k] : -1, right = k + 1 < L ? y[k + 1] : -1;
    const bool from_left = k >= 1 && cl != left;       // a[.][2k-1] enters the new symbol
    const bool to_right = k + 1 < L && cl != right;    // substitution: the new symbol steps over the blank to y[l+1]
    const bool to_here = cl != here;                   // insertion: the new symbol steps to y[p] without a blank (p == L: the end)
    const bool is_blank = cl == blank;
    const bool deletion_left = k >= 1 && (k + 1 == L || left != right);
    // the exits: substitution b[.][2l+2] and b[.][2l+3], insertion b[.][2p+1]; a state past S - 1 exists only as the virtual frame's
    const int exit0 = substitution ? 2 * k + 2 : 2 * k + 1, exit1 = 2 * k + 3;
    const bool has0 = exit0 < S, has1 = substitution && exit1 < S;
    const float end0 = (substitution ? exit0 == S - 1 : k == L) ? 0.0f : neg_inf;  // b[len][exit0]

    // What the frames t0 .. t0 + 63 read besides the emission of the lane's class, a frame per lane: a0 = a[t-1][2k] and
    // aa = lse(a0, a[t-1][2k-1]), b0 = b[t+1][exit0] and bb = lse(b0, b[t+1][exit1]), each with its virtual frame and its range
    // applied, and as `last` b[t+1][exit1] itself (substitution slots: the deletion's x of the next frame) or lp[t][blank]
    // (insertion slots).  Whatever is the same for every class is computed here, 64 frames at a time; the frame loop
    // broadcasts it lane by lane.
    struct Block {
        float a0, aa, b0, bb, last;
    };
    auto stage = [&](int t0) {
        Block f{neg_inf, neg_inf, neg_inf, neg_inf, neg_inf};
        const int t = t0 + lane;
        if (t < len) {
            float a1 = neg_inf, b1 = neg_inf;
            if (t == 0) {
                f.a0 = k == 0 ? 0.0f : neg_inf;
            } else {
                f.a0 = forward[lattice_at(t - 1, 2 * k, W)];
                if (k >= 1) a1 = forward[lattice_at(t - 1, 2 * k - 1, W)];
            }
            if (t + 1 == len) {
                f.b0 = end0;
            } else {
                if (has0) f.b0 = backward[lattice_at(t + 1, exit0, W)];
                if (has1) b1 = backward[lattice_at(t + 1, exit1, W)];
            }
            f.aa = lse2(f.a0, a1), f.bb = lse2(f.b0, b1);
            f.last = substitution ? b1 : lp[(int64_t)t * st + blank];
        }
        return f;
    };
    auto of_lane = [](float value, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(value), j)); };

    float ahead[PF];  // lp[t][c] of the next PF frames, frame t in ahead[t % PF]
#pragma unroll
    for (int j = 0; j < PF; ++j) ahead[j] = j < len ? lp[(int64_t)j * st + cl] : 0.0f;
    Block block = stage(0);
    float v = neg_inf, w = neg_inf, z = neg_inf;  // z = lse(w, v) of the frame before
    RunningLse sum;
    // the deletion's x[t] for the frame at hand: b[t][2l+3], which the frame before read as its `last` (a substitution slot
    // has a target and so, at status 0, a frame)
    float x = has1 ? backward[lattice_at(0, exit1, W)] : neg_inf;

    for (int t0 = 0; t0 < len; t0 += CTC_WAVE) {
        const Block next = stage(t0 + CTC_WAVE);  // (nothing is read past the row's frames)
        const int count = min(CTC_WAVE, len - t0);
        for (int j0 = 0; j0 < count; j0 += PF) {
#pragma unroll
            for (int jj = 0; jj < PF; ++jj) {
                const int j = j0 + jj, t = t0 + j;
                if (j < count) {
                    const float e = ahead[jj];
                    if (t + PF < len) ahead[jj] = lp[(int64_t)(t + PF) * st + cl];
                    const float a0 = of_lane(block.a0, j), aa = of_lane(block.aa, j), b0 = of_lane(block.b0, j);
                    const float last = of_lane(block.last, j);
                    const float entered = lse2(v, from_left ? aa : a0);
                    if (substitution) {
                        v = entered + e;
                        const float variant = v + (to_right ? of_lane(block.bb, j) : b0);
                        const float deleted = (deletion_left ? aa : a0) + x;  // the term t - 1 of the deletion
                        sum.add(is_blank ? deleted : variant);
                        x = last;
                    } else {
                        w = z + last;
                        v = entered + e;
                        z = lse2(w, v);
                        sum.add((to_here ? z : w) + b0);
                    }
                }
            }
        }
        block = next;
    }
    if (substitution) {
        // the deletion's last term, t = len - 1: the frames end in 2l or 2l - 1 when y[l] was the last symbol
        if (k + 1 == L) {
            const float a0 = forward[lattice_at(len - 1, 2 * k, W)];
            const float a1 = deletion_left ? forward[lattice_at(len - 1, 2 * k - 1, W)] : neg_inf;
            if (is_blank) sum.add(lse2(a0, a1));
        }
        if (c < a.C) a.substitutions[(r * a.max_target + k) * a.C + c] = sum.value();
    } else {
        if (c < a.C) a.insertions[(r * (a.max_target + 1) + k) * a.C + c] = is_blank ? a.log_likelihood[r] : sum.value();
    }
}

}  // namespace

bool ctc_variants_workspace_bytes(int64_t rows, int64_t T, int64_t max_target, size_t* bytes) {
    const size_t states = (size_t)(ctc_strips(max_target) * CTC_WAVE);
    size_t total = 0;
    if (__builtin_mul_overflow((size_t)rows, (size_t)T, &total) || __builtin_mul_overflow(total, states, &total) ||
        __builtin_mul_overflow(total, 2 * sizeof(float), &total))
        return false;
    *bytes = total;
    return true;
}

void launch_ctc_variants(VariantsArgs a, hipStream_t s) {
    a.strips = (int)ctc_strips(a.max_target);
    a.backward = a.forward + a.rows * a.T * a.strips * CTC_WAVE;
    ctc_launch_rows(a, s, ctc_lattice_kernel<1, 4>, ctc_lattice_kernel<2, 4>, ctc_lattice_kernel<4, 2>, ctc_lattice_kernel<8, 1>);
    const unsigned slots = 2 * (unsigned)a.max_target + 1, class_strips = ((unsigned)a.C + CTC_WAVE - 1) / CTC_WAVE;
    for (a.row_base = 0; a.row_base < a.rows; a.row_base += VARIANTS_GRID_ROWS) {  // (a grid's y holds 65535 rows)
        const unsigned rows = (unsigned)min((int64_t)VARIANTS_GRID_ROWS, a.rows - a.row_base);
        hipLaunchKernelGGL(ctc_variants_kernel<4>, dim3(slots * class_strips, rows), dim3(CTC_WAVE), 0, s, a);
    }
}

}  // namespace amx
