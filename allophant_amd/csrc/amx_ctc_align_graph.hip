// CTC forced alignment over a graph of alternative label sequences (Viterbi); contract in include/allophant_amx_align_graph.h.
//
// The frame of amx_ctc_align.hip: one workgroup per row, the S = 2L + 1 states cut into strips of 64, wave w owning strips
// w, w + waves, ... (SPW of them, a template parameter), one state per lane, the previous frame's row double-buffered in LDS
// with one barrier per frame, and lp[t][label] gathered PF frames ahead.  What a state reads from the previous row is no longer
// its two left neighbours but up to seven sources: slot 0 is move 1 (the leading blank of a label state), slots 1..6 are the
// predecessors' label states (for E: the finals').  A lane keeps them as 13-bit row indices packed into three registers; an absent
// candidate is the index of a slot past every state that always holds -inf, so it never wins a strict comparison.  The
// strip's largest in-degree is a wave-uniform loop bound: a chain-like strip gathers one predecessor.
//
// The moves (0..7) are recorded as three ballots per (frame, strip), one per bit, in a 32-byte record at
// workspace[strip][frame]; they are staged one frame per lane and stored 64 frames at a time where the registers allow.
// Wave 0 walks back from the end state, wave-uniformly: a move >= 2 is decoded through the node's arc list (its offset
// and first predecessor wait in LDS, where the state rows are dead by then; a later predecessor is read from the CSR
// arrays).  Paths and frame scores are written 64 frames at a time; the span bounds go through LDS, start as (-1, -1), and one
// thread per node writes them out and adds the node's frame scores in frame order.  No atomics anywhere.
#include "amx_common.h"
#include "../../include/allophant_amx_align_graph.h"

#include <cmath>

namespace amx {

namespace {

#include "amx_ctc_row.inc"

constexpr int GRAPH_IN = AMX_ALIGN_GRAPH_MAX_IN;
constexpr int GRAPH_CHUNKS = (AMX_ALIGN_GRAPH_MAX_NODES + CTC_WAVE - 1) / CTC_WAVE;  // chunks of 64 nodes
constexpr int SOURCE_BITS = 13;
static_assert(2 * AMX_ALIGN_GRAPH_MAX_NODES + 1 < (1 << SOURCE_BITS), "a source index is kept in 13 bits");

// the candidate sources of one state: slot 0 (move 1) and slots 1 .. 6 (moves 2 .. 7), 13 bits each in one 96-bit string
// (the slots are compile-time constants where the sweep reads them: a shift, or one alignbit across two words)
struct Sources {
    uint32_t word[3];
};
__device__ __forceinline__ int source_of(const Sources& s, int slot) {
    const int bit = SOURCE_BITS * slot, w = bit >> 5;
    const uint64_t two = s.word[w] | ((uint64_t)(w < 2 ? s.word[w + 1] : 0u) << 32);
    return (int)((two >> (bit & 31)) & ((1u << SOURCE_BITS) - 1));
}
__device__ __forceinline__ void set_source(Sources& s, int slot, int index) {
    const int bit = SOURCE_BITS * slot, w = bit >> 5;
    const uint64_t mask = (uint64_t)((1u << SOURCE_BITS) - 1) << (bit & 31), value = (uint64_t)(uint32_t)index << (bit & 31);
    s.word[w] = (s.word[w] & ~(uint32_t)mask) | (uint32_t)value;
    if (w < 2) s.word[w + 1] = (s.word[w + 1] & ~(uint32_t)(mask >> 32)) | (uint32_t)(value >> 32);
}

template <int SPW, int PF, bool STAGED>
__global__ __launch_bounds__(ALIGN_MAX_WAVES * CTC_WAVE) void ctc_align_graph_kernel(AlignGraphArgs a) {
    extern __shared__ float state_rows[];  // two rows of a.strips * 64 states; later the span bounds and the arc lists' heads
    __shared__ int final_count[GRAPH_CHUNKS];  // final nodes per chunk of 64 nodes
    __shared__ int finals[GRAPH_IN];           // the final nodes, ascending
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (CTC_WAVE - 1), wave = tid / CTC_WAVE, waves = blockDim.x / CTC_WAVE;
    const float neg_inf = -INFINITY;

    int64_t n = r, block = 0;  // utterance r of one tensor, or row o * N + n over the output blocks
    if (a.descs) n = (int)(r % a.N), block = r / a.N;
    CtcRow row;
    if (!ctc_open_row(a, r, n, block, row)) {  // frame length, node offsets, node count and classes
        if (tid == 0) a.status[r] = -2;
        return;
    }
    const float* lp = row.lp;
    const int64_t st = row.st;
    const int blank = row.blank, len = row.len, L = row.L;
    const int32_t* y = row.y;
    const int node_base = a.target_offsets[r];
    const int32_t* flags = a.node_flags + node_base;
    const int32_t* arcs = a.arc_offsets + node_base;  // arcs[j] .. arcs[j + 1] in arc_preds
    const int arc_count = a.arc_offsets[a.target_offsets[a.rows]];

    // the graph: arc offsets, in-degrees, predecessors, initial and final nodes (chunk c of 64 nodes belongs to one wave)
    int wrong = 0, initial = 0;
    for (int base = 0; base < L; base += blockDim.x) {
        const int j = base + tid;
        bool is_final = false;
        if (j < L) {
            const int f = flags[j], ab = arcs[j], ae = arcs[j + 1];
            initial |= f & 1;
            is_final = (f & 2) != 0;
            if (ab < 0 || ae < ab || ae > arc_count || ae - ab > GRAPH_IN) {
                wrong = 1;
            } else {
                for (int q = ab; q < ae; ++q) {
                    const int p = a.arc_preds[q];
                    wrong |= p < 0 || p >= j;
                }
            }
        }
        const unsigned long long b = __ballot(is_final);
        const int chunk = (base >> 6) + wave;
        if (lane == 0 && chunk * CTC_WAVE < L) final_count[chunk] = __popcll(b);
    }
    wrong = __syncthreads_or(wrong);
    initial = __syncthreads_or(initial);
    int final_nodes = 0;
    for (int c = 0; c * CTC_WAVE < L; ++c) final_nodes += final_count[c];
    if (wrong || (L > 0 && (!initial || final_nodes == 0 || final_nodes > GRAPH_IN))) {
        if (tid == 0) a.status[r] = -2;
        return;
    }

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

    const int S = 2 * L + 1, E = 2 * L;
    const int absent = a.strips * CTC_WAVE - 1;  // past every state (S is odd): holds -inf in both rows
    float* row0 = state_rows;
    float* row1 = state_rows + a.strips * CTC_WAVE;
    uint4* moves = a.workspace + r * a.strips * a.t_pad * 2;

    for (int base = 0; base < L; base += blockDim.x) {
        const int j = base + tid;
        const bool is_final = j < L && (flags[j] & 2);
        const unsigned long long b = __ballot(is_final);
        if (is_final) {
            int rank = __popcll(b & ((1ull << lane) - 1));
            for (int c = 0; c < (base >> 6) + wave; ++c) rank += final_count[c];
            finals[rank] = j;
        }
    }
    if (tid == 0) row0[absent] = neg_inf, row1[absent] = neg_inf;
    __syncthreads();

    int lab[SPW];
    uint32_t degrees = 0;  // per strip 3 bits: its largest candidate count past slot 0, wave-uniform
    Sources from[SPW];
    float x0[SPW], ahead[SPW][PF];
    uint4 word[STAGED ? SPW : 1][2];  // STAGED: lane c holds the strip's record of frame 64 q + c until 64 frames are stored at once
#pragma unroll
    for (int k = 0; k < SPW; ++k) {
        const int strip = k * waves + wave, i = strip * CTC_WAVE + lane;
        const bool live = strip * CTC_WAVE < S;  // wave-uniform
        const bool mine = i < S;                 // the lanes past S keep -inf
        lab[k] = blank, x0[k] = neg_inf;
        from[k].word[0] = from[k].word[1] = from[k].word[2] = 0;
#pragma unroll
        for (int q = 0; q <= GRAPH_IN; ++q) set_source(from[k], q, absent);
        if (STAGED) word[k][0] = word[k][1] = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < PF; ++j) ahead[k][j] = 0.0f;
        if (live) {
            int d = 0;
            if (mine && i == E) {
                d = final_nodes;
#pragma unroll
                for (int q = 0; q < GRAPH_IN; ++q)
                    if (q < d) set_source(from[k], 1 + q, 2 * finals[q] + 1);
                if (L == 0) x0[k] = lp[blank];
            } else if (mine) {
                const int j = i >> 1;
                const bool label = i & 1;
                if (label) {
                    lab[k] = y[j];
                    set_source(from[k], 0, i - 1);
                }
                const int ab = arcs[j];
                d = arcs[j + 1] - ab;
#pragma unroll
                for (int q = 0; q < GRAPH_IN; ++q) {
                    if (q < d) {
                        const int p = a.arc_preds[ab + q];
                        if (!label || y[p] != lab[k]) set_source(from[k], 1 + q, 2 * p + 1);
                    }
                }
                if (flags[j] & 1) x0[k] = lp[lab[k]];
            }
#pragma unroll
            for (int q = 1; q <= GRAPH_IN; ++q)
                if (__ballot(d >= q)) degrees = (degrees & ~(7u << (3 * k))) | ((uint32_t)q << (3 * k));
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
                    const int strip = k * waves + wave, i = strip * CTC_WAVE + lane;
                    if (strip * CTC_WAVE < S) {  // wave-uniform
                        const int degree = (degrees >> (3 * k)) & 7;
                        float best = x0[k];
                        int m = 0;
                        // the first two sources are read together, as the chain kernel reads its two neighbours (an
                        // absent one reads -inf); only a strip with a second predecessor goes on
                        const float x1 = prev[source_of(from[k], 0)], x2 = prev[source_of(from[k], 1)];
                        if (x1 > best) best = x1, m = 1;
                        if (x2 > best) best = x2, m = 2;
#pragma unroll
                        for (int q = 1; q < GRAPH_IN; ++q) {
                            if (q < degree) {
                                const float x = prev[source_of(from[k], 1 + q)];
                                if (x > best) best = x, m = 2 + q;
                            }
                        }
                        x0[k] = i < S ? best + ahead[k][j] : neg_inf;  // the lanes past S keep -inf
                        cur[i] = x0[k];
                        if (t + PF < len) ahead[k][j] = lp[(int64_t)(t + PF) * st + lab[k]];
                        const unsigned long long b0 = __ballot(m & 1), b1 = __ballot(m & 2), b2 = __ballot(m & 4);
                        const uint4 low = make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
                        const uint4 high = make_uint4((uint32_t)b2, (uint32_t)(b2 >> 32), 0, 0);
                        uint4* records = moves + (strip * a.t_pad) * 2;
                        if (STAGED) {
                            if (lane == c) word[k][0] = low, word[k][1] = high;
                            if ((c == CTC_WAVE - 1 || t == len - 1) && lane <= c) {
                                records[(t - c + lane) * 2] = word[k][0];
                                records[(t - c + lane) * 2 + 1] = word[k][1];
                            }
                        } else if (lane == c) {
                            records[t * 2] = low;
                            records[t * 2 + 1] = high;
                        }
                    }
                }
                __syncthreads();  // the row is complete (and, after the last frame, the moves are visible to wave 0)
            }
        }
    }

    const float* last = ((len - 1) & 1) ? row1 : row0;
    int e = E;
    float total = last[E];
    if (final_nodes) {
        e = 2 * finals[0] + 1, total = last[e];
        for (int q = 1; q < final_nodes; ++q) {
            const int i = 2 * finals[q] + 1;
            const float x = last[i];
            if (x > total) total = x, e = i;
        }
        const float x = last[E];
        if (x > total) total = x, e = E;
    }
    if (total == neg_inf) {
        if (tid == 0) a.status[r] = -1;
        return;
    }
    __syncthreads();  // every wave has read the end states: the rows now hold the span bounds and the arc lists' heads

    int* first = reinterpret_cast<int*>(state_rows);  // [L], then the ends [L], the arc offsets [L + 1] and first predecessors [L]
    int* past = first + L;
    int* arc_head = past + L;
    int* pred0 = arc_head + L + 1;  // 4 L + 2 ints in all, within the 2 * strips * 64 >= 4 L + 4 of the rows
    float* frame_scores = a.frame_scores + r * a.T;
    for (int l = tid; l < L; l += blockDim.x) {
        const int ab = arcs[l];
        first[l] = -1, past[l] = -1;  // an unvisited node
        arc_head[l] = ab;
        pred0[l] = arcs[l + 1] > ab ? a.arc_preds[ab] : 0;
    }
    if (tid == 0) arc_head[L] = arcs[L];
    __syncthreads();
    if (wave == 0) {
        int after_block = -1;  // the state of the frame after the 64 being walked
        for (int tb = (len - 1) & ~(CTC_WAVE - 1); tb >= 0; tb -= CTC_WAVE) {
            const int hi = min(len - 1, tb + CTC_WAVE - 1);
            int own = -1, loaded = -1;
            uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
            for (int t = hi; t >= tb; --t) {
                if (lane == t - tb) own = e;
                if (t > 0) {
                    const int strip = e >> 6, bit = e & 63;
                    if (strip != loaded) {
                        const uint4* records = moves + (strip * a.t_pad + tb + lane) * 2;
                        w0 = records[0], w1 = records[1];
                        loaded = strip;
                    }
                    const uint32_t m0 = __builtin_amdgcn_readlane(bit < 32 ? w0.x : w0.y, t - tb);
                    const uint32_t m1 = __builtin_amdgcn_readlane(bit < 32 ? w0.z : w0.w, t - tb);
                    const uint32_t m2 = __builtin_amdgcn_readlane(bit < 32 ? w1.x : w1.y, t - tb);
                    const int m = ((m0 >> (bit & 31)) & 1) + 2 * ((m1 >> (bit & 31)) & 1) + 4 * ((m2 >> (bit & 31)) & 1);
                    if (m == 1) {
                        e = max(e - 1, 0);
                    } else if (m >= 2) {  // (the range checks can fail only on a NaN-ridden row)
                        const int q = m - 2;
                        if (e == E) {
                            if (q < final_nodes) e = 2 * finals[q] + 1;
                        } else {
                            const int j = e >> 1, ab = arc_head[j];
                            if (ab + q < arc_head[j + 1]) e = 2 * (q == 0 ? pred0[j] : a.arc_preds[ab + q]) + 1;
                        }
                        e = __builtin_amdgcn_readfirstlane(e);
                    }
                }
            }
            // frame tb + lane has state `own`; e is now the state of frame tb - 1
            const int t = tb + lane;
            const int up = __shfl_up(own, 1), down = __shfl_down(own, 1);
            const int before = lane > 0 ? up : (tb > 0 ? e : -1);
            const int after = t < hi ? down : after_block;
            if (t <= hi) {
                const int label = (own & 1) ? y[own >> 1] : blank;
                paths[t] = label;
                frame_scores[t] = lp[(int64_t)t * st + label];
                if (own & 1) {
                    const int l = own >> 1;
                    if (before != own) first[l] = t;
                    if (after != own) past[l] = t + 1;
                }
            }
            after_block = __builtin_amdgcn_readfirstlane(own);
        }
    }
    for (int t = len + tid; t < a.T; t += blockDim.x) paths[t] = -1;
    __syncthreads();

    int32_t* spans = a.spans + r * a.max_target * 2;
    for (int l = tid; l < L; l += blockDim.x) {
        const float* column = lp + y[l];
        const int begin = first[l], end = past[l];
        float sum = 0.0f;
        for (int t = begin; t < end; ++t) sum = sum + column[(int64_t)t * st];  // the values frame_scores holds
        spans[2 * l] = begin, spans[2 * l + 1] = end;
        a.span_scores[r * a.max_target + l] = sum;
    }
    if (tid == 0) {
        a.totals[r] = total;
        a.status[r] = 0;
    }
}

}  // namespace

bool ctc_align_graph_workspace_bytes(int64_t rows, int64_t T, int64_t max_nodes, size_t* bytes) {
    const size_t strips = (size_t)ctc_strips(max_nodes), t_pad = (size_t)((T + CTC_WAVE - 1) / CTC_WAVE * CTC_WAVE);
    size_t total = 0;
    if (__builtin_mul_overflow((size_t)rows, strips, &total) || __builtin_mul_overflow(total, t_pad, &total) ||
        __builtin_mul_overflow(total, 2 * sizeof(uint4), &total))
        return false;
    *bytes = total;
    return true;
}

void launch_ctc_align_graph(AlignGraphArgs a, hipStream_t s) {
    a.strips = (int)ctc_strips(a.max_target);
    a.t_pad = ((int64_t)a.T + CTC_WAVE - 1) / CTC_WAVE * CTC_WAVE;
    ctc_launch_rows(a, s, ctc_align_graph_kernel<1, 4, true>, ctc_align_graph_kernel<2, 4, true>,
                    ctc_align_graph_kernel<4, 2, false>, ctc_align_graph_kernel<8, 1, false>);
}

}  // namespace amx
