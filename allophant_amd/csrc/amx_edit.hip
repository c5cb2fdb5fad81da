// Edit statistics of decoded hypotheses against labels (upstream `levensthein_statistics` + run.py evaluate's candidate choice);
// contract in include/allophant_amx_edit.h.
//
// One wave scores one (output, utterance, candidate) row.  It first expands the label ids and the candidate's tokens through
// their CSR maps into the row's workspace (a wave-wide prefix sum places every entry's expansion).  The DP then never keeps
// the matrix: the back-trace's step out of cell (i, j) depends only on M[i][j] and its three predecessors, so the walk's
// counts ride forward with the cost.  Each cell carries (cost, S << 16 | D) of the walk that starts there; at the end
// C = m - S - D and I = n - C - S.  Lane l owns expected row i = 64 s + l + 1 of strip s and the wave sweeps the
// hypothesis as an anti-diagonal: at step t lane l computes column j = t - l, with the cell above and the diagonal arriving
// from lane l - 1 by a DPP wave shift.  Lane 0 reads the strip's top boundary, and lane 63's cells become the next strip's,
// through two boundary rows in the workspace, staged 64 columns at a time in registers.
#include "amx_common.h"
#include "../../include/allophant_amx_edit.h"

namespace amx {

namespace {

constexpr int WAVE = 64;
constexpr int SELECT_THREADS = 256;

// wave_shr:1 -- lane l receives lane l - 1's `v`, lane 0 receives `lane0`
__device__ __forceinline__ int shift_in(int lane0, int v) {
    return __builtin_amdgcn_update_dpp(lane0, v, 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ int lane_value(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

__device__ __forceinline__ int inclusive_scan(int v, int lane) {
    for (int d = 1; d < WAVE; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// Expands ids src[0, len) through the map whose entry e spans values[offsets[e] .. offsets[e + 1]) (e < entries) into
// out[0, cap).  Returns the expanded length, or -1 when an id lies outside the map or the expansion exceeds `cap`: nothing
// outside the map or past `cap` is touched.
template <typename Id>
__device__ int expand(const Id* src, int64_t len, const int32_t* offsets, const int32_t* values, int entries, int32_t* out,
                      int cap, int lane) {
    int pos = 0;
    for (int64_t base = 0; base < len; base += WAVE) {
        const int64_t idx = base + lane;
        bool bad = false;
        int first = 0, count = 0;
        if (idx < len) {
            const int64_t id = (int64_t)src[idx];
            if (id < 0 || id >= entries) {
                bad = true;
            } else {
                first = offsets[id];
                count = offsets[id + 1] - first;
                if (count < 0 || count > AMX_EDIT_MAX_LENGTH) bad = true, count = 0;
            }
        }
        const int incl = inclusive_scan(count, lane);
        const int total = lane_value(incl, WAVE - 1);
        if (__any(bad) || pos + total > cap) return -1;
        const int start = pos + incl - count;
        for (int e = 0; e < count; ++e) out[start + e] = values[first + e];
        pos += total;
    }
    return pos;
}

// The forward-carried DP of one row: expected A[0, m), actual B[0, n) (m, n <= 65535), boundary rows bnd0 / bnd1 of n + 1
// cells.  Returns (cost, S << 16 | D) of cell (m, n), identical in every lane.
__device__ int2 carried_dp(const int32_t* A, int m, const int32_t* B, int n, int2* bnd0, int2* bnd1, int lane) {
    if (m == 0) return make_int2(n, 0);
    const int strips = (m + WAVE - 1) / WAVE;
    int2* bin = bnd0;
    int2* bout = bnd1;
    int2 result = make_int2(0, 0);
    for (int s = 0; s < strips; ++s) {
        const int i0 = s * WAVE;
        const int i = i0 + lane + 1;
        const int ai = i <= m ? A[i - 1] : -1;
        const int last = min(WAVE - 1, m - i0 - 1);  // the lane of the strip's last row
        const bool top = s == 0, hand_on = s + 1 < strips;
        int cost = 0, sd = 0, up_c = 0, up_sd = 0, bj = 0;
        int in_c = 0, in_sd = 0, in_b = 0, out_c = 0, out_sd = 0;
        for (int t = 0; t <= n + last; ++t) {
            const int c = t & (WAVE - 1);
            if (c == 0) {  // the next 64 columns of lane 0's inputs
                const int col = t + lane;
                if (top) {
                    in_c = col, in_sd = 0;  // row 0: j insertions
                } else if (col <= n) {
                    const int2 v = bin[col];
                    in_c = v.x, in_sd = v.y;
                }
                const int bi = col - 1;
                in_b = bi >= 0 && bi < n ? B[bi] : -1;
            }
            const int dg_c = up_c, dg_sd = up_sd;
            up_c = shift_in(lane_value(in_c, c), cost);
            up_sd = shift_in(lane_value(in_sd, c), sd);
            bj = shift_in(lane_value(in_b, c), bj);
            const int j = t - lane;
            if (j == 0) {  // column 0: i deletions
                cost = i, sd = i;
            } else if (j > 0 && j <= n) {
                const int ch = min(up_c, cost);  // deletion if strictly cheaper, else insertion
                const int nc = min(ch + 1, dg_c + (ai == bj ? 0 : 1));
                int nsd = up_c < cost ? up_sd + 1 : sd;
                if (dg_c <= ch) nsd = dg_sd + (dg_c != nc ? 0x10000 : 0);  // the diagonal; correct when its cost is ours
                cost = nc;
                sd = nc == 0 ? 0 : nsd;  // the walk stops here: everything above is correct
            }
            if (hand_on) {  // lane 63's cell (i0 + 64, t - 63) goes to the next strip's top boundary
                const int jo = t - (WAVE - 1);
                if (jo >= 0 && jo <= n) {
                    const int vc = lane_value(cost, WAVE - 1), vs = lane_value(sd, WAVE - 1);
                    if (lane == (jo & (WAVE - 1))) out_c = vc, out_sd = vs;
                    if ((jo & (WAVE - 1)) == WAVE - 1 || jo == n) {
                        const int col = (jo & ~(WAVE - 1)) + lane;
                        if (col <= jo) bout[col] = make_int2(out_c, out_sd);
                    }
                }
            }
        }
        if (!hand_on) result = make_int2(lane_value(cost, last), lane_value(sd, last));
        int2* swap = bin;
        bin = bout;
        bout = swap;
        wave_fence();
    }
    return result;
}

__global__ __launch_bounds__(WAVE) void edit_rows_kernel(EditArgs a) {
    const int64_t r = blockIdx.x;  // (o * N + n) * K + k
    const int lane = threadIdx.x;
    const int k = (int)(r % a.K);
    const int64_t on = r / a.K;
    const int n = (int)(on % a.N), o = (int)(on / a.N);
    int32_t* st = a.statistics + r * 4;
    const int present = a.hyp_counts ? min(max(a.hyp_counts[on], 0), a.K) : a.K;
    if (k >= present) {
        if (lane < 4) st[lane] = -1;
        return;
    }
    const int g = a.groups[n];
    const int length = a.counts[r];
    const int lb = a.label_offsets[n], le = a.label_offsets[n + 1];
    if (g < 0 || g >= a.G || length < 0 || length > a.T || lb < 0 || le < lb) {
        if (lane < 4) st[lane] = -2;
        return;
    }
    int32_t* ws = a.workspace + r * a.span;
    int32_t* A = ws;
    int32_t* B = ws + a.cap_a_pad;
    int2* bnd0 = reinterpret_cast<int2*>(B + a.cap_b_pad);
    int2* bnd1 = bnd0 + a.bnd_pad;
    const int32_t* lmap = a.label_maps + 2 * o;
    const int32_t* hmap = a.hyp_maps + 2 * ((int64_t)(a.H > 1 ? g : 0) * a.O + o);
    const int m = expand(a.label_ids + lb, le - lb, a.map_offsets + lmap[0], a.map_values, lmap[1], A, a.cap_a, lane);
    const int64_t* tokens = a.tokens + o * a.stride_o + n * a.stride_n + k * a.stride_k;
    const int nb = m < 0 ? -1 : expand(tokens, length, a.map_offsets + hmap[0], a.map_values, hmap[1], B, a.cap_b, lane);
    if (m < 0 || nb < 0) {
        if (lane < 4) st[lane] = -2;
        return;
    }
    wave_fence();  // the expansions are read back by other lanes
    const int2 cell = carried_dp(A, m, B, nb, bnd0, bnd1, lane);
    const int S = (int)((uint32_t)cell.y >> 16), D = cell.y & 0xffff;
    const int C = m - S - D;
    const int I = nb - C - S;
    if (lane < 4) st[lane] = lane == 0 ? I : lane == 1 ? D : lane == 2 ? S : C;
}

// One thread per (output, utterance): the first candidate of strictly lowest fp32 word_error_rate, then its counts added.
__global__ __launch_bounds__(SELECT_THREADS) void edit_select_kernel(EditArgs a) {
    const int64_t on = (int64_t)blockIdx.x * SELECT_THREADS + threadIdx.x;
    if (on >= (int64_t)a.O * a.N) return;
    const int n = (int)(on % a.N), o = (int)(on / a.N);
    const int present = a.hyp_counts ? min(max(a.hyp_counts[on], 0), a.K) : a.K;
    const int g = a.groups[n];
    int best = g < 0 || g >= a.G ? -2 : -1;
    float lowest = __builtin_huge_valf();
    for (int k = 0; k < present && best != -2; ++k) {
        const int32_t* st = a.statistics + (on * a.K + k) * 4;
        if (st[0] < 0) {
            best = -2;
            break;
        }
        // edit_distance.rs word_error_rate: (f32(S + D) + f32(I)) / (f32(S + D) + f32(C)), correctly rounded
        const float sd = (float)(st[2] + st[1]);
        const float rate = (sd + (float)st[0]) / (sd + (float)st[3]);
        if (rate < lowest) lowest = rate, best = k;
    }
    a.best[on] = best;
    if (best >= 0) {
        const int32_t* st = a.statistics + (on * a.K + best) * 4;
        unsigned long long* total = reinterpret_cast<unsigned long long*>(a.totals) + ((int64_t)g * a.O + o) * 4;
        for (int q = 0; q < 4; ++q) atomicAdd(total + q, (unsigned long long)st[q]);
    }
}

}  // namespace

int64_t edit_pad(int64_t v) { return (v + 15) / 16 * 16; }

size_t edit_workspace_bytes(int64_t rows, int64_t max_expected, int64_t max_actual) {
    const int64_t span = edit_pad(max_expected) + edit_pad(max_actual) + 4 * edit_pad(max_actual + 1);
    return (size_t)rows * (size_t)span * sizeof(int32_t);
}

void launch_edit_statistics(EditArgs a, hipStream_t s) {
    a.cap_a_pad = edit_pad(a.cap_a);
    a.cap_b_pad = edit_pad(a.cap_b);
    a.bnd_pad = edit_pad(a.cap_b + 1);  // int2 cells per boundary row
    a.span = a.cap_a_pad + a.cap_b_pad + 4 * edit_pad(a.cap_b + 1);
    const int64_t rows = (int64_t)a.O * a.N * a.K;
    hipLaunchKernelGGL(edit_rows_kernel, dim3((unsigned)rows), dim3(WAVE), 0, s, a);
    const int64_t pairs = (int64_t)a.O * a.N;
    hipLaunchKernelGGL(edit_select_kernel, dim3((unsigned)((pairs + SELECT_THREADS - 1) / SELECT_THREADS)), dim3(SELECT_THREADS),
                       0, s, a);
}

}  // namespace amx
