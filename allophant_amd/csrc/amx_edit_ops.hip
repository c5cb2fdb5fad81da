// Edit operations of decoded hypotheses against labels (upstream `levensthein_operations` + `to_substitutions`, as run.py
// edits uses them on the first candidate); contract in include/allophant_amx_edit.h.
//
// One wave per (output, utterance) row.  The label and the candidate's tokens are expanded as for the statistics, and the
// same wavefront DP (amx_edit_dp.inc) runs over them.  The back-trace's move out of cell (i, j) depends only on its three
// predecessors, so the sweep records it as it computes the cell: two ballots per wave step, (diagonal, second) over the 64
// cells of the step, staged in registers and stored 64 steps at a time as one 16-byte word per (strip, step).  With `second`
// a diagonal is a substitution (the symbols differ) rather than a match, and a non-diagonal move a deletion rather than an
// insertion.
//
// The walk then starts at (m, n).  Every recorded operation lowers the cost by exactly 1 and a match by 0, so the walk ends
// after `cost` = M[m][n] operations, where upstream's reaches a cost of 0, and operation k (in walk order) is written at
// index cost - 1 - k: upstream's reversed list, with no reversal pass.  Cell (i, j) of strip s = (i - 1) / 64 lies at step
// t = j + (i - 1) % 64, and every move inside a strip lowers t by 1 or 2, so one wave-wide load of the 64 words below t
// serves at least 32 moves, read with readlane.  The walk is wave-uniform; records are staged one per lane and written 64 at
// a time, with their symbol ids read in parallel.
#include "amx_common.h"
#include "../../include/allophant_amx_edit.h"

namespace amx {

namespace {

#include "amx_edit_dp.inc"

// The sweep's hook for the operations: per strip s and step t, bit l of (diagonal lo, hi, second lo, hi) is lane l's move.
struct PathCodes {
    uint4* codes;    // this row's words: strip s, step t at codes[s * stride + t]
    int64_t stride;  // words per strip
    uint4 word;      // staged: lane c holds step 64 q + c of the current 64 steps
    __device__ void step(int s, int t, bool last, bool diag, bool second, int lane) {
        const unsigned long long d = __ballot(diag), q = __ballot(second);
        const int c = t & (WAVE - 1);
        if (lane == c) word = make_uint4((uint32_t)d, (uint32_t)(d >> 32), (uint32_t)q, (uint32_t)(q >> 32));
        if (c == WAVE - 1 || last) {
            const int col = (t & ~(WAVE - 1)) + lane;
            if (col <= t) codes[s * stride + col] = word;
        }
    }
};

__device__ __forceinline__ void flag_row(const EditOpsArgs& x, int64_t r, int value, int lane) {
    if (lane == 0) x.operation_counts[r] = value;
}

__global__ __launch_bounds__(WAVE) void edit_ops_kernel(EditOpsArgs x) {
    const EditArgs& a = x.e;
    const int64_t r = blockIdx.x;  // o * N + n
    const int lane = threadIdx.x;
    const int n = (int)(r % a.N), o = (int)(r / a.N);
    if (a.hyp_counts && a.hyp_counts[r] <= 0) return flag_row(x, r, -1, lane);
    const int g = a.groups[n];
    const int length = a.counts[r];
    const int lb = a.label_offsets[n], le = a.label_offsets[n + 1];
    if (g < 0 || g >= a.G || length < 0 || length > a.T || lb < 0 || le < lb) return flag_row(x, r, -2, lane);
    int32_t* ws = a.workspace + r * a.span;
    int32_t* A = ws;
    int32_t* B = ws + a.cap_a_pad;
    int2* bnd0 = reinterpret_cast<int2*>(B + a.cap_b_pad);
    int2* bnd1 = bnd0 + a.bnd_pad;
    uint4* codes = reinterpret_cast<uint4*>(ws + x.codes_at);
    const int32_t* lmap = a.label_maps + 2 * o;
    const int32_t* hmap = a.hyp_maps + 2 * ((int64_t)(a.H > 1 ? g : 0) * a.O + o);
    const int m = expand(a.label_ids + lb, le - lb, a.map_offsets + lmap[0], a.map_values, lmap[1], A, a.cap_a, lane);
    const int64_t* tokens = a.tokens + o * a.stride_o + n * a.stride_n;
    const int nb = m < 0 ? -1 : expand(tokens, length, a.map_offsets + hmap[0], a.map_values, hmap[1], B, a.cap_b, lane);
    if (m < 0 || nb < 0) return flag_row(x, r, -2, lane);
    wave_fence();  // the expansions are read back by other lanes
    PathCodes path{codes, x.code_stride, make_uint4(0, 0, 0, 0)};
    const int cost = carried_dp(A, m, B, nb, bnd0, bnd1, lane, path).x;  // its last strip ends with a fence: the codes are visible

    int32_t* out = x.operations + r * x.max_ops * 5;
    int i = m, j = nb, k = 0, written = 0;
    int win_s = -1, win_t = 0;  // the loaded window: strip win_s, steps [win_t, win_t + 64)
    uint4 w = make_uint4(0, 0, 0, 0);
    int rec_act = 0, rec_i = 0, rec_j = 0;  // lane q stages operation written + q
    while (k < cost && (i > 0 || j > 0)) {  // (the origin is never reached first; the guard keeps every index in range)
        int act = 0;  // 0: a match, recorded as nothing
        if (i == 0) {
            act = AMX_EDIT_INSERTION, --j;
        } else if (j == 0) {
            act = AMX_EDIT_DELETION, --i;
        } else {
            const int s = (i - 1) / WAVE, l = (i - 1) % WAVE, t = j + l;
            if (s != win_s || t < win_t) {
                win_s = s, win_t = max(0, t - (WAVE - 1));
                w = codes[s * x.code_stride + win_t + lane];  // win_t + 63 <= max(t, 63) < code_stride
            }
            const int q = t - win_t, bit = l & 31;
            const bool diag = ((uint32_t)lane_value(l < 32 ? w.x : w.y, q) >> bit) & 1;
            const bool second = ((uint32_t)lane_value(l < 32 ? w.z : w.w, q) >> bit) & 1;
            if (diag) {
                --i, --j;
                if (second) act = AMX_EDIT_SUBSTITUTION;
            } else if (second) {
                act = AMX_EDIT_DELETION, --i;
            } else {
                act = AMX_EDIT_INSERTION, --j;
            }
        }
        if (act == 0) continue;
        if (lane == k - written) rec_act = act, rec_i = i, rec_j = j;  // the coordinates after the move
        ++k;
        if (k - written == WAVE || k == cost) {
            const int q = written + lane;
            if (q < k) {
                int32_t* rec = out + (int64_t)(cost - 1 - q) * 5;
                rec[0] = rec_act, rec[1] = rec_i, rec[2] = rec_j;
                rec[3] = rec_act != AMX_EDIT_INSERTION ? A[rec_i] : -1;
                rec[4] = rec_act != AMX_EDIT_DELETION ? B[rec_j] : -1;
            }
            written = k;
        }
    }
    if (lane == 0) x.operation_counts[r] = cost;
}

}  // namespace

// Per row: the statistics row's layout for one candidate, then ceil(max_expected / 64) strips of code words.
bool edit_operations_workspace_bytes(int64_t rows, int64_t max_expected, int64_t max_actual, size_t* bytes) {
    const int64_t codes = (max_expected + WAVE - 1) / WAVE * edit_pad(max_actual + WAVE) * 4;  // int32 per row
    const int64_t span = edit_pad(max_expected) + edit_pad(max_actual) + 4 * edit_pad(max_actual + 1) + codes;
    size_t total = 0;
    if (__builtin_mul_overflow((size_t)rows, (size_t)span, &total) || __builtin_mul_overflow(total, sizeof(int32_t), &total))
        return false;
    *bytes = total;
    return true;
}

void launch_edit_operations(EditOpsArgs x, hipStream_t s) {
    EditArgs& a = x.e;
    a.cap_a_pad = edit_pad(a.cap_a);
    a.cap_b_pad = edit_pad(a.cap_b);
    a.bnd_pad = edit_pad(a.cap_b + 1);  // int2 cells per boundary row
    x.codes_at = a.cap_a_pad + a.cap_b_pad + 4 * a.bnd_pad;
    x.code_stride = edit_pad(a.cap_b + WAVE);  // steps t <= n + 63 of a strip
    a.span = x.codes_at + (a.cap_a + WAVE - 1) / WAVE * x.code_stride * 4;
    const int64_t rows = (int64_t)a.O * a.N;
    hipLaunchKernelGGL(edit_ops_kernel, dim3((unsigned)rows), dim3(WAVE), 0, s, x);
}

}  // namespace amx
