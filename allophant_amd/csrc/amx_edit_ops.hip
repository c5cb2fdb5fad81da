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

    walk_operations(codes, x.code_stride, A, m, B, nb, cost, x.operations + r * x.max_ops * 5, lane);
    if (lane == 0) x.operation_counts[r] = cost;
}

}  // namespace

// Per row: the statistics row's layout for one candidate, then ceil(max_expected / 64) strips of code words.
bool edit_operations_workspace_bytes(int64_t rows, int64_t max_expected, int64_t max_actual, size_t* bytes) {
    EditOpsArgs x{};
    x.e.cap_a = (int)max_expected, x.e.cap_b = (int)max_actual;
    edit_layout(x);
    size_t total = 0;
    if (__builtin_mul_overflow((size_t)rows, (size_t)x.e.span, &total) || __builtin_mul_overflow(total, sizeof(int32_t), &total))
        return false;
    *bytes = total;
    return true;
}

void launch_edit_operations(EditOpsArgs x, hipStream_t s) {
    edit_layout(x);
    const EditArgs& a = x.e;
    const int64_t rows = (int64_t)a.O * a.N;
    hipLaunchKernelGGL(edit_ops_kernel, dim3((unsigned)rows), dim3(WAVE), 0, s, x);
}

}  // namespace amx
