// Edit statistics of decoded hypotheses against labels (upstream `levensthein_statistics` + run.py evaluate's candidate choice);
// contract in include/allophant_amx_edit.h.
//
// One wave scores one (output, utterance, candidate) row.  It first expands the label ids and the candidate's tokens through
// their CSR maps into the row's workspace (a wave-wide prefix sum places every entry's expansion).  The DP then never keeps
// the matrix: the back-trace's step out of cell (i, j) depends only on M[i][j] and its three predecessors, so the walk's
// counts ride forward with the cost.  Each cell carries (cost, S << 16 | D) of the walk that starts there; at the end
// C = m - S - D and I = n - C - S.  The expansion and the wavefront sweep live in amx_edit_dp.inc, shared with
// amx_edit_ops.hip.
#include "amx_common.h"
#include "../../include/allophant_amx_edit.h"

namespace amx {

namespace {

#include "amx_edit_dp.inc"

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
    NoPath path;
    const int2 cell = carried_dp(A, m, B, nb, bnd0, bnd1, lane, path);
    const int S = (int)((uint32_t)cell.y >> 16), D = cell.y & 0xffff;
    const int C = m - S - D;
    const int I = nb - C - S;
    if (lane < 4) st[lane] = lane == 0 ? I : lane == 1 ? D : lane == 2 ? S : C;
}

// One thread per (output, utterance): select_candidate of amx_edit_dp.inc.
__global__ __launch_bounds__(SELECT_THREADS) void edit_select_kernel(EditArgs a) { select_candidate(a); }

}  // namespace

int64_t edit_pad(int64_t v) { return (v + 15) / 16 * 16; }

// The layout of a row's workspace, in int32: expected, actual, two boundary rows of int2 cells, each padded to 16.  Every
// size that a caller is told and every offset that a kernel indexes with comes from here.
void edit_layout(EditArgs& a) {
    a.cap_a_pad = edit_pad(a.cap_a);
    a.cap_b_pad = edit_pad(a.cap_b);
    a.bnd_pad = edit_pad(a.cap_b + 1);  // int2 cells per boundary row
    a.span = a.cap_a_pad + a.cap_b_pad + 4 * a.bnd_pad;
}

// The operations' and confusions' row: the same, then the path codes, per strip of 64 expected symbols code_stride words of
// 16 bytes.
void edit_layout(EditOpsArgs& x) {
    EditArgs& a = x.e;
    edit_layout(a);
    x.codes_at = a.span;
    x.code_stride = edit_pad(a.cap_b + WAVE);  // steps t <= n + 63 of a strip
    a.span = x.codes_at + (a.cap_a + WAVE - 1) / WAVE * x.code_stride * 4;
}

size_t edit_workspace_bytes(int64_t rows, int64_t max_expected, int64_t max_actual) {
    EditArgs a{};
    a.cap_a = (int)max_expected, a.cap_b = (int)max_actual;
    edit_layout(a);
    return (size_t)rows * (size_t)a.span * sizeof(int32_t);
}

void launch_edit_statistics(EditArgs a, hipStream_t s) {
    edit_layout(a);
    const int64_t rows = (int64_t)a.O * a.N * a.K;
    hipLaunchKernelGGL(edit_rows_kernel, dim3((unsigned)rows), dim3(WAVE), 0, s, a);
    const int64_t pairs = (int64_t)a.O * a.N;
    hipLaunchKernelGGL(edit_select_kernel, dim3((unsigned)((pairs + SELECT_THREADS - 1) / SELECT_THREADS)), dim3(SELECT_THREADS),
                       0, s, a);
}

}  // namespace amx
