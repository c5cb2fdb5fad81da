// Feature-weighted edit distance (upstream `PropertyWeighting`: levensthein_statistics / _operations / _matrix with fp32
// insertion and deletion costs and the number of differing articulatory features as the substitution cost); contract in
// include/allophant_amx_edit.h.
//
// The rows, the CSR expansion and the wavefront sweep are those of amx_edit.hip / amx_edit_ops.hip: carried_dp of
// amx_edit_dp.inc runs here under the FeatureCosts model instead of UnitCosts.  Cells are fp32 and every cell performs
// upstream's additions and minima, one rounding each, so the costs are upstream's bit for bit; column 0 is built by repeated
// addition, 64 per strip.
//
// Substitution costs come from a pairwise table uint8 [V, V] per id space, built once by edit_cost_table_kernel from the
// feature codes uint8 [V, F]: one byte per cell, whatever F is, where keeping a_i's codes in registers and fetching b_j's
// would cost F bytes of registers and F compares per cell.  The gather is off the dependent chain: the hypothesis symbols
// run down the lanes in a second DPP pipeline AHEAD wave steps early, and a lane issues the load for the cell it reaches
// AHEAD steps later into slot t % AHEAD of a register queue (the sweep's inner loop is unrolled AHEAD times, so the slots
// are plain registers and a load is only waited for where it is used).
//
// An operation no longer lowers the cost by one, so the operations walk ends after S + D + I records, which the sweep's
// carried counts give before the walk starts; record k (in walk order) goes to index count - 1 - k.
#include "amx_common.h"
#include "../../include/allophant_amx_edit.h"

namespace amx {

namespace {

#include "amx_edit_dp.inc"

#include "amx_edit_feature_costs.inc"  // FeatureCosts: shared with amx_edit_weighted_confusion.hip

// Every id of ids[0, count) inside [0, V)?  (wave-uniform answer)
__device__ bool in_table(const int32_t* ids, int count, int V, int lane) {
    bool bad = false;
    for (int base = 0; base < count; base += WAVE) {
        const int idx = base + lane;
        if (idx < count) bad |= ids[idx] < 0 || ids[idx] >= V;
    }
    return !__any(bad);
}

// A scored row: the expanded sequences and the boundary rows in its workspace.
struct Row {
    int32_t *A, *B;
    int2 *bnd0, *bnd1;
    int m, nb;
};

// Row r = (o, n) [candidate k] of the uniform kernels, expanded, under output o's table.  Returns 0, or the row's flag:
// -2 as the uniform kernels flag it, or for a symbol outside the table.
__device__ int open_row(const EditWeightedArgs& w, int64_t r, int o, int n, int k, int lane, Row& row, FeatureCosts& costs) {
    const EditArgs& a = w.x.e;
    const int g = a.groups[n];
    const int length = a.counts[r];
    const int lb = a.label_offsets[n], le = a.label_offsets[n + 1];
    if (g < 0 || g >= a.G || length < 0 || length > a.T || lb < 0 || le < lb) return -2;
    int32_t* ws = a.workspace + r * a.span;
    row.A = ws;
    row.B = ws + a.cap_a_pad;
    row.bnd0 = reinterpret_cast<int2*>(row.B + a.cap_b_pad);
    row.bnd1 = row.bnd0 + a.bnd_pad;
    const int32_t* lmap = a.label_maps + 2 * o;
    const int32_t* hmap = a.hyp_maps + 2 * ((int64_t)(a.H > 1 ? g : 0) * a.O + o);
    row.m = expand(a.label_ids + lb, le - lb, a.map_offsets + lmap[0], a.map_values, lmap[1], row.A, a.cap_a, lane);
    if (row.m < 0) return -2;
    const int64_t* tokens = a.tokens + o * a.stride_o + n * a.stride_n + k * a.stride_k;
    row.nb = expand(tokens, length, a.map_offsets + hmap[0], a.map_values, hmap[1], row.B, a.cap_b, lane);
    if (row.nb < 0) return -2;
    wave_fence();  // the expansions are read back by other lanes
    const int64_t first = w.tables[2 * o], V = w.tables[2 * o + 1];
    costs.insertion = w.insertion_cost, costs.deletion = w.deletion_cost;
    costs.table = V > 0 ? w.table_data + first : nullptr;
    costs.V = (int)V;
    costs.matrix = nullptr, costs.ld = 0, costs.rows = 0;
    costs.column = 0.f;
    if (V > 0 && !(in_table(row.A, row.m, (int)V, lane) && in_table(row.B, row.nb, (int)V, lane))) return -2;
    return 0;
}

// table[x, y] = the number of feature columns in which codes[x] and codes[y] differ
__global__ __launch_bounds__(256) void edit_cost_table_kernel(const uint8_t* codes, int V, int F, uint8_t* table) {
    const int x = blockIdx.y;
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= V) return;
    const uint8_t* cx = codes + (int64_t)x * F;
    const uint8_t* cy = codes + (int64_t)y * F;
    int differing = 0;
    for (int f = 0; f < F; ++f) differing += cx[f] != cy[f];
    table[(int64_t)x * V + y] = (uint8_t)differing;
}

__global__ __launch_bounds__(WAVE) void edit_weighted_rows_kernel(EditWeightedArgs w) {
    const EditArgs& a = w.x.e;
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
    Row row;
    FeatureCosts costs;
    const int flag = open_row(w, r, o, n, k, lane, row, costs);
    if (flag < 0) {
        if (lane < 4) st[lane] = flag;
        return;
    }
    NoPath path;
    const int2 cell = carried_dp(row.A, row.m, row.B, row.nb, row.bnd0, row.bnd1, lane, costs, path);
    const int S = (int)((uint32_t)cell.y >> 16), D = cell.y & 0xffff;
    const int C = row.m - S - D;
    const int I = row.nb - C - S;
    if (lane < 4) st[lane] = lane == 0 ? I : lane == 1 ? D : lane == 2 ? S : C;
    if (lane == 0) w.costs[r] = as_float(cell.x);
}

__global__ __launch_bounds__(SELECT_THREADS) void edit_weighted_select_kernel(EditArgs a) { select_candidate(a); }

__global__ __launch_bounds__(WAVE) void edit_weighted_ops_kernel(EditWeightedArgs w) {
    const EditOpsArgs& x = w.x;
    const EditArgs& a = x.e;
    const int64_t r = blockIdx.x;  // o * N + n
    const int lane = threadIdx.x;
    const int n = (int)(r % a.N), o = (int)(r / a.N);
    if (a.hyp_counts && a.hyp_counts[r] <= 0) {
        if (lane == 0) x.operation_counts[r] = -1;
        return;
    }
    Row row;
    FeatureCosts costs;
    const int flag = open_row(w, r, o, n, 0, lane, row, costs);
    if (flag < 0) {
        if (lane == 0) x.operation_counts[r] = flag;
        return;
    }
    uint4* codes = reinterpret_cast<uint4*>(a.workspace + r * a.span + x.codes_at);
    PathCodes path{codes, x.code_stride, make_uint4(0, 0, 0, 0)};
    const int m = row.m, nb = row.nb;
    // (the sweep's last strip ends with a fence: the codes are visible)
    const int2 cell = carried_dp(row.A, m, row.B, nb, row.bnd0, row.bnd1, lane, costs, path);
    const int S = (int)((uint32_t)cell.y >> 16), D = cell.y & 0xffff;
    const int count = nb - m + 2 * D + S;  // S + D + I with I = n - (m - S - D) - S

    walk_operations(codes, x.code_stride, row.A, m, row.B, nb, count, x.operations + r * x.max_ops * 5, lane);
    if (lane == 0) x.operation_counts[r] = count, w.costs[r] = as_float(cell.x);
}

__global__ __launch_bounds__(WAVE) void edit_matrix_kernel(EditMatrixArgs a) {
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    const int ab = a.expected_offsets[r], ae = a.expected_offsets[r + 1];
    const int bb = a.actual_offsets[r], be = a.actual_offsets[r + 1];
    const int64_t m = (int64_t)ae - ab, n = (int64_t)be - bb;
    bool ok = ab >= 0 && bb >= 0 && m >= 0 && m <= a.cap_a && n >= 0 && n <= a.cap_b;
    const int32_t* A = a.expected_ids + ab;
    const int32_t* B = a.actual_ids + bb;
    if (ok && a.V > 0) ok = in_table(A, (int)m, a.V, lane) && in_table(B, (int)n, a.V, lane);
    if (lane == 0) a.status[r] = ok ? 0 : -2;
    if (!ok) return;
    FeatureCosts costs;
    costs.insertion = a.insertion_cost, costs.deletion = a.deletion_cost;
    costs.table = a.V > 0 ? a.table : nullptr;
    costs.V = a.V;
    costs.ld = a.cap_b + 1;
    costs.matrix = a.matrix + r * (a.cap_a + 1) * costs.ld;
    costs.rows = (int)m;
    costs.column = 0.f;
    for (int j = lane; j <= n; j += WAVE) costs.matrix[j] = costs.row0(j);
    int2* bnd0 = a.workspace + r * 2 * a.bnd_pad;
    NoPath path;
    carried_dp(A, (int)m, B, (int)n, bnd0, bnd0 + a.bnd_pad, lane, costs, path);
}

}  // namespace

void launch_edit_cost_table(const uint8_t* codes, int V, int F, uint8_t* table, hipStream_t s) {
    hipLaunchKernelGGL(edit_cost_table_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)V), dim3(256), 0, s, codes, V, F, table);
}

void launch_edit_weighted_statistics(EditWeightedArgs w, hipStream_t s) {
    EditArgs& a = w.x.e;
    edit_layout(a);
    const int64_t rows = (int64_t)a.O * a.N * a.K;
    hipLaunchKernelGGL(edit_weighted_rows_kernel, dim3((unsigned)rows), dim3(WAVE), 0, s, w);
    const int64_t pairs = (int64_t)a.O * a.N;
    hipLaunchKernelGGL(edit_weighted_select_kernel, dim3((unsigned)((pairs + SELECT_THREADS - 1) / SELECT_THREADS)),
                       dim3(SELECT_THREADS), 0, s, a);
}

void launch_edit_weighted_operations(EditWeightedArgs w, hipStream_t s) {
    edit_layout(w.x);
    const EditArgs& a = w.x.e;
    hipLaunchKernelGGL(edit_weighted_ops_kernel, dim3((unsigned)((int64_t)a.O * a.N)), dim3(WAVE), 0, s, w);
}

void launch_edit_matrix(EditMatrixArgs a, hipStream_t s) {
    a.bnd_pad = edit_pad(a.cap_b + 1);
    hipLaunchKernelGGL(edit_matrix_kernel, dim3((unsigned)a.rows), dim3(WAVE), 0, s, a);
}

}  // namespace amx
