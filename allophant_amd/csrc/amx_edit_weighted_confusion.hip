// Confusion tables on the paths of the feature-weighted costs (amx_edit_weighted_confusions; contract in
// include/allophant_amx_edit.h): amx_edit_confusion.hip's row under the FeatureCosts model of amx_edit_weighted.hip, which the
// two translation units share through amx_edit_feature_costs.inc.  The row is edit_weighted_ops_kernel's up to the walk, for
// candidate best[o, n] of K, then walk_confusions.  A pair whose table cost is 0 is a match of this path, so the tail below
// the walk's last operation holds pairs of cost 0, equal symbols or not.
#include "amx_common.h"
#include "../../include/allophant_amx_edit.h"

namespace amx {

namespace {

#include "amx_edit_dp.inc"
#include "amx_edit_feature_costs.inc"

__global__ __launch_bounds__(WAVE) void edit_weighted_confusion_kernel(EditWeightedConfusionArgs p) {
    const EditWeightedArgs& w = p.w;
    const EditOpsArgs& x = w.x;
    const EditArgs& a = x.e;
    const EditConfusionOut& c = p.c;
    const int64_t r = blockIdx.x;  // o * N + n
    const int lane = threadIdx.x;
    const int n = (int)(r % a.N), o = (int)(r / a.N);
    const auto flag_row = [&](int value) {
        if (lane == 0) c.row_events[r] = value;
    };
    const int k = confusion_candidate(a, c.best, r);
    if (k < 0) return flag_row(k);
    const int g = a.groups[n];
    const int length = a.counts[r * a.K + k];
    const int lb = a.label_offsets[n], le = a.label_offsets[n + 1];
    if (g < 0 || g >= a.G || length < 0 || length > a.T || lb < 0 || le < lb || (int64_t)a.G * a.O > CONFUSION_MAX_GROUPS)
        return flag_row(-2);
    int32_t* ws = a.workspace + r * a.span;
    int32_t* A = ws;
    int32_t* B = ws + a.cap_a_pad;
    int2* bnd0 = reinterpret_cast<int2*>(B + a.cap_b_pad);
    int2* bnd1 = bnd0 + a.bnd_pad;
    uint4* codes = reinterpret_cast<uint4*>(ws + x.codes_at);
    const int32_t* lmap = a.label_maps + 2 * o;
    const int32_t* hmap = a.hyp_maps + 2 * ((int64_t)(a.H > 1 ? g : 0) * a.O + o);
    const int m = expand(a.label_ids + lb, le - lb, a.map_offsets + lmap[0], a.map_values, lmap[1], A, a.cap_a, lane);
    const int64_t* tokens = a.tokens + o * a.stride_o + n * a.stride_n + k * a.stride_k;
    const int nb = m < 0 ? -1 : expand(tokens, length, a.map_offsets + hmap[0], a.map_values, hmap[1], B, a.cap_b, lane);
    if (m < 0 || nb < 0) return flag_row(-2);
    wave_fence();  // the expansions are read back by other lanes
    const int64_t first = w.tables[2 * o], V = w.tables[2 * o + 1];
    const int limit = V > 0 ? min((int)V - 1, CONFUSION_MAX_SYMBOL) : CONFUSION_MAX_SYMBOL;  // inside the table, and in a key
    if (!(symbols_within(A, m, limit, lane) && symbols_within(B, nb, limit, lane))) return flag_row(-2);
    ConfusionSink sink{c.table, (unsigned long long)c.capacity - 1,
                       (unsigned long long)((int64_t)g * a.O + o + 1) << (2 * CONFUSION_SYMBOL_BITS), 0, 0};
    int events;
    if (m == 0 || nb == 0) {
        events = pure_confusions(A, m, B, nb, sink, lane);
    } else {
        FeatureCosts costs;
        costs.insertion = w.insertion_cost, costs.deletion = w.deletion_cost;
        costs.table = V > 0 ? w.table_data + first : nullptr;
        costs.V = (int)V;
        costs.matrix = nullptr, costs.ld = 0, costs.rows = 0;
        costs.column = 0.f;
        PathCodes path{codes, x.code_stride, make_uint4(0, 0, 0, 0)};
        // (the sweep's last strip ends with a fence: the codes are visible)
        const int2 cell = carried_dp(A, m, B, nb, bnd0, bnd1, lane, costs, path);
        const int S = (int)((uint32_t)cell.y >> 16), D = cell.y & 0xffff;
        events = walk_confusions(codes, x.code_stride, A, m, B, nb, nb - m + 2 * D + S, sink, lane);  // S + D + I operations
    }
    sink.finish(c.counters, lane);
    if (lane == 0) c.row_events[r] = events;
}

}  // namespace

void launch_edit_weighted_confusions(EditWeightedConfusionArgs p, hipStream_t s) {
    edit_layout(p.w.x);
    const EditArgs& a = p.w.x.e;
    hipLaunchKernelGGL(edit_weighted_confusion_kernel, dim3((unsigned)((int64_t)a.O * a.N)), dim3(WAVE), 0, s, p);
}

}  // namespace amx
