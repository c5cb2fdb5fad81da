// Confusion tables of decoded hypotheses against labels: every aligned pair of the path that amx_edit_statistics counts and
// amx_edit_operations lists, matches included, added to a sparse table that lives on the device across a corpus; contract in
// include/allophant_amx_edit.h.
//
// One wave per (output, utterance) row, as edit_ops_kernel: the label and the chosen candidate's tokens are expanded, the
// wavefront DP (amx_edit_dp.inc) records the path codes, and walk_confusions follows them from (m, n), naming every move as
// an event (expected id or epsilon, actual id or epsilon).  Below the cell where upstream's walk stops (cost 0) every move is
// a match on the main diagonal, so those pairs are read straight from the two sequences.  A row with an empty side is m
// deletions or n insertions and runs no DP.
//
// The table is open-addressed over (key, count) slots of 64 bits each: the key's hash picks the first slot, linear probing
// the next, an empty slot is claimed by a compare-and-swap on its key, and the count grows by an integer atomic add.  Events
// are staged one per lane and inserted 64 at a time, so the atomics leave as whole wave instructions.  A probe sequence ends
// after `capacity` slots: an event without a slot is counted as dropped.  Counts are integer sums, the same in any order;
// which slot a key lands in depends on the order of arrival.
#include "amx_common.h"
#include "../../include/allophant_amx_edit.h"

namespace amx {

namespace {

#include "amx_edit_dp.inc"

__device__ __forceinline__ void flag_row(const EditConfusionOut& c, int64_t r, int value, int lane) {
    if (lane == 0) c.row_events[r] = value;
}

__global__ __launch_bounds__(WAVE) void edit_confusion_kernel(EditConfusionArgs p) {
    const EditOpsArgs& x = p.x;
    const EditArgs& a = x.e;
    const EditConfusionOut& c = p.c;
    const int64_t r = blockIdx.x;  // o * N + n
    const int lane = threadIdx.x;
    const int n = (int)(r % a.N), o = (int)(r / a.N);
    const int k = confusion_candidate(a, c.best, r);
    if (k < 0) return flag_row(c, r, k, lane);
    const int g = a.groups[n];
    const int length = a.counts[r * a.K + k];
    const int lb = a.label_offsets[n], le = a.label_offsets[n + 1];
    if (g < 0 || g >= a.G || length < 0 || length > a.T || lb < 0 || le < lb || (int64_t)a.G * a.O > CONFUSION_MAX_GROUPS)
        return flag_row(c, r, -2, lane);
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
    if (m < 0 || nb < 0) return flag_row(c, r, -2, lane);
    wave_fence();  // the expansions are read back by other lanes
    if (!(symbols_within(A, m, CONFUSION_MAX_SYMBOL, lane) && symbols_within(B, nb, CONFUSION_MAX_SYMBOL, lane)))
        return flag_row(c, r, -2, lane);
    ConfusionSink sink{c.table, (unsigned long long)c.capacity - 1,
                       (unsigned long long)((int64_t)g * a.O + o + 1) << (2 * CONFUSION_SYMBOL_BITS), 0, 0};
    int events;
    if (m == 0 || nb == 0) {
        events = pure_confusions(A, m, B, nb, sink, lane);
    } else {
        PathCodes path{codes, x.code_stride, make_uint4(0, 0, 0, 0)};
        const int cost = carried_dp(A, m, B, nb, bnd0, bnd1, lane, path).x;  // ends with a fence: the codes are visible
        events = walk_confusions(codes, x.code_stride, A, m, B, nb, cost, sink, lane);
    }
    sink.finish(c.counters, lane);
    if (lane == 0) c.row_events[r] = events;
}

constexpr int MERGE_THREADS = 256;

__global__ __launch_bounds__(MERGE_THREADS) void edit_confusion_merge_kernel(const unsigned long long* src, int64_t src_capacity,
                                                                            unsigned long long* dst, unsigned long long dst_mask,
                                                                            unsigned long long* counters) {
    const int64_t slot = (int64_t)blockIdx.x * MERGE_THREADS + threadIdx.x;
    unsigned long long added = 0, dropped = 0;
    if (slot < src_capacity) {
        const unsigned long long key = src[2 * slot], count = src[2 * slot + 1];
        if (key != 0 && count != 0) {
            if (confusion_insert(dst, dst_mask, key, count)) added = count;
            else dropped = count;
        }
    }
    added = wave_sum(added), dropped = wave_sum(dropped);
    if (threadIdx.x % WAVE == 0 && added) atomicAdd(counters, added);
    if (threadIdx.x % WAVE == 0 && dropped) atomicAdd(counters + 1, dropped);
}

}  // namespace

void launch_edit_confusions(EditConfusionArgs p, hipStream_t s) {
    edit_layout(p.x);
    const int64_t rows = (int64_t)p.x.e.O * p.x.e.N;
    hipLaunchKernelGGL(edit_confusion_kernel, dim3((unsigned)rows), dim3(WAVE), 0, s, p);
}

void launch_edit_confusion_merge(const unsigned long long* src, int64_t src_capacity, unsigned long long* dst,
                                 int64_t dst_capacity, unsigned long long* counters, hipStream_t s) {
    const int64_t blocks = (src_capacity + MERGE_THREADS - 1) / MERGE_THREADS;
    hipLaunchKernelGGL(edit_confusion_merge_kernel, dim3((unsigned)blocks), dim3(MERGE_THREADS), 0, s, src, src_capacity, dst,
                       (unsigned long long)dst_capacity - 1, counters);
}

}  // namespace amx
