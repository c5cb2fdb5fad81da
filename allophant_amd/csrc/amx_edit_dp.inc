// Device helpers shared by amx_edit.hip (statistics), amx_edit_ops.hip (operations), amx_edit_confusion.hip (confusion
// tables) and amx_edit_weighted.hip / amx_edit_weighted_confusion.hip (the three under feature-weighted costs): the CSR
// expansion of a row's ids, the
// anti-diagonal wavefront DP over a cost model, the path codes and the walks over them, the confusion table's insert, and
// the candidate choice.  Included inside namespace amx { namespace { ... } }.
//
// Lane l owns expected row i = 64 s + l + 1 of strip s and the wave sweeps the hypothesis as an anti-diagonal: at step t lane
// l computes column j = t - l, with the cell above and the diagonal arriving from lane l - 1 by a DPP wave shift.  Lane 0
// reads the strip's top boundary, and lane 63's cells become the next strip's, through two boundary rows in the workspace,
// staged 64 columns at a time in registers.

constexpr int WAVE = 64;

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

// The sweep's hook for the statistics: nothing recorded.
struct NoPath {
    __device__ void step(int, int, bool, bool, bool, int) {}
};

// The sweep's cost model.  UnitCosts is upstream's uniform_costs in integers: every operation 1, a substitution a != b.  A
// model names its cell type T (carried between lanes and through the boundary rows as 32 bits), how many wave steps ahead
// of its use a substitution cost is fetched (AHEAD: the sweep's inner loop is unrolled that many times), and:
//   row0(j), column0(i, lane)   the matrix's first row and column (column0 is called once per strip, in strip order)
//   begin_strip / stage / fetch the substitution cost of the cell a lane reaches at this step (fetch's first argument is the unrolled slot)
//   next                        the cell's cost from its three predecessors
//   substituted                 whether a diagonal move is a substitution rather than a match
//   cell                        sees every cell (i, j) of columns 0 .. n with its cost
struct UnitCosts {
    typedef int T;
    static constexpr int AHEAD = 1;
    __device__ static int bits(int v) { return v; }
    __device__ static int value(int b) { return b; }
    __device__ int row0(int j) const { return j; }
    __device__ int column0(int i, int) { return i; }
    __device__ void begin_strip(int, const int32_t*, int, int) {}
    __device__ void stage(const int32_t*, int, int) {}
    __device__ int fetch(int, int, int ai, int bj) { return ai == bj ? 0 : 1; }
    __device__ int next(int, int, int chosen, int dg, int sub) const { return min(chosen + 1, dg + sub); }
    __device__ bool substituted(int sub, int, int) const { return sub != 0; }
    __device__ void cell(int, int, int) {}
};

// The forward-carried DP of one row: expected A[0, m), actual B[0, n) (m, n <= 65535), boundary rows bnd0 / bnd1 of n + 1
// cells.  Returns (cost as 32 bits, S << 16 | D) of cell (m, n), identical in every lane.  After every wave step t of strip s,
// every lane calls path.step(s, t, last, diag, second, lane), `last` marking the strip's final step, with the move out of its
// cell (i, j) of the back-trace: the diagonal (`diag`; `second`: a substitution), else a deletion (`second`) or an insertion.
// Outside 1 <= j <= n both flags are false.
template <class Costs, class Path>
__device__ int2 carried_dp(const int32_t* A, int m, const int32_t* B, int n, int2* bnd0, int2* bnd1, int lane, Costs& costs,
                           Path& path) {
    typedef typename Costs::T T;
    if (m == 0) return make_int2(Costs::bits(costs.row0(n)), 0);
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
        const T first = costs.column0(i, lane);
        costs.begin_strip(ai, B, n, lane);
        T cost = 0, up_c = 0;
        int sd = 0, up_sd = 0, bj = 0;
        int in_c = 0, in_sd = 0, in_b = 0, out_c = 0, out_sd = 0;
        // one wave step; `u` is the step's slot in the cost model's unrolled window
        auto step = [&](int t, int u) __attribute__((always_inline)) {
            const int c = t & (WAVE - 1);
            if (c == 0) {  // the next 64 columns of lane 0's inputs
                const int col = t + lane;
                if (top) {
                    in_c = Costs::bits(costs.row0(col)), in_sd = 0;  // row 0: j insertions
                } else if (col <= n) {
                    const int2 v = bin[col];
                    in_c = v.x, in_sd = v.y;
                }
                const int bi = col - 1;
                in_b = bi >= 0 && bi < n ? B[bi] : -1;
                costs.stage(B, n, col);
            }
            const T dg_c = up_c;
            const int dg_sd = up_sd;
            up_c = Costs::value(shift_in(lane_value(in_c, c), Costs::bits(cost)));
            up_sd = shift_in(lane_value(in_sd, c), sd);
            bj = shift_in(lane_value(in_b, c), bj);
            const T sub = costs.fetch(u, c, ai, bj);
            const int j = t - lane;
            bool diag = false, second = false;
            if (j == 0) {  // column 0: i deletions
                cost = first, sd = i;
                costs.cell(i, 0, cost);
            } else if (j > 0 && j <= n) {
                const T ch = min(up_c, cost);  // deletion if strictly cheaper, else insertion
                const T nc = costs.next(up_c, cost, ch, dg_c, sub);
                int nsd = up_c < cost ? up_sd + 1 : sd;
                if (dg_c <= ch) nsd = dg_sd + (dg_c != nc ? 0x10000 : 0);  // the diagonal; correct when its cost is ours
                diag = dg_c <= ch;
                second = diag ? costs.substituted(sub, dg_c, nc) : up_c < cost;
                cost = nc;
                sd = nc == 0 ? 0 : nsd;  // the walk stops here: everything above is correct
                costs.cell(i, j, cost);
            }
            path.step(s, t, t == n + last, diag, second, lane);
            if (hand_on) {  // lane 63's cell (i0 + 64, t - 63) goes to the next strip's top boundary
                const int jo = t - (WAVE - 1);
                if (jo >= 0 && jo <= n) {
                    const int vc = lane_value(Costs::bits(cost), WAVE - 1), vs = lane_value(sd, WAVE - 1);
                    if (lane == (jo & (WAVE - 1))) out_c = vc, out_sd = vs;
                    if ((jo & (WAVE - 1)) == WAVE - 1 || jo == n) {
                        const int col = (jo & ~(WAVE - 1)) + lane;
                        if (col <= jo) bout[col] = make_int2(out_c, out_sd);
                    }
                }
            }
        };
        if constexpr (Costs::AHEAD == 1) {  // (one plain loop: the compiler specialises it per strip kind)
            for (int t = 0; t <= n + last; ++t) step(t, 0);
        } else {
            for (int t0 = 0; t0 <= n + last; t0 += Costs::AHEAD) {
#pragma unroll
                for (int u = 0; u < Costs::AHEAD; ++u)
                    if (t0 + u <= n + last) step(t0 + u, u);
            }
        }
        if (!hand_on) result = make_int2(lane_value(Costs::bits(cost), last), lane_value(sd, last));
        int2* swap = bin;
        bin = bout;
        bout = swap;
        wave_fence();
    }
    return result;
}

// The uniform sweep: (cost, S << 16 | D) of cell (m, n).
template <class Path>
__device__ int2 carried_dp(const int32_t* A, int m, const int32_t* B, int n, int2* bnd0, int2* bnd1, int lane, Path& path) {
    UnitCosts costs;
    return carried_dp(A, m, B, n, bnd0, bnd1, lane, costs, path);
}

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

// The back-trace over the recorded codes of one row, from (m, n): `count` operations (what upstream's walk records before it
// reaches a cost of 0), operation k in walk order written as the record (action, i, j, expected id, actual id) at
// out[count - 1 - k]: upstream's reversed list, with no reversal pass.  Wave-uniform; records are staged one per lane and
// written 64 at a time, with their symbol ids read in parallel.
__device__ __forceinline__ void walk_operations(const uint4* codes, int64_t stride, const int32_t* A, int m, const int32_t* B,
                                                int nb, int count, int32_t* out, int lane) {
    int i = m, j = nb, k = 0, written = 0;
    int win_s = -1, win_t = 0;  // the loaded window: strip win_s, steps [win_t, win_t + 64)
    uint4 w = make_uint4(0, 0, 0, 0);
    int rec_act = 0, rec_i = 0, rec_j = 0;  // lane q stages operation written + q
    while (k < count && (i > 0 || j > 0)) {  // (the origin is never reached first; the guard keeps every index in range)
        int act = 0;  // 0: a match, recorded as nothing
        if (i == 0) {
            act = AMX_EDIT_INSERTION, --j;
        } else if (j == 0) {
            act = AMX_EDIT_DELETION, --i;
        } else {
            const int s = (i - 1) / WAVE, l = (i - 1) % WAVE, t = j + l;
            if (s != win_s || t < win_t) {
                win_s = s, win_t = max(0, t - (WAVE - 1));
                w = codes[s * stride + win_t + lane];  // win_t + 63 <= max(t, 63) < code_stride
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
        if (k - written == WAVE || k == count) {
            const int q = written + lane;
            if (q < k) {
                int32_t* rec = out + (int64_t)(count - 1 - q) * 5;
                rec[0] = rec_act, rec[1] = rec_i, rec[2] = rec_j;
                rec[3] = rec_act != AMX_EDIT_INSERTION ? A[rec_i] : -1;
                rec[4] = rec_act != AMX_EDIT_DELETION ? B[rec_j] : -1;
            }
            written = k;
        }
    }
}

// Confusion tables (amx_edit_confusions and its siblings): an open-addressed table of (key, count) slots of 64 bits each, key 0
// empty.  A key packs (g * O + o + 1, expected id + 1, actual id + 1), epsilon as 0, in GROUP / SYMBOL / SYMBOL bits.
constexpr int CONFUSION_SYMBOL_BITS = AMX_EDIT_CONFUSION_SYMBOL_BITS;
constexpr int CONFUSION_MAX_GROUPS = (1 << AMX_EDIT_CONFUSION_GROUP_BITS) - 1;  // G * O
constexpr int CONFUSION_MAX_SYMBOL = (1 << CONFUSION_SYMBOL_BITS) - 2;           // the largest id

// Adds `count` to `key`'s slot of table[0, mask + 1): linear probing from the key's hash, an empty slot claimed by a
// compare-and-swap on its key.  At most mask + 1 probes: false when every slot holds another key.
__device__ __forceinline__ bool confusion_insert(unsigned long long* table, unsigned long long mask, unsigned long long key,
                                                 unsigned long long count) {
    unsigned long long h = key;
    h ^= h >> 30, h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27, h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    h &= mask;
    for (unsigned long long probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
        unsigned long long* slot = table + 2 * h;
        unsigned long long held = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (held == 0) {
            held = atomicCAS(slot, 0ull, key);
            if (held == 0) held = key;
        }
        if (held == key) {
            atomicAdd(slot + 1, count);
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;  // lane 0's
}

// One row's events on their way into the table: every lane adds its own staged event, so a wave issues up to 64 atomics at
// a time; `finish` adds the row's added / dropped events to counters[0 / 1] with one atomic each.
struct ConfusionSink {
    unsigned long long* table;
    unsigned long long mask;    // capacity - 1
    unsigned long long prefix;  // (g * O + o + 1) << (2 * CONFUSION_SYMBOL_BITS)
    unsigned int added, dropped;  // this lane's
    __device__ __forceinline__ void add(int expected, int actual) {  // symbol ids, -1: epsilon
        const unsigned long long key =
            prefix | (unsigned long long)(expected + 1) << CONFUSION_SYMBOL_BITS | (unsigned long long)(actual + 1);
        if (confusion_insert(table, mask, key, 1)) ++added;
        else ++dropped;
    }
    __device__ __forceinline__ void finish(unsigned long long* counters, int lane) {
        const unsigned long long a = wave_sum(added), d = wave_sum(dropped);
        if (lane == 0 && a) atomicAdd(counters, a);
        if (lane == 0 && d) atomicAdd(counters + 1, d);
    }
};

// Every id of ids[0, count) in [0, limit]?  (wave-uniform answer)
__device__ __forceinline__ bool symbols_within(const int32_t* ids, int count, int limit, int lane) {
    bool bad = false;
    for (int base = 0; base < count; base += WAVE) {
        const int idx = base + lane;
        if (idx < count) bad |= ids[idx] < 0 || ids[idx] > limit;
    }
    return !__any(bad);
}

// The candidate a confusion row walks: best[on] where `best` is given, else candidate 0.  -1: no candidate (none present, or
// best == -1); -2: flagged (best == -2, or a best at or past the candidates present).
__device__ __forceinline__ int confusion_candidate(const EditArgs& a, const int32_t* best, int64_t on) {
    const int present = a.hyp_counts ? min(max(a.hyp_counts[on], 0), a.K) : a.K;
    if (!best) return present > 0 ? 0 : -1;
    const int k = best[on];
    if (k < 0) return k == -1 ? -1 : -2;
    return k < present ? k : -2;
}

// A row with an empty side: m deletions or n insertions (or nothing), 64 per step.  Returns the number of events.
__device__ __forceinline__ int pure_confusions(const int32_t* A, int m, const int32_t* B, int nb, ConfusionSink& sink, int lane) {
    for (int q = lane; q < m; q += WAVE) sink.add(A[q], -1);
    for (int q = lane; q < nb; q += WAVE) sink.add(-1, B[q]);
    return m + nb;
}

// The back-trace of walk_operations with every move an event (expected id, actual id): a diagonal move names both symbols,
// match or substitution alike, a deletion (A[i], epsilon), an insertion (epsilon, B[j]).  `count` is the number of
// operations, as there: after them the walk stands on a cell of cost 0, where i == j and everything below is diagonal, so the
// pairs (A[q], B[q]), q < i, follow without code words, 64 per step.  Wave-uniform; events are staged one per lane and added
// 64 at a time.  Returns the number of events, m + n - #diagonal.
__device__ __forceinline__ int walk_confusions(const uint4* codes, int64_t stride, const int32_t* A, int m, const int32_t* B,
                                               int nb, int count, ConfusionSink& sink, int lane) {
    int i = m, j = nb, k = 0, events = 0, added = 0;
    int win_s = -1, win_t = 0;  // the loaded window: strip win_s, steps [win_t, win_t + 64)
    uint4 w = make_uint4(0, 0, 0, 0);
    int ev_i = -1, ev_j = -1;  // lane q stages event added + q: its indices into A and B, -1 for epsilon
    while (k < count && (i > 0 || j > 0)) {
        int act = 0;  // 0: a match
        if (i == 0) {
            act = AMX_EDIT_INSERTION, --j;
        } else if (j == 0) {
            act = AMX_EDIT_DELETION, --i;
        } else {
            const int s = (i - 1) / WAVE, l = (i - 1) % WAVE, t = j + l;
            if (s != win_s || t < win_t) {
                win_s = s, win_t = max(0, t - (WAVE - 1));
                w = codes[s * stride + win_t + lane];  // win_t + 63 <= max(t, 63) < code_stride
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
        if (lane == events - added) {  // the coordinates after the move
            ev_i = act != AMX_EDIT_INSERTION ? i : -1;
            ev_j = act != AMX_EDIT_DELETION ? j : -1;
        }
        ++events;
        if (act != 0) ++k;
        if (events - added == WAVE) {
            sink.add(ev_i >= 0 ? A[ev_i] : -1, ev_j >= 0 ? B[ev_j] : -1);
            added = events;
        }
    }
    if (lane < events - added) sink.add(ev_i >= 0 ? A[ev_i] : -1, ev_j >= 0 ? B[ev_j] : -1);
    const int tail = min(i, j);  // (equal wherever the loop ends)
    for (int q = lane; q < tail; q += WAVE) sink.add(A[q], B[q]);
    return events + tail;
}

// The candidate choice, one thread per (output, utterance) in blocks of SELECT_THREADS: the first candidate of strictly
// lowest fp32 word_error_rate, then its counts added to its group's totals.
constexpr int SELECT_THREADS = 256;

__device__ __forceinline__ void select_candidate(const EditArgs& a) {
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
