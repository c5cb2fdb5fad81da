// Device helpers shared by amx_edit.hip (statistics) and amx_edit_ops.hip (operations): the CSR expansion of a row's ids and
// the anti-diagonal wavefront DP.  Included inside namespace amx { namespace { ... } }.
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

// The forward-carried DP of one row: expected A[0, m), actual B[0, n) (m, n <= 65535), boundary rows bnd0 / bnd1 of n + 1
// cells.  Returns (cost, S << 16 | D) of cell (m, n), identical in every lane.  After every wave step t of strip s, every lane
// calls path.step(s, t, last, diag, second, lane), `last` marking the strip's final step, with the move out of its cell (i, j)
// of the back-trace: the diagonal (`diag`; `second`: the symbols differ, a substitution), else a deletion (`second`) or an
// insertion.  Outside 1 <= j <= n both flags are false.
template <class Path>
__device__ int2 carried_dp(const int32_t* A, int m, const int32_t* B, int n, int2* bnd0, int2* bnd1, int lane, Path& path) {
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
            bool diag = false, second = false;
            if (j == 0) {  // column 0: i deletions
                cost = i, sd = i;
            } else if (j > 0 && j <= n) {
                const int ch = min(up_c, cost);  // deletion if strictly cheaper, else insertion
                const int nc = min(ch + 1, dg_c + (ai == bj ? 0 : 1));
                int nsd = up_c < cost ? up_sd + 1 : sd;
                if (dg_c <= ch) nsd = dg_sd + (dg_c != nc ? 0x10000 : 0);  // the diagonal; correct when its cost is ours
                diag = dg_c <= ch;
                second = diag ? ai != bj : up_c < cost;
                cost = nc;
                sd = nc == 0 ? 0 : nsd;  // the walk stops here: everything above is correct
            }
            path.step(s, t, t == n + last, diag, second, lane);
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
