// The feature-weighted cost model of carried_dp (amx_edit_dp.inc), shared by amx_edit_weighted.hip (statistics, operations,
// matrix) and amx_edit_weighted_confusion.hip (confusion tables).  Included after amx_edit_dp.inc, inside
// namespace amx { namespace { ... } }.  See the head of amx_edit_weighted.hip for the gather's pipeline.

__device__ __forceinline__ float as_float(int v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ int as_bits(float v) { return __builtin_bit_cast(int, v); }

struct FeatureCosts {
    typedef float T;
    static constexpr int AHEAD = 8;
    float insertion, deletion;
    const uint8_t* table;  // [V, V], or null: a != b
    int V;
    float* matrix;  // cell (i, j), i <= rows, at matrix[i * ld + j]; or null
    int64_t ld;
    int rows;
    float column;            // M[64 s][0] of the strip about to start
    const uint8_t* row;      // table + a_i * V
    int ai;
    int ahead_b, staged_b;   // the symbol of column t + AHEAD - lane; lane 0's next 64 inputs of that pipeline
    int queue[AHEAD];        // slot u: the substitution cost of the cell reached at the next step t = u (mod AHEAD)

    __device__ __forceinline__ static int bits(float v) { return as_bits(v); }
    __device__ __forceinline__ static float value(int b) { return as_float(b); }
    __device__ __forceinline__ float row0(int j) const { return (float)j; }  // one per insertion, whatever insertion_cost is
    __device__ __forceinline__ float column0(int, int lane) {
        float v = column, mine = 0.f;
        for (int q = 0; q < WAVE; ++q) {  // M[i][0] = M[i - 1][0] + deletion_cost, rounded each time
            v += deletion;
            if (lane == q) mine = v;
        }
        column = v;
        return mine;
    }
    __device__ __forceinline__ int lookup(int b) const {
        if (ai < 0 || b < 0) return 0;
        return table ? (int)row[b] : (ai != b ? 1 : 0);
    }
    // column j's symbol, -1 outside 1 .. n
    __device__ __forceinline__ static int symbol(const int32_t* B, int n, int j) { return j >= 1 && j <= n ? B[j - 1] : -1; }
    __device__ __forceinline__ void begin_strip(int a, const int32_t* B, int n, int lane) {
        ai = a;
        row = table + (int64_t)max(a, 0) * V;
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) queue[u] = lookup(symbol(B, n, u - lane));
        ahead_b = symbol(B, n, AHEAD - 1 - lane);
    }
    __device__ __forceinline__ void stage(const int32_t* B, int n, int col) { staged_b = symbol(B, n, col + AHEAD); }
    __device__ __forceinline__ float fetch(int u, int c, int, int) {
        const int d = queue[u];
        ahead_b = shift_in(lane_value(staged_b, c), ahead_b);
        queue[u] = lookup(ahead_b);
        return (float)d;
    }
    __device__ __forceinline__ float next(float up, float left, float, float dg, float sub) const {
        return fminf(fminf(left + insertion, up + deletion), dg + sub);
    }
    __device__ __forceinline__ bool substituted(float, float dg, float cost) const { return dg != cost; }
    __device__ __forceinline__ void cell(int i, int j, float cost) {
        if (matrix && i <= rows) matrix[i * ld + j] = cost;
    }
};
