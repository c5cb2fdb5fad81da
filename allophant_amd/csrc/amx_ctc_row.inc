// Device and launch helpers shared by amx_ctc_align.hip and amx_ctc_score.hip, which run one workgroup per row of a CtcRows
// (amx_common.h): opening a row (its emissions, frame length and validated targets) and the choice of the kernel by strips per
// wave.  Included inside namespace amx { namespace { ... } }.

// One opened row: the emissions lp[t][c] at lp[t * st + c], `len` frames, the L targets y.
struct CtcRow {
    const float* lp;
    int64_t st;
    int C, blank, len, L;
    const int32_t* y;
};

// Opens row r, which reads utterance n (of output block `block` when the rows have `descs`).  Block-wide: false, for every
// thread alike, when the row is malformed (the caller reports status -2).  (`a` by value: by reference the kernels'
// register allocation changes.)
__device__ __forceinline__ bool ctc_open_row(const CtcRows a, int64_t r, int64_t n, int64_t block, CtcRow& row) {
    if (a.descs) {
        const OutDesc d = a.descs[block];
        row.lp = a.emissions + (int64_t)a.T * a.N * d.prefix + n * d.C;
        row.st = (int64_t)a.N * d.C, row.C = d.C, row.blank = 0;
    } else {
        row.lp = a.emissions + n * a.stride_n;
        row.st = a.stride_t, row.C = a.C, row.blank = a.blank;
    }
    row.len = a.frame_lengths[n];
    const int lb = a.target_offsets[r], le = a.target_offsets[r + 1], id_count = a.target_offsets[a.rows];
    const bool malformed = row.len < 0 || row.len > a.T || lb < 0 || le < lb || le > id_count || le - lb > a.max_target;
    row.L = malformed ? 0 : le - lb;
    row.y = a.target_ids + lb;
    int wrong = 0;
    for (int l = threadIdx.x; l < row.L; l += blockDim.x) {
        const int v = row.y[l];
        wrong |= v < 0 || v >= row.C || v == row.blank;
    }
    return !__syncthreads_or(malformed || wrong);
}

// Launches one workgroup per row with two LDS rows of strips * 64 states: wave w owns strips w, w + waves, ..., and the kernel
// is the one instantiated for that many strips per wave (1, 2, 4 or 8).
template <typename Args>
void ctc_launch_rows(const Args& a, hipStream_t s, void (*k1)(Args), void (*k2)(Args), void (*k4)(Args), void (*k8)(Args)) {
    const int waves = min(ALIGN_MAX_WAVES, a.strips);
    const int per_wave = (a.strips + waves - 1) / waves;
    void (*kernel)(Args) = per_wave <= 1 ? k1 : per_wave <= 2 ? k2 : per_wave <= 4 ? k4 : k8;
    const size_t lds = (size_t)a.strips * CTC_WAVE * 2 * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.rows), dim3(waves * CTC_WAVE), lds, s, a);
}
