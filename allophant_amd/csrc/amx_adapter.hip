// The attention adapter of an MMS encoder layer (transformers Wav2Vec2AttnAdapterLayer behind the FFN residual of
// Wav2Vec2EncoderLayerStableLayerNorm, config.adapter_attn_dim = A):
//
//     h' = h + W2 relu(W1 LN_a(h) + b1) + b2
//
// one launch per layer, in place on the fp32 residual rows; for every layer but the last the same launch also writes the planes
// of the LayerNorm (without affine part) of h' -- the A operand of the next layer's QKV product -- so that the row pass at the top
// of that layer is not launched.  A row is read once (4 bytes per element), written back (4) and written as planes (4).
//
// Layout: a workgroup of ceil(D / 256) waves works on TWO rows at a time, thread t owning the four columns 4 t .. 4 t + 3 of both
// (the unit of the plane writer, store_planes4), and walks the row pairs blockIdx.x, blockIdx.x + gridDim.x, ...  The weights of a
// thread's four columns -- W1' [A, 4] and W2 [4, A] -- are loaded ONCE into registers (8 A of them: 128 at A = 16) and stay there
// across the rows the workgroup walks: at D = 1280, A = 16 the two matrices are 164 KB in fp32, more than the 160 KiB of a CU's LDS,
// and re-read per row they would be 40 times the traffic of the rows themselves.  Adapter widths beyond ADAPTER_REG_DIM have no
// room in the register file (8 A registers per thread) and read the weights through the cache per row pair: correct for every
// A <= 64, not tuned.  The row statistics go wave-wise over the DPP network and through LDS; the A partial sums of the first
// product are reduce-scattered over each row of 16 lanes (DPP) and the 4 x waves totals added up in a fixed order behind a barrier: no
// atomics, the same bits whatever the grid.  With 215 registers a CU holds one workgroup of five waves, so what the kernel waits
// for is its own chain of reductions and barriers (six per iteration); two rows per iteration share that chain.  fp32 FMAs
// throughout: 4 A D flop per row is a fiftieth of the layer's products, and the adapter's input and output are the fp32 stream.
#include "amx_common.h"

namespace amx {

namespace {

constexpr int ADAPTER_REG_DIM = 16;   // adapter widths up to this keep their weights in registers
constexpr int ADAPTER_MAX_WAVES = 8;   // D <= 2048: 512 threads of four columns
constexpr int ADAPTER_ROWS = 2;        // rows a workgroup works on at a time: their reductions share the barriers and overlap
constexpr int ADAPTER_PART_LD = ADAPTER_MAX_DIM + 1;  // (odd row stride: the four row-of-16 totals of a wave land in four banks)

__device__ __forceinline__ float sum4(float4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ float4 minus(float4 v, float m) { return make_float4(v.x - m, v.y - m, v.z - m, v.w - m); }
// One level of a reduce-scatter over a row of 16 lanes: v[0 .. 2 HALF) -> v[0 .. HALF), every lane adding to the half it keeps
// (the upper one where `upper`) what its partner under the DPP pattern CTRL sends of that same half.
template <int CTRL, int HALF>
__device__ __forceinline__ void scatter_level(float* v, bool upper) {
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float keep = upper ? v[i + HALF] : v[i];
        const float send = upper ? v[i] : v[i + HALF];
        v[i] = keep + dpp_move<CTRL>(send);
    }
}
// 32 values per lane -> their totals over each row of 16 lanes, two per lane: v[0], v[1] end up as the totals of the values
// row16_slot(lane) and row16_slot(lane) + 1.  31 additions per lane instead of the 128 of 32 all-lane butterflies (wave_sum's
// patterns: lane ^ 1, lane ^ 2, 7 - lane within 8, 15 - lane within 16).  The half a lane keeps at a level is chosen so that both
// partners of every LATER level hold the same values: the mirrors flip the low lane bits too, hence the parities below.
__device__ __forceinline__ void row16_reduce_scatter32(float* v, int lane) {
    const int b0 = lane & 1, b1 = (lane >> 1) & 1, b2 = (lane >> 2) & 1, b3 = (lane >> 3) & 1;
    scatter_level<0xB1, 16>(v, (b0 ^ b2) != 0);   // partner lane ^ 1
    scatter_level<0x4E, 8>(v, (b1 ^ b2) != 0);    // partner lane ^ 2
    scatter_level<0x141, 4>(v, (b2 ^ b3) != 0);   // partner 7 - lane within the row's halves
    scatter_level<0x140, 2>(v, b3 != 0);          // partner 15 - lane
}
__device__ __forceinline__ int row16_slot(int lane) {
    const int b0 = lane & 1, b1 = (lane >> 1) & 1, b2 = (lane >> 2) & 1, b3 = (lane >> 3) & 1;
    return 16 * (b0 ^ b2) + 8 * (b1 ^ b2) + 4 * (b2 ^ b3) + 2 * b3;
}

// blockDim.x = 64 * ceil(D / 256); every thread stays in the row loop (the reductions read whole waves), threads whose columns lie
// beyond D contribute zeros and store nothing, and so does a row beyond M (the second of the last pair when M is odd).  h carries
// no __restrict__: rows are updated in place (a row belongs to one workgroup, which holds it in registers between load and store).
// LDS slots are written once per iteration and read behind the next barrier; an iteration has at least four barriers, so a slot is
// never rewritten while a slower wave still reads it.
template <typename T, int NT, bool REG>
__global__ __launch_bounds__(64 * ADAPTER_MAX_WAVES) void adapter_kernel(float* h, int64_t M, int D, int A,
                                                                        const float* __restrict__ w1, const float* __restrict__ b1,
                                                                        const float* __restrict__ w2t, const float* __restrict__ b2,
                                                                        float eps_a, float eps, T* __restrict__ out_p, int64_t out_plane) {
    constexpr int G = ADAPTER_REG_DIM, R = ADAPTER_ROWS;
    __shared__ float red[4][R][ADAPTER_MAX_WAVES];
    __shared__ float part[R][4 * ADAPTER_MAX_WAVES][ADAPTER_PART_LD];  // [row][wave, row of 16 lanes][a]
    __shared__ float hid[R][ADAPTER_MAX_DIM];
    __shared__ float bias1[ADAPTER_MAX_DIM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int c = (int)threadIdx.x * 4;
    const bool live = c < D;
    const float invD = 1.0f / (float)D;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 w1r[REG ? G : 1], w2r[REG ? G : 1];
    if (REG) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const bool on = live && j < A;
            w1r[j] = on ? *(const float4*)(w1 + (int64_t)j * D + c) : zero4;
            w2r[j] = on ? *(const float4*)(w2t + (int64_t)j * D + c) : zero4;
        }
    }
    const float4 bias2 = live ? *(const float4*)(b2 + c) : zero4;
    if ((int)threadIdx.x < A) bias1[threadIdx.x] = b1[threadIdx.x];  // (read behind the barriers of the first iteration)
    auto load_row = [&](int64_t row) { return live && row < M ? *(const float4*)(h + row * D + c) : zero4; };
    auto total = [&](const float* slot) {  // wave totals in wave order: the same bits in every thread
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += slot[w];
        return s;
    };
    const int64_t pairs = (M + R - 1) / R;
    int64_t pair = blockIdx.x;
    float4 xn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) xn[r] = load_row(pair * R + r);
    for (; pair < pairs; pair += gridDim.x) {
        const int64_t row0 = pair * R;
        float4 x[R], d[R], y[R];
        float rs[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            x[r] = xn[r];
            xn[r] = load_row((pair + gridDim.x) * R + r);  // the next rows' loads fly under these rows' arithmetic
        }
        // LN_a without its affine part: exact two-pass statistics, like rownorm_kernel
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float s = wave_sum(sum4(x[r]));
            if (lane == 0) red[0][r][wave] = s;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            d[r] = live ? minus(x[r], total(red[0][r]) * invD) : zero4;
            const float q = wave_sum(dot4(d[r], d[r]));
            if (lane == 0) red[1][r][wave] = q;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) rs[r] = 1.0f / sqrtf(total(red[1][r]) * invD + eps_a);
        // first product: this thread's share of (h - mu) . W1'[a, :] for 16 values of a and both rows, summed over each row of 16
        // lanes; the totals of the 4 * nw rows of lanes are added up, and the row's rstd applied, behind the barrier
        static_assert(R * G == 32, "row16_reduce_scatter32 takes 32 values: 2 rows x 16 adapter columns");
        const int slot = row16_slot(lane), lanes16 = wave * 4 + (lane >> 4);
        for (int a0 = 0; a0 < A; a0 += G) {
            float v[R * G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                float4 w = zero4;
                if (REG) w = w1r[REG ? j : 0];  // (zeros beyond A)
                else if (live && a0 + j < A) w = *(const float4*)(w1 + (int64_t)(a0 + j) * D + c);
#pragma unroll
                for (int r = 0; r < R; ++r) v[r * G + j] = dot4(d[r], w);
            }
            row16_reduce_scatter32(v, lane);
            // (value r * 16 + j is row r, column a0 + j; columns A .. a0 + 15 are zeros that nothing reads)
            part[slot >> 4][lanes16][a0 + (slot & 15)] = v[0];
            part[slot >> 4][lanes16][a0 + (slot & 15) + 1] = v[1];
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < R * A; idx += blockDim.x) {
            const int r = idx / A, a = idx - r * A;
            float sum = 0.f, rstd = rs[0];
#pragma unroll
            for (int k = 1; k < R; ++k) rstd = r == k ? rs[k] : rstd;
            for (int k = 0; k < 4 * nw; ++k) sum += part[r][k][a];
            hid[r][a] = fmaxf(fmaf(rstd, sum, bias1[a]), 0.f);
        }
        __syncthreads();
        // second product and the residual
#pragma unroll
        for (int r = 0; r < R; ++r) y[r] = make_float4(x[r].x + bias2.x, x[r].y + bias2.y, x[r].z + bias2.z, x[r].w + bias2.w);
        for (int a0 = 0; a0 < A; a0 += G) {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int a = a0 + j;
                if (a < A) {
                    const float4 w = REG ? w2r[REG ? j : 0] : (live ? *(const float4*)(w2t + (int64_t)a * D + c) : zero4);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float hv = hid[r][a];
                        y[r].x = fmaf(hv, w.x, y[r].x);
                        y[r].y = fmaf(hv, w.y, y[r].y);
                        y[r].z = fmaf(hv, w.z, y[r].z);
                        y[r].w = fmaf(hv, w.w, y[r].w);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (live && row0 + r < M) *(float4*)(h + (row0 + r) * D + c) = y[r];
        if (out_p) {
            // the next layer's first LayerNorm (gamma / beta live in its QKV weights): planes of (h' - mu) * rstd
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float s = wave_sum(live ? sum4(y[r]) : 0.f);
                if (lane == 0) red[2][r][wave] = s;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                d[r] = live ? minus(y[r], total(red[2][r]) * invD) : zero4;
                const float q = wave_sum(dot4(d[r], d[r]));
                if (lane == 0) red[3][r][wave] = q;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float rs2 = 1.0f / sqrtf(total(red[3][r]) * invD + eps);
                if (live && row0 + r < M)
                    store_planes4<T, NT>(out_p, out_plane, (row0 + r) * D + c, make_float4(d[r].x * rs2, d[r].y * rs2, d[r].z * rs2, d[r].w * rs2));
            }
        }
    }
}

int adapter_cus() {
    static int per_device[MAX_DEVICES] = {};
    int& cus = per_device[current_device()];
    if (!cus) {
        hipDeviceProp_t prop;
        cus = hipGetDeviceProperties(&prop, current_device()) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return cus;
}

}  // namespace

void launch_adapter(int prec, float* h, int64_t M, int D, int A, const float* w1, const float* b1, const float* w2t, const float* b2,
                    float eps, void* out_p, int64_t out_plane, hipStream_t s) {
    if (M <= 0) return;
    const int nw = (D + 255) / 256;
    // persistent workgroups: as many as the register file keeps resident (two waves per SIMD with the weights in registers)
    const int64_t resident = (int64_t)adapter_cus() * std::max(1, 8 / nw);
    const dim3 grid((unsigned)std::min<int64_t>((M + ADAPTER_ROWS - 1) / ADAPTER_ROWS, resident)), block(64 * nw);
    if (A <= ADAPTER_REG_DIM) {
        AMX_DISPATCH(prec, hipLaunchKernelGGL((adapter_kernel<T16, NT, true>), grid, block, 0, s, h, M, D, A, w1, b1, w2t, b2,
                                              ADAPTER_LN_EPS, eps, (T16*)out_p, out_plane));
    } else {
        AMX_DISPATCH(prec, hipLaunchKernelGGL((adapter_kernel<T16, NT, false>), grid, block, 0, s, h, M, D, A, w1, b1, w2t, b2,
                                              ADAPTER_LN_EPS, eps, (T16*)out_p, out_plane));
    }
}

}  // namespace amx
