// Band-limited sinc resampling: torchaudio's `functional.resample(..., resampling_method="sinc_interp_hann")`, which upstream
// runs on every utterance before `Estimator.predict` (include/allophant_amx_resample.h states the contract).
//
//   y[f * m + j] = sum_k bank[k * m + j] * x[f * o + first_j + k - W]
//
// The bank is built on the host in float64 and rounded to fp32 once (resample_bank); each phase keeps the contiguous run of
// taps whose unclamped window argument lies inside (-lpw, lpw) and is padded with zeros to the longest run K, so every
// output runs the same K fp32 FMAs in the same order, whatever the batch around it.  The bank is stored tap-major: the 64
// lanes of a wave own consecutive outputs, hence consecutive phases, and read consecutive bank words per tap.
#include "../../include/allophant_amx_resample.h"
#include "amx_common.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace amx {

namespace {

constexpr int RS_THREADS = 256;

__device__ __forceinline__ void fill_tile(float* dst, int tile, float v) {
    for (int u = threadIdx.x; u < tile; u += RS_THREADS) dst[u] = v;
}

// grid (ceil(L_out / RS_TILE), N): one workgroup = RS_TILE consecutive output samples of one utterance.  The input window of
// the tile's frames, [f0 * o + first_0 - W, f1 * o + first_{m-1} + K - W), is staged in LDS with loads masked by the row's
// length (zeros outside [0, len)); outputs at or past len' are written 0.
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const float* __restrict__ x, int64_t stride, int64_t L_in,
                                                              const int64_t* __restrict__ lengths,
                                                              const amx_resample_row* __restrict__ rows,
                                                              const float* __restrict__ bank, const int32_t* __restrict__ phases,
                                                              int window, int64_t L_out, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int n = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * RS_TILE;
    const int tile = (int)min((int64_t)RS_TILE, L_out - t0);
    float* dst = y + (int64_t)n * L_out + t0;
    const amx_resample_row r = rows[n];
    if (r.o < 1 || r.m < 1 || r.m > AMX_RESAMPLE_MAX_PHASES || r.taps < 0 || r.width < 0) {  // outside the ABI contract: mark
        fill_tile(dst, tile, __builtin_nanf(""));
        return;
    }
    const int o = (int)r.o, m = (int)r.m, W = (int)r.width, K = (int)r.taps;
    const int64_t len = min(max(lengths[n], (int64_t)0), L_in);
    const int64_t len_out = min(L_out, (len * m + o - 1) / o);
    const int live = (int)max((int64_t)0, min((int64_t)tile, len_out - t0));  // outputs of the tile inside len'
    if (live == 0) {
        fill_tile(dst, tile, 0.f);
        return;
    }
    const float* src = x + (int64_t)n * stride;
    if (o == m) {
        for (int u = threadIdx.x; u < tile; u += RS_THREADS) dst[u] = u < live ? src[t0 + u] : 0.f;
        return;
    }
    const int32_t* first = phases + r.phase_offset;
    const int64_t f0 = t0 / m;
    const int rem0 = (int)(t0 - f0 * m);
    const int a0 = first[0];
    const int64_t nwin = (int64_t)((rem0 + live - 1) / m) * o + (first[m - 1] + K - a0);
    if (nwin > window) {  // the caller's window is too small for this row: never stage past the LDS it asked for
        fill_tile(dst, tile, __builtin_nanf(""));
        return;
    }
    const int64_t g0 = f0 * o + a0 - W;
    for (int i = threadIdx.x; i < nwin; i += RS_THREADS) {
        const int64_t g = g0 + i;
        xs[i] = (g >= 0 && g < len) ? src[g] : 0.f;
    }
    __syncthreads();
    const float* bj0 = bank + r.bank_offset;
    for (int u = threadIdx.x; u < tile; u += RS_THREADS) {
        float acc = 0.f;
        if (u < live) {
            const int q = (rem0 + u) / m;  // frame f - f0
            const int j = rem0 + u - q * m;
            const float* xw = xs + q * o + (first[j] - a0);
            const float* bj = bj0 + j;
#pragma unroll 4
            for (int k = 0; k < K; ++k) acc = fmaf(bj[k * m], xw[k], acc);
        }
        dst[u] = acc;
    }
}

}  // namespace

std::string resample_bank(int64_t orig, int64_t new_rate, int32_t lpw, double rolloff, amx_resample_geometry* g, float* bank,
                          int32_t* phases) {
    const int64_t rate_max = ((int64_t)1 << 31) - 1;
    if (orig < 1 || new_rate < 1 || orig > rate_max || new_rate > rate_max) return "sample rates must be 1 to 2^31 - 1";
    if (lpw < 1 || lpw > 1024) return "lowpass_filter_width must be 1 to 1024";
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return "rolloff must be in (0, 1]";
    const int64_t d = std::gcd(orig, new_rate);
    const int64_t o = orig / d, m = new_rate / d;
    if (o == m) {
        *g = amx_resample_geometry{1, 1, 0, 0, 0, 0};
        return "";
    }
    if (m > AMX_RESAMPLE_MAX_PHASES)
        return "the reduced target rate new / gcd(orig, new) = " + std::to_string(m) + " exceeds " + std::to_string(AMX_RESAMPLE_MAX_PHASES);
    const double f_c = (double)std::min(o, m) * rolloff;
    const double w = std::ceil((double)((int64_t)lpw * o) / f_c);
    // every tile stages at least one frame (o samples) and both filter wings (2W): reject before sizing anything by them
    if (!(w <= AMX_RESAMPLE_MAX_WINDOW) || o > AMX_RESAMPLE_MAX_WINDOW)
        return "the filter window exceeds " + std::to_string(AMX_RESAMPLE_MAX_WINDOW) + " samples";
    const int64_t W = (int64_t)w;
    const int64_t n_taps = 2 * W + o;
    std::vector<int32_t> first(m), count(m);
    int64_t K = 0;
    for (int64_t j = 0; j < m; ++j) {
        int64_t lo = -1, hi = -1;
        for (int64_t i = 0; i < n_taps; ++i) {
            const double tau = ((double)(i - W) / (double)o - (double)j / (double)m) * f_c;
            if (std::fabs(tau) < (double)lpw) {
                if (lo < 0) lo = i;
                hi = i;
            }
        }
        if (lo < 0) lo = hi = W;  // (unreachable: the tap nearest the phase's centre has |tau| <= f_c / 2 < lpw)
        first[j] = (int32_t)lo;
        count[j] = (int32_t)(hi - lo + 1);
        K = std::max<int64_t>(K, hi - lo + 1);
    }
    if (K * m > ((int64_t)1 << 22)) return "the filter bank exceeds 2^22 floats";
    const int64_t window = ((RS_TILE - 1) / m + 1) * o + (first[m - 1] + K - first[0]);
    if (window > AMX_RESAMPLE_MAX_WINDOW)
        return "a tile of " + std::to_string(RS_TILE) + " outputs needs an input window of " + std::to_string(window) +
               " samples, more than " + std::to_string(AMX_RESAMPLE_MAX_WINDOW) + ": the rate ratio is too large";
    *g = amx_resample_geometry{o, m, W, K, K * m, window};
    const double pi = 3.14159265358979323846;
    if (bank) {
        for (int64_t j = 0; j < m; ++j)
            for (int64_t k = 0; k < K; ++k) {
                double h = 0.0;
                if (k < count[j]) {
                    const int64_t i = first[j] + k;
                    const double tau = ((double)(i - W) / (double)o - (double)j / (double)m) * f_c;
                    const double c = std::cos(pi * tau / (2.0 * lpw));
                    const double sinc = tau == 0.0 ? 1.0 : std::sin(pi * tau) / (pi * tau);
                    h = (f_c / (double)o) * c * c * sinc;
                }
                bank[k * m + j] = (float)h;
            }
    }
    if (phases)
        for (int64_t j = 0; j < m; ++j) {
            phases[j] = first[j];
            phases[m + j] = count[j];
        }
    return "";
}

void launch_resample(const float* x, int64_t stride, int64_t L_in, const int64_t* lengths, const amx_resample_row* rows,
                     const float* bank, const int32_t* phases, int window, int N, int64_t L_out, float* y, hipStream_t s) {
    dim3 grid((unsigned)((L_out + RS_TILE - 1) / RS_TILE), (unsigned)N);
    hipLaunchKernelGGL(resample_kernel, grid, dim3(RS_THREADS), (size_t)window * sizeof(float), s, x, stride, L_in, lengths, rows,
                       bank, phases, window, L_out, y);
}

}  // namespace amx
