// Kernel-level timing of the attention adapter (allophant_amd/csrc/amx_adapter.hip) against the row pass it replaces, on the same
// rows in one process: launch_adapter with and without the next layer's planes, and launch_rownorm (unit gamma, planes only) --
// the launch at the top of a layer that an adapter model does not issue.  Links the built library (its launchers are exported):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iallophant_amd/csrc -Iinclude -o build/attn_adapter_probe tools/attn_adapter_probe.hip \
//         -Lallophant_amd -lallophant_amx -Wl,-rpath,'$ORIGIN/../allophant_amd'
//   build/attn_adapter_probe [rows] [hidden] [adapter dim] [precision 0..3] [iterations]      (tools/attn_adapter_bench.py runs it)
// Prints one JSON line: microseconds per launch (mean over the iterations, HIP events around the whole run) and the bytes each
// launch moves per element of the stream.
#include "amx_common.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace amx;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

static std::vector<float> randn(size_t n, float scale, float mean, unsigned seed) {
    std::vector<float> v(n);
    srand(seed);
    for (auto& x : v) {
        float s = 0.f;
        for (int i = 0; i < 4; ++i) s += (float)rand() / (float)RAND_MAX - 0.5f;  // ~ N(0, 1/3)
        x = mean + scale * s * 1.7320508f;
    }
    return v;
}

template <class F>
static float time_us(F launch, int iters, hipStream_t s) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) launch();
    CK(hipStreamSynchronize(s));
    CK(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i) launch();
    CK(hipEventRecord(b, s));
    CK(hipEventSynchronize(b));
    CK(hipGetLastError());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, a, b));
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    return ms * 1000.f / (float)iters;
}

int main(int argc, char** argv) {
    const int64_t M = argc > 1 ? atoll(argv[1]) : 32 * 499;
    const int D = argc > 2 ? atoi(argv[2]) : 1280, A = argc > 3 ? atoi(argv[3]) : 16, prec = argc > 4 ? atoi(argv[4]) : PREC_F16X3;
    const int iters = argc > 5 ? atoi(argv[5]) : 50;
    if (M < 1 || D < 8 || D > 2048 || D % 8 || A < 1 || A > ADAPTER_MAX_DIM || prec < 0 || prec > 3 || iters < 1) {
        printf("usage: attn_adapter_probe [rows] [hidden: a multiple of 8 up to 2048] [adapter dim 1..64] [precision 0..3] [iterations]\n");
        return 2;
    }
    const int NT = prec_planes(prec);
    const bool il = NT > 1 && D % 32 == 0;
    const int64_t plane = il ? PLANE_IL : M * D;
    float *h, *h0, *w1, *b1, *w2t, *b2, *ones, *zeros;
    void* xp;
    const size_t hb = (size_t)M * D * 4;
    CK(hipMalloc(&h, hb));
    CK(hipMalloc(&h0, hb));
    CK(hipMalloc(&xp, (size_t)M * D * 2 * NT + 256));
    CK(hipMalloc(&w1, (size_t)A * D * 4));
    CK(hipMalloc(&w2t, (size_t)A * D * 4));
    CK(hipMalloc(&b1, (size_t)A * 4));
    CK(hipMalloc(&b2, (size_t)D * 4));
    CK(hipMalloc(&ones, (size_t)D * 4));
    CK(hipMalloc(&zeros, (size_t)D * 4));
    auto up = [](float* d, const std::vector<float>& v) { CK(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice)); };
    up(h0, randn((size_t)M * D, 2.f, 0.1f, 1));
    up(w1, randn((size_t)A * D, 1.f / sqrtf((float)D), 0.f, 2));
    up(w2t, randn((size_t)A * D, 1.f / sqrtf((float)A), 0.f, 3));
    up(b1, randn(A, 0.3f, 0.f, 4));
    up(b2, randn(D, 0.2f, 0.f, 5));
    up(ones, std::vector<float>(D, 1.f));
    up(zeros, std::vector<float>(D, 0.f));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    // (the adapter works in place: every measurement starts from the same rows)
    CK(hipMemcpyAsync(h, h0, hb, hipMemcpyDeviceToDevice, s));
    const float us_norm = time_us([&] { launch_rownorm(prec, h, D, M, D, ones, zeros, 0, nullptr, nullptr, 1e-5f, 0.f, xp, plane, D, nullptr, 0, s); }, iters, s);
    const float us_planes = time_us([&] { launch_adapter(prec, h, M, D, A, w1, b1, w2t, b2, 1e-5f, xp, plane, s); }, iters, s);
    CK(hipMemcpyAsync(h, h0, hb, hipMemcpyDeviceToDevice, s));
    const float us_last = time_us([&] { launch_adapter(prec, h, M, D, A, w1, b1, w2t, b2, 1e-5f, nullptr, plane, s); }, iters, s);
    CK(hipStreamSynchronize(s));
    const double elems = (double)M * D;
    printf("{\"rows\": %lld, \"hidden\": %d, \"adapter_dim\": %d, \"precision\": %d, \"iterations\": %d, "
           "\"rownorm_us\": %.2f, \"adapter_us\": %.2f, \"adapter_last_layer_us\": %.2f, \"adapter_over_rownorm\": %.2f, "
           "\"rownorm_bytes_per_element\": %d, \"adapter_bytes_per_element\": %d, \"rownorm_GBps\": %.0f, \"adapter_GBps\": %.0f}\n",
           (long long)M, D, A, prec, iters, us_norm, us_planes, us_last, us_planes / us_norm, 4 + 2 * NT, 8 + 2 * NT,
           elems * (4 + 2 * NT) / us_norm * 1e-3, elems * (8 + 2 * NT) / us_planes * 1e-3);
    return 0;
}
