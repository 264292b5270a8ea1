// Microbenchmark: the rate of a bare v_mfma_f64_16x16x4 loop, the ceiling profiles/pearson_pca.md sets the tall-skinny f64 SYRK
// of pearson_pca.hip beside.  Every wave keeps eight independent accumulators (the SYRK keeps four, the scores kernel four) and
// issues nothing but MFMAs in its loop: operands stay in registers, nothing is loaded.  Four waves per SIMD, every CU.
// Build: hipcc --offload-arch=gfx950 -O3 -o mfma_f64_peak mfma_f64_peak.hip        Run: ./mfma_f64_peak [iterations]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef double dvec4 __attribute__((ext_vector_type(4)));
constexpr int kAcc = 8;

__global__ __launch_bounds__(256) void k_mfma_loop(int iters, double a0, double b0, double* __restrict__ out) {
    dvec4 acc[kAcc];
#pragma unroll
    for (int i = 0; i < kAcc; ++i) acc[i] = dvec4{0.0, 0.0, 0.0, 0.0};
    const double a = a0 + (double)(threadIdx.x & 63) * 1e-3, b = b0 - (double)(threadIdx.x & 63) * 1e-3;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < kAcc; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kAcc; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) out[blockIdx.x * 256 + threadIdx.x] = s;          // (keeps the loop; never true for these operands)
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 20000;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int n_cus = prop.multiProcessorCount;
    const int grid = n_cus * 4;                      // 4 workgroups of 4 waves per CU: 4 waves per SIMD
    double* out;
    CK(hipMalloc(&out, (size_t)grid * 256 * sizeof(double)));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        CK(hipEventRecord(e0, nullptr));
        hipLaunchKernelGGL(k_mfma_loop, dim3(grid), dim3(256), 0, nullptr, iters, 1.0, 0.5, out);
        CK(hipGetLastError());
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;         // the first launch loads the code object
    }
    const double flop = (double)grid * 4 * (double)iters * kAcc * (16.0 * 16.0 * 4.0 * 2.0);
    printf("{\"cus\": %d, \"iters\": %d, \"ms\": %.4f, \"f64_mfma_tflops\": %.3f}\n", n_cus, iters, best, flop / (best * 1e-3) / 1e12);
    CK(hipFree(out));
    return 0;
}
