// Micro-benchmark: what the f64 matrix pipe sustains on MI355X with nothing but MFMAs in flight - v_mfma_f64_16x16x4_f64 streams
// over 4 / 8 independent accumulators, operands in registers, 1 / 2 waves per SIMD on every CU, random operands - beside the same
// number of multiply-adds issued as v_fma_f64 on the vector unit (the two have the same nominal rate on this chip; what a GEMM
// gains from the pipe is operand reuse, not arithmetic rate: jstsp19_amd/csrc/zgemm64.hip).
//   hipcc --offload-arch=gfx950 -O3 -o mfma_f64_rate mfma_f64_rate.cpp
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <int NACC>
__global__ __launch_bounds__(256) void k_mfma(const double *ops, double *out, int iters)
{
    const int tid = threadIdx.x;
    double a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = ops[(i * 256 + tid) % 2048]; b[i] = ops[((i + 4) * 256 + tid) % 2048]; }
    f64x4 c[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) c[q] = f64x4{0, 0, 0, 0};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < NACC; ++q) c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(u + q) & 3], b[u], c[q], 0, 0, 0);
    }
    double s = 0;
    for (int q = 0; q < NACC; ++q) s += c[q][0] + c[q][1] + c[q][2] + c[q][3];
    out[blockIdx.x * 256 + tid] = s;
}

// 16 independent v_fma_f64 chains per lane
__global__ __launch_bounds__(256) void k_valu(const double *ops, double *out, int iters)
{
    const int tid = threadIdx.x;
    const double a = ops[tid % 2048] * 1e-3, b = ops[(tid + 256) % 2048];
    double c[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) c[q] = ops[(q * 256 + tid) % 2048];
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < 16; ++q) c[q] = __builtin_fma(c[q], a, b);
    }
    double s = 0;
    for (int q = 0; q < 16; ++q) s += c[q];
    out[blockIdx.x * 256 + tid] = s;
}

template <class K> double time_ms(K launch)
{
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    launch(100);
    hipDeviceSynchronize();
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
        hipEventRecord(e0);
        launch(20000);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
    }
    return best;
}

int main()
{
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int cus = prop.multiProcessorCount;
    std::vector<double> h(2048);
    srand(7);
    for (auto &x : h) x = (double)rand() / RAND_MAX - 0.5;
    double *ops, *out;
    hipMalloc(&ops, h.size() * sizeof(double));
    hipMalloc(&out, (size_t)cus * 2 * 256 * sizeof(double));
    hipMemcpy(ops, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
    printf("{\"compute_units\": %d, \"rows\": [", cus);
    bool first = true;
    for (int wps = 1; wps <= 2; ++wps) {
        const int blocks = cus * wps;
        const double mf = 2.0 * 16 * 16 * 4;
        const double m4 = time_ms([&](int it) { k_mfma<4><<<blocks, 256>>>(ops, out, it); });
        const double m8 = time_ms([&](int it) { k_mfma<8><<<blocks, 256>>>(ops, out, it); });
        const double v = time_ms([&](int it) { k_valu<<<blocks, 256>>>(ops, out, it); });
        const double tf4 = (double)blocks * 4 * 20000 * 4 * 4 * mf / m4 / 1e9, tf8 = (double)blocks * 4 * 20000 * 4 * 8 * mf / m8 / 1e9;
        const double tfv = (double)blocks * 256 * 20000.0 * 4 * 16 * 2 / v / 1e9;
        printf("%s\n {\"waves_per_simd\": %d, \"mfma_f64_16x16x4_4acc_tflops\": %.2f, \"mfma_f64_16x16x4_8acc_tflops\": %.2f, \"v_fma_f64_tflops\": %.2f}",
               first ? "" : ",", wps, tf4, tf8, tfv);
        first = false;
    }
    printf("]}\n");
    return 0;
}
