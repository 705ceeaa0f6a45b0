// The f64-MFMA GEMM of jstsp19_amd/csrc/zgemm64.hip against the 16 x 16 LDS-tile VALU kernel of vamp64.hip (zgemm_kernel) on the
// five product shapes of the float64 proposed_algorithm at BASELINE configs[1] (N = Gr = 64, G2 = 512, M = 4096), batch 16.
// Both kernels live in unnamed namespaces of the library's sources, so this file includes the two sources themselves and links
// the library for the rest:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -x hip -I../../jstsp19_amd/csrc f64_gemm_bench.cpp -o f64_gemm_bench \
//         -L../../jstsp19_amd/csrc -ljstsp_mi355x -Wl,-rpath,'$ORIGIN/../../jstsp19_amd/csrc'
// Prints one JSON object: per shape the median of 9 timed launches (after 2 warm-up launches) of each kernel, GFLOP/s, and the
// largest entrywise difference between the two results relative to the largest entry.
#include "vamp64.hip"
#include "zgemm64.hip"

#include <cmath>
#include <cstdio>

namespace {
template <class F> double median_ms(hipStream_t st, F launch)
{
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    launch(); launch();
    hipStreamSynchronize(st);
    std::vector<float> ms(9);
    for (auto &m : ms) {
        hipEventRecord(e0, st);
        launch();
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&m, e0, e1);
    }
    std::sort(ms.begin(), ms.end());
    return ms[4];
}
}  // namespace

int main()
{
    using namespace jstsp;
    const int N = 64, Gr = 64, G2 = 512, M = 4096, batch = 16;
    struct Shape { const char *name; char opA, opB; int m, n, k; };
    const Shape shapes[5] = {{"(N x Gr)(Gr x G2)", 'N', 'N', N, G2, Gr}, {"(N x G2)(G2 x M)", 'N', 'N', N, M, G2}, {"(Gr x N)(N x M), A^H", 'C', 'N', Gr, M, N},
                             {"(Gr x M)(M x G2), B^H", 'N', 'C', Gr, G2, M}, {"(N x M)(M x N), Z Z^H", 'N', 'C', N, N, M}};
    hipStream_t st;
    hipStreamCreate(&st);
    printf("{\"batch\": %d, \"shapes\": [", batch);
    for (int s = 0; s < 5; ++s) {
        const Shape &sh = shapes[s];
        const size_t na = (size_t)sh.m * sh.k * batch, nb = (size_t)sh.k * sh.n * batch, nc = (size_t)sh.m * sh.n * batch;
        std::vector<double2> ha(na), hb(nb);
        srand(11 + s);
        for (auto &x : ha) x = make_double2((double)rand() / RAND_MAX - 0.5, (double)rand() / RAND_MAX - 0.5);
        for (auto &x : hb) x = make_double2((double)rand() / RAND_MAX - 0.5, (double)rand() / RAND_MAX - 0.5);
        double2 *a, *b, *c0, *c1, *ws;
        hipMalloc(&a, na * sizeof(double2)); hipMalloc(&b, nb * sizeof(double2)); hipMalloc(&c0, nc * sizeof(double2)); hipMalloc(&c1, nc * sizeof(double2));
        hipMalloc(&ws, std::max<size_t>(1, zgemm64_ws_elems(sh.m, sh.n, sh.k, batch)) * sizeof(double2));
        hipMemcpy(a, ha.data(), na * sizeof(double2), hipMemcpyHostToDevice);
        hipMemcpy(b, hb.data(), nb * sizeof(double2), hipMemcpyHostToDevice);
        // stored shapes: op 'C' operands are stored transposed
        const int lda = sh.opA == 'C' ? sh.k : sh.m, ldb = sh.opB == 'C' ? sh.n : sh.k;
        const long long sa = (long long)sh.m * sh.k, sb = (long long)sh.k * sh.n, sc = (long long)sh.m * sh.n;
        const double t_valu = median_ms(st, [&] { zgemm(st, sh.opA, sh.opB, sh.m, sh.n, sh.k, batch, MatD{a, sa, lda}, MatD{b, sb, ldb}, c0, sc, sh.m); });
        const double t_mfma = median_ms(st, [&] { zgemm64(st, sh.opA, sh.opB, sh.m, sh.n, sh.k, batch, Mat64{a, sa, lda}, Mat64{b, sb, ldb}, c1, sc, sh.m, ws); });
        std::vector<double2> h0(nc), h1(nc);
        hipMemcpy(h0.data(), c0, nc * sizeof(double2), hipMemcpyDeviceToHost);
        hipMemcpy(h1.data(), c1, nc * sizeof(double2), hipMemcpyDeviceToHost);
        double dmax = 0, cmax = 0;
        for (size_t i = 0; i < nc; ++i) {
            dmax = std::max(dmax, std::hypot(h0[i].x - h1[i].x, h0[i].y - h1[i].y));
            cmax = std::max(cmax, std::hypot(h0[i].x, h0[i].y));
        }
        const double gf = 8.0 * sh.m * sh.n * sh.k * batch / 1e6;
        printf("%s\n {\"shape\": \"%s\", \"m\": %d, \"n\": %d, \"k\": %d, \"valu_tile_ms\": %.4f, \"mfma_ms\": %.4f, \"valu_tile_gflops\": %.0f, \"mfma_gflops\": %.0f, "
               "\"speedup\": %.2f, \"max_rel_diff\": %.2e}", s ? "," : "", sh.name, sh.m, sh.n, sh.k, t_valu, t_mfma, gf / t_valu, gf / t_mfma, t_valu / t_mfma, dmax / cmax);
        hipFree(a); hipFree(b); hipFree(c0); hipFree(c1); hipFree(ws);
    }
    printf("]}\n");
    return 0;
}
