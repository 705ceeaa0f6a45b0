// Batched complex float64 GEMM on the f64 matrix pipe (v_mfma_f64_16x16x4_f64) and the two kernel-level float64 entries built on
// it, jstsp_correlate_f64 (A' K B') and jstsp_synthesize_f64 (A S B).
//
//   C[t] (m x n) = op(A[t]) op(B[t]),  op: as stored or conjugate transpose,  column-major interleaved double2
//
// The shapes this serves have one skinny dimension (N, Gr: 16 .. 128) against a long one (G2, M: hundreds to thousands), so a
// workgroup of four waves owns a 64 x 64 tile of C - the whole skinny side of a trial at the sizes of BASELINE configs[1] - and
// streams the long operand through LDS in steps of 16 along k (32 x 32 tiles when a trial has too few 64 x 64 ones to fill the chip).
//   * staging: 256 threads fetch the 64 x 16 tile of op(A) and the 16 x 64 tile of op(B) (one k step ahead, in registers, while
//     the matrix pipe works on the current one) and write them to LDS split into real and imaginary PLANES, [k][row] with a row
//     stride of tile + 16 doubles (the four k rows that one MFMA operand read touches fall into different halves of the 64 banks).  A
//     conjugate-transposed operand is transposed here - its global reads run along its own leading dimension - and never exists
//     in global memory.  A gets a third plane, -Im(A), negated once here.
//   * a complex product is four real accumulations on those planes: Re += Ar Br, Re += (-Ai) Bi, Im += Ar Bi, Im += Ai Br.  No
//     3-multiplication form: its cancellation would break the entrywise bound |C - C_ref| <= c k eps (|A| |B|).
//   * operands: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one double each; the f64 result tile has
//     col = l & 15, row = (l >> 4) + 4 r in register r - NOT the row map of the other MFMA shapes.  The tile is accumulated
//     transposed (B fragment first) so that the lane index runs along the rows of C and the stores are 256-byte runs.
//   * edges: rows, columns and k beyond the matrix are staged as zeros and never stored (an Inf in the operand therefore meets
//     padding only in entries that are dropped).
//   * a result of few tiles with a long k (the Gram Z Z^H: one tile per trial; T B^H: eight) is cut along k into chunks whose partial
//     products go to a scratch array and are added in a fixed order by zsplit_sum_kernel: the number of chunks depends on the shape
//     alone, so a trial's bits do not depend on the batch, and there is no atomic anywhere.
// The pipe's f64 rate equals the vector unit's on this chip; what this kernel gains over the 16 x 16 LDS-tile VALU kernel of
// vamp64.hip is that one 8-byte LDS read feeds 16 multiply-adds instead of one (DESIGN.md section 6 has the measured rates).
#include "zgemm64.h"

#include <algorithm>
#include <vector>

namespace jstsp {
namespace {

using d4 = __attribute__((ext_vector_type(4))) double;

constexpr int ZK = 16;           // k per LDS stage

// One workgroup (four waves, 2 x 2) owns a TM x TM tile of C, TM = 32 MI; a wave owns MI x MI MFMA tiles of 16 x 16.  MI = 2 is
// the streaming configuration; MI = 1 serves products with so few 64 x 64 tiles that they would leave most of the chip idle.
// element e of a staged TM x 16 tile -> (index along the TM-wide side, index along k); the fast index follows the operand's
// contiguous direction in global memory
template <int TM> __device__ __forceinline__ void tile_elem(int e, bool k_fast, int &w, int &kk)
{
    if (k_fast) { kk = e & (ZK - 1); w = e >> 4; }
    else { w = e & (TM - 1); kk = e / TM; }
}

template <int MI>
__global__ __launch_bounds__(256) void zgemm64_kernel(int opA, int opB, int m, int n, int k, int kchunk, Mat64 A, Mat64 B, double2 *C, long long sC,
                                                      int ldc, long long sSplit)
{
    constexpr int TM = 32 * MI, LD = TM + 16, PT = TM * ZK / 256;       // tile, LDS row stride (doubles), staged elements per thread
    __shared__ double sAr[ZK * LD], sAi[ZK * LD], sAn[ZK * LD], sBr[ZK * LD], sBi[ZK * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_m = (m + TM - 1) / TM;
    const int i0 = (blockIdx.x % tiles_m) * TM, j0 = (blockIdx.x / tiles_m) * TM;
    const int t = blockIdx.z;
    const int k0 = blockIdx.y * kchunk, k1 = min(k, k0 + kchunk);
    const double2 *a = A.p + (long long)t * A.st, *b = B.p + (long long)t * B.st;
    const int wm = (wave & 1) * 16 * MI, wn = (wave >> 1) * 16 * MI;

    double2 ra[PT], rb[PT];
    auto fetch = [&](int kk0) {
#pragma unroll
        for (int r = 0; r < PT; ++r) {
            const int e = tid + 256 * r;
            int w, kk;
            tile_elem<TM>(e, opA != 0, w, kk);
            const int i = i0 + w, kg = kk0 + kk;
            double2 v = make_double2(0.0, 0.0);
            if (i < m && kg < k1) {
                v = opA ? a[kg + (long long)A.ld * i] : a[i + (long long)A.ld * kg];
                if (opA) v.y = -v.y;
            }
            ra[r] = v;
            tile_elem<TM>(e, opB == 0, w, kk);
            const int j = j0 + w, kh = kk0 + kk;
            v = make_double2(0.0, 0.0);
            if (j < n && kh < k1) {
                v = opB ? b[j + (long long)B.ld * kh] : b[kh + (long long)B.ld * j];
                if (opB) v.y = -v.y;
            }
            rb[r] = v;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int r = 0; r < PT; ++r) {
            const int e = tid + 256 * r;
            int w, kk;
            tile_elem<TM>(e, opA != 0, w, kk);
            sAr[kk * LD + w] = ra[r].x; sAi[kk * LD + w] = ra[r].y; sAn[kk * LD + w] = -ra[r].y;
            tile_elem<TM>(e, opB == 0, w, kk);
            sBr[kk * LD + w] = rb[r].x; sBi[kk * LD + w] = rb[r].y;
        }
    };

    d4 accR[MI][MI], accI[MI][MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < MI; ++ni) { accR[mi][ni] = d4{0.0, 0.0, 0.0, 0.0}; accI[mi][ni] = d4{0.0, 0.0, 0.0, 0.0}; }

    if (k0 < k1) fetch(k0);
    for (int kk0 = k0; kk0 < k1; kk0 += ZK) {
        stage();
        __syncthreads();
        if (kk0 + ZK < k1) fetch(kk0 + ZK);
#pragma unroll
        for (int ks = 0; ks < ZK / 4; ++ks) {
            const int row = (ks * 4 + (lane >> 4)) * LD + (lane & 15);
            double ar[MI], ai[MI], an[MI], br[MI], bi[MI];
#pragma unroll
            for (int u = 0; u < MI; ++u) {
                ar[u] = sAr[row + wm + 16 * u]; ai[u] = sAi[row + wm + 16 * u]; an[u] = sAn[row + wm + 16 * u];
                br[u] = sBr[row + wn + 16 * u]; bi[u] = sBi[row + wn + 16 * u];
            }
            // The tile is accumulated TRANSPOSED, D = (B tile)^T (A tile)^T: the B fragment goes in as the MFMA's first operand and the
            // A fragment as its second, so that the lane index of the result runs along the ROWS of C, which are contiguous in memory
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < MI; ++ni) {
                    accR[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(br[ni], ar[mi], accR[mi][ni], 0, 0, 0);
                    accR[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(bi[ni], an[mi], accR[mi][ni], 0, 0, 0);
                    accI[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(bi[ni], ar[mi], accI[mi][ni], 0, 0, 0);
                    accI[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(br[ni], ai[mi], accI[mi][ni], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    // f64 C/D map of the transposed tile: row of C = lane & 15, column of C = (lane >> 4) + 4 r: a store instruction writes four runs
    // of 16 consecutive rows (256 bytes each)
    double2 *c = C + (long long)t * sC + (long long)blockIdx.y * sSplit;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < MI; ++ni) {
            const int i = i0 + wm + 16 * mi + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + wn + 16 * ni + (lane >> 4) + 4 * r;
                if (i < m && j < n) c[i + (long long)ldc * j] = make_double2(accR[mi][ni][r], accI[mi][ni][r]);
            }
        }
}

// C[t](i, j) = sum over s (in order) of P[(t splits + s) m n + i + m j]
__global__ __launch_bounds__(256) void zsplit_sum_kernel(int m, int n, int splits, const double2 *P, double2 *C, long long sC, int ldc)
{
    const int t = blockIdx.y;
    const long long mn = (long long)m * n;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < mn; e += (long long)gridDim.x * 256) {
        const double2 *p = P + (long long)t * splits * mn + e;
        double2 acc = p[0];
        for (int s = 1; s < splits; ++s) { const double2 v = p[(long long)s * mn]; acc.x += v.x; acc.y += v.y; }
        C[(long long)t * sC + (e % m) + (long long)ldc * (e / m)] = acc;
    }
}

}  // namespace

static long long tiles64(int m, int n) { return (long long)((m + 63) / 64) * ((n + 63) / 64); }

// chunks along k: enough that a trial offers about 32 workgroups, at least 256 of k each - a function of the shape alone
int zgemm64_splits(int m, int n, int k)
{
    const long long s = std::min<long long>(k / 256, 32 / std::max<long long>(1, tiles64(m, n)));
    return (int)std::max<long long>(1, std::min<long long>(16, s));
}

size_t zgemm64_ws_elems(int m, int n, int k, int batch)
{
    const int s = zgemm64_splits(m, n, k);
    return s > 1 ? (size_t)s * m * n * batch : 0;
}

int zgemm64(hipStream_t st, char opA, char opB, int m, int n, int k, int batch, Mat64 A, Mat64 B, double2 *C, long long sC, int ldc, double2 *ws)
{
    JSTSP_REQUIRE(m > 0 && n > 0 && k > 0 && batch > 0 && batch <= 65535, JSTSP_E_UNSUPPORTED, "float64 GEMM: %d x %d x %d, batch %d (batch <= 65535)",
                  m, n, k, batch);
    const int splits = ws ? zgemm64_splits(m, n, k) : 1;
    const bool small = tiles64(m, n) * splits < 32;             // few 64 x 64 tiles per trial: 32 x 32 tiles instead
    const int tm = small ? 32 : 64;
    const long long tiles = (long long)((m + tm - 1) / tm) * ((n + tm - 1) / tm);
    JSTSP_REQUIRE(tiles < (1ll << 31), JSTSP_E_UNSUPPORTED, "float64 GEMM: grid too large");
    const int kchunk = splits > 1 ? (((k + splits - 1) / splits + ZK - 1) / ZK) * ZK : k;
    const int oa = opA == 'C' ? 1 : 0, ob = opB == 'C' ? 1 : 0;
    const long long mn = (long long)m * n;
    double2 *out = splits > 1 ? ws : C;
    const long long so = splits > 1 ? (long long)splits * mn : sC, ss = splits > 1 ? mn : 0;
    const int ldo = splits > 1 ? m : ldc;
    const dim3 grid((unsigned)tiles, splits, batch);
    if (small) hipLaunchKernelGGL(zgemm64_kernel<1>, grid, dim3(256), 0, st, oa, ob, m, n, k, kchunk, A, B, out, so, ldo, ss);
    else hipLaunchKernelGGL(zgemm64_kernel<2>, grid, dim3(256), 0, st, oa, ob, m, n, k, kchunk, A, B, out, so, ldo, ss);
    if (splits > 1)
        hipLaunchKernelGGL(zsplit_sum_kernel, dim3((unsigned)std::min<long long>((mn + 255) / 256, 1024), batch), dim3(256), 0, st, m, n, splits, ws, C, sC, ldc);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

}  // namespace jstsp

using namespace jstsp;

namespace {

// stream-ordered temporaries of one call; a caller array in device memory is itself (JSTSP_DEVICE) or a staged copy (JSTSP_HOST)
struct Stage64 {
    hipStream_t st;
    int memspace, rc = 0;
    std::vector<void *> held;
    Stage64(hipStream_t s, int ms) : st(s), memspace(ms) {}
    ~Stage64() { for (void *p : held) (void)hipFreeAsync(p, st); }
    template <class T> T *get(size_t n)
    {
        if (rc) return nullptr;
        void *p = nullptr;
        const hipError_t e = hipMallocAsync(&p, std::max<size_t>(n * sizeof(T), 16), st);
        if (e != hipSuccess) { set_error("float64 path: hipMallocAsync(%zu) failed: %s", n * sizeof(T), hipGetErrorString(e)); rc = (int)e; return nullptr; }
        held.push_back(p);
        return static_cast<T *>(p);
    }
    const double2 *in(const jstsp_c64 *src, size_t n)
    {
        if (memspace == JSTSP_DEVICE) return reinterpret_cast<const double2 *>(src);
        double2 *d = get<double2>(n);
        if (!d) return nullptr;
        const hipError_t e = hipMemcpyAsync(d, src, n * sizeof(double2), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) { set_error("float64 path: upload failed: %s", hipGetErrorString(e)); rc = (int)e; return nullptr; }
        return d;
    }
};

// out = op(A) X op(B) in two products: first A (left), then B (right)
int kron_apply64(jstsp_ctx *ctx, bool adjoint, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *X_, const jstsp_c64 *A_, long long strideA,
                 const jstsp_c64 *B_, long long strideB, jstsp_c64 *out_, int memspace, const char *nm)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0 && strideA >= 0 && strideB >= 0, JSTSP_E_SHAPE, "%s: bad shape", nm);
    JSTSP_REQUIRE(X_ && A_ && B_ && out_, JSTSP_E_NULL, "%s: NULL argument", nm);
    const int xr = adjoint ? N : Gr, xc = adjoint ? M : G2, orr = adjoint ? Gr : N, oc = adjoint ? G2 : M;
    const size_t nx = (size_t)xr * xc * batch, no = (size_t)orr * oc * batch;
    const size_t szA = (strideA ? (size_t)strideA * (batch - 1) : 0) + (size_t)N * Gr, szB = (strideB ? (size_t)strideB * (batch - 1) : 0) + (size_t)G2 * M;
    Stage64 sg(ctx->stream, memspace);
    const double2 *X = sg.in(X_, nx), *A = sg.in(A_, szA), *B = sg.in(B_, szB);
    double2 *out = memspace == JSTSP_DEVICE ? reinterpret_cast<double2 *>(out_) : sg.get<double2>(no);
    double2 *T = sg.get<double2>((size_t)orr * xc * batch);       // op(A) X
    const char op = adjoint ? 'C' : 'N';
    const int ka = adjoint ? N : Gr, kb = adjoint ? M : G2;
    double2 *ws = sg.get<double2>(std::max<size_t>(1, std::max(zgemm64_ws_elems(orr, xc, ka, batch), zgemm64_ws_elems(orr, oc, kb, batch))));
    JSTSP_TRY(sg.rc);
    JSTSP_TRY(zgemm64(ctx->stream, op, 'N', orr, xc, ka, batch, Mat64{A, strideA, N}, Mat64{X, (long long)xr * xc, xr}, T, (long long)orr * xc, orr, ws));
    JSTSP_TRY(zgemm64(ctx->stream, 'N', op, orr, oc, kb, batch, Mat64{T, (long long)orr * xc, orr}, Mat64{B, strideB, G2}, out, (long long)orr * oc, orr, ws));
    if (memspace == JSTSP_HOST) {
        JSTSP_HIP(hipMemcpyAsync(out_, out, no * sizeof(double2), hipMemcpyDeviceToHost, ctx->stream));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

}  // namespace

extern "C" {

int jstsp_correlate_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *K, const jstsp_c64 *A, long long strideA,
                        const jstsp_c64 *B, long long strideB, jstsp_c64 *out, int memspace)
{
    return kron_apply64(ctx, true, N, M, Gr, G2, batch, K, A, strideA, B, strideB, out, memspace, "correlate (float64)");
}

int jstsp_synthesize_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *S, const jstsp_c64 *A, long long strideA,
                         const jstsp_c64 *B, long long strideB, jstsp_c64 *out, int memspace)
{
    return kron_apply64(ctx, false, N, M, Gr, G2, batch, S, A, strideA, B, strideB, out, memspace, "synthesize (float64)");
}

}  // extern "C"
