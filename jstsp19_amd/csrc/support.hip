// [~, indx] = sort(abs(vec(S)), 'descend') per trial on the device (plot_errorVSsnr.m:143 for an S that is not the true channel's):
// the order every indx_S argument of the solvers takes, from an estimate that never leaves HBM.
//
//   jstsp_support_order_c32: key ~bits(|z|^2) in fp32 above the index in one 64-bit word (support_key.h, the expression of the
//                            trial builder's indx_S), one hipcub::DeviceSegmentedRadixSort over the trials - the builder's route,
//                            so support_order(Zbar) of a built trial is its indx_S on the bits.
//   jstsp_support_order_f64: the float64 key has 64 bits of its own, and a segmented radix sort promises no stability.  So:
//                            sort the keys alone; class(i) = the position of the first entry equal to key(i) in its trial's sorted
//                            keys (a binary search: equal keys share a class, a larger magnitude has a smaller class); then sort the
//                            words (class << w | index), w = bits of Gr*G2 - unique per trial, 2w <= 62 bits.
// Both sorts are exact on unique or index-free keys, so an order is a function of its own trial alone: of no batch, no chunk and
// no memspace.  Trials are taken in chunks of at most 2^31 - 1 entries (the sort's int counts).
#include "solver_common.h"
#include "support_key.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>

using namespace jstsp;

namespace {

inline int so_grid(long long n) { return (int)std::min<long long>((n + 255) / 256, 4096); }

__global__ void so_offsets_kernel(int count, long long nz, int *off)
{
    for (int i = threadIdx.x; i <= count; i += blockDim.x) off[i] = (int)(i * nz);
}

// _c32: (key << 32) | index
__global__ __launch_bounds__(256) void so_key32_kernel(long long total, long long nz, const float2 *S, uint64_t *keys)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        keys[i] = ((uint64_t)support_key(S[i]) << 32) | (uint64_t)(uint32_t)(i % nz);
}

// _f64: the key alone
__global__ __launch_bounds__(256) void so_key64_kernel(long long total, const double2 *S, uint64_t *keys)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        keys[i] = support_key(S[i]);
}

// _f64: (class << w) | index, class = lower bound of the entry's key in the sorted keys of its trial
__global__ __launch_bounds__(256) void so_class_kernel(long long total, long long nz, int w, const uint64_t *keys,
                                                       const uint64_t *sorted, uint64_t *words)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / nz, idx = i - t * nz;
        const uint64_t k = keys[i];
        const uint64_t *seg = sorted + t * nz;
        long long lo = 0, hi = nz;                      // first position with seg[pos] >= k; k is in seg, so lo < nz at the end
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (seg[mid] < k) lo = mid + 1; else hi = mid;
        }
        words[i] = ((uint64_t)lo << w) | (uint64_t)idx;
    }
}

__global__ __launch_bounds__(256) void so_index_kernel(long long total, uint64_t mask, const uint64_t *words, int32_t *indx)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        indx[i] = (int32_t)(uint32_t)(words[i] & mask) + 1;             // 1-based as MATLAB
}

template <class Z> int support_order_impl(jstsp_ctx *ctx, int Gr, int G2, int batch, const Z *S, int32_t *indx_S, int memspace)
{
    constexpr bool F64 = sizeof(Z) == sizeof(double2);
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "support_order: NULL context");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "support_order: bad memspace");
    JSTSP_REQUIRE(Gr > 0 && G2 > 0 && batch > 0, JSTSP_E_SHAPE, "support_order: Gr, G2 and batch must be positive (got %d, %d, %d)",
                  Gr, G2, batch);
    JSTSP_REQUIRE((long long)Gr * G2 < (1ll << 31), JSTSP_E_SHAPE, "support_order: Gr * G2 = %lld exceeds 2^31 - 1", (long long)Gr * G2);
    JSTSP_REQUIRE(S && indx_S, JSTSP_E_NULL, "support_order: NULL array");
    JSTSP_ENTER(ctx);
    const long long nz = (long long)Gr * G2;
    const int chunk = (int)std::min<long long>(batch, ((1ll << 31) - 1) / nz);
    const size_t ce = (size_t)chunk * (size_t)nz;
    int w = 1;
    while ((1ll << w) < nz) ++w;                        // index < 2^w, class < 2^w
    size_t sort_tmp = 0;
    JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)ce, chunk,
                                                         (const int *)nullptr, (const int *)nullptr, 0, 64, ctx->stream));
    const bool host = memspace == JSTSP_HOST;
    JSTSP_TRY(ctx->arena.reserve((F64 ? 3 : 2) * rnd256(ce * 8) + rnd256(sort_tmp ? sort_tmp : 1) + rnd256(((size_t)chunk + 1) * 4) +
                                 (host ? rnd256(ce * sizeof(Z)) + rnd256(ce * 4) : 0) + 4096));
    ctx->arena.reset();
    Arena &ar = ctx->arena;
    hipStream_t st = ctx->stream;
    uint64_t *k0 = ar.get<uint64_t>(ce), *k1 = ar.get<uint64_t>(ce), *k2 = F64 ? ar.get<uint64_t>(ce) : nullptr;
    void *tmp = ar.get<char>(sort_tmp ? sort_tmp : 1);
    int *off = ar.get<int>((size_t)chunk + 1);
    Z *Sdev = host ? ar.get<Z>(ce) : nullptr;
    int32_t *idev = host ? ar.get<int32_t>(ce) : nullptr;
    JSTSP_REQUIRE(k0 && k1 && (k2 || !F64) && tmp && off && (!host || (Sdev && idev)), JSTSP_E_NOMEM, "support_order: workspace exhausted");
    so_offsets_kernel<<<1, 256, 0, st>>>(chunk, nz, off);
    for (int t0 = 0; t0 < batch; t0 += chunk) {
        const int nb = std::min(chunk, batch - t0);
        const long long total = (long long)nb * nz;
        const Z *src = S + (size_t)t0 * nz;
        int32_t *dst = indx_S + (size_t)t0 * nz;
        if (host) {
            JSTSP_HIP(hipMemcpyAsync(Sdev, src, (size_t)total * sizeof(Z), hipMemcpyHostToDevice, st));
            src = Sdev;
        }
        int32_t *out = host ? idev : dst;
        if constexpr (!F64) {
            so_key32_kernel<<<so_grid(total), 256, 0, st>>>(total, nz, reinterpret_cast<const float2 *>(src), k0);
            JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, sort_tmp, k0, k1, (int)total, nb, off, off + 1, 0, 64, st));
            so_index_kernel<<<so_grid(total), 256, 0, st>>>(total, 0xFFFFFFFFull, k1, out);
        } else {
            so_key64_kernel<<<so_grid(total), 256, 0, st>>>(total, reinterpret_cast<const double2 *>(src), k0);
            JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, sort_tmp, k0, k1, (int)total, nb, off, off + 1, 0, 64, st));
            so_class_kernel<<<so_grid(total), 256, 0, st>>>(total, nz, w, k0, k1, k2);
            JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, sort_tmp, k2, k0, (int)total, nb, off, off + 1, 0, 2 * w, st));
            so_index_kernel<<<so_grid(total), 256, 0, st>>>(total, (1ull << w) - 1, k0, out);
        }
        JSTSP_HIP(hipGetLastError());
        if (host) {
            JSTSP_HIP(hipMemcpyAsync(dst, idev, (size_t)total * 4, hipMemcpyDeviceToHost, st));
            JSTSP_HIP(hipStreamSynchronize(st));        // (the staging arrays are reused by the next chunk)
        }
    }
    return 0;
}

}  // namespace

extern "C" int jstsp_support_order_c32(jstsp_ctx *ctx, int Gr, int G2, int batch, const jstsp_c32 *S, int32_t *indx_S, int memspace)
{
    return support_order_impl(ctx, Gr, G2, batch, reinterpret_cast<const float2 *>(S), indx_S, memspace);
}

extern "C" int jstsp_support_order_f64(jstsp_ctx *ctx, int Gr, int G2, int batch, const double *S, int32_t *indx_S, int memspace)
{
    return support_order_impl(ctx, Gr, G2, batch, reinterpret_cast<const double2 *>(S), indx_S, memspace);
}
