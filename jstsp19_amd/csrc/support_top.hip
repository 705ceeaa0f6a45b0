// jstsp_support_top_f64 / _c32: the first `count` entries of jstsp_support_order_f64 / _c32 per trial, bit for bit, by the selection
// kernel of support_top.h - one workgroup per trial, one launch for the batch, no vendor sort and no workspace on the device path.
// It is the kernel the refreshed ADMMs (jstsp_proposed_refresh_f64, csrc/proposed64.hip; jstsp_proposed_refresh_c32,
// csrc/proposed.hip through launch_support_top of csrc/admm.hip) run inside their loops; these entries give it callers of its own
// and a test against the full order.  A host call stages V and the list in the context's arena, in chunks of at most 2^31 - 1
// entries as the sibling entries do.
#include "solver_common.h"
#include "support_top.h"
#include <algorithm>

using namespace jstsp;

// Z: double2 (jstsp_support_top_f64) or float2 (jstsp_support_top_c32)
template <class Z> static int support_top_entry(jstsp_ctx *ctx, int Gr, int G2, int batch, const Z *V, int count, int32_t *indx_top, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "support_top: NULL context");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "support_top: bad memspace");
    JSTSP_REQUIRE(Gr > 0 && G2 > 0 && batch > 0, JSTSP_E_SHAPE, "support_top: Gr, G2 and batch must be positive (got %d, %d, %d)", Gr, G2,
                  batch);
    JSTSP_REQUIRE((long long)Gr * G2 < (1ll << 31), JSTSP_E_SHAPE, "support_top: Gr * G2 = %lld exceeds 2^31 - 1", (long long)Gr * G2);
    JSTSP_REQUIRE(V && indx_top, JSTSP_E_NULL, "support_top: NULL array");
    const long long nz = (long long)Gr * G2;
    JSTSP_REQUIRE(count >= 1 && count <= std::min<long long>(nz, JSTSP_SUPPORT_TOP_MAX), JSTSP_E_ARG,
                  "support_top: count = %d: need 1 <= count <= min(Gr * G2, %d) = %lld", count, JSTSP_SUPPORT_TOP_MAX,
                  std::min<long long>(nz, JSTSP_SUPPORT_TOP_MAX));
    static_assert(ST_MAX == JSTSP_SUPPORT_TOP_MAX, "the kernel's LDS list is the header's limit");
    JSTSP_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const int chunk = (int)std::min<long long>(batch, ((1ll << 31) - 1) / nz);
    const bool host = memspace == JSTSP_HOST;
    Z *Vdev = nullptr;
    int32_t *idev = nullptr;
    if (host) {
        const size_t ce = (size_t)chunk * (size_t)nz;
        JSTSP_TRY(ctx->arena.reserve(rnd256(ce * sizeof(Z)) + rnd256((size_t)chunk * count * 4) + 4096));
        ctx->arena.reset();
        Vdev = ctx->arena.get<Z>(ce);
        idev = ctx->arena.get<int32_t>((size_t)chunk * count);
        JSTSP_REQUIRE(Vdev && idev, JSTSP_E_NOMEM, "support_top: workspace exhausted");
    }
    for (int t0 = 0; t0 < batch; t0 += chunk) {
        const int nb = std::min(chunk, batch - t0);
        const Z *src = V + (size_t)t0 * nz;
        int32_t *dst = indx_top + (size_t)t0 * count;
        if (host) {
            JSTSP_HIP(hipMemcpyAsync(Vdev, src, (size_t)nb * nz * sizeof(Z), hipMemcpyHostToDevice, st));
            src = Vdev;
        }
        support_top_kernel<Z><<<nb, ST_THREADS, 0, st>>>((int)nz, count, src, host ? idev : dst, (int32_t *)nullptr);
        JSTSP_HIP(hipGetLastError());
        if (host) {
            JSTSP_HIP(hipMemcpyAsync(dst, idev, (size_t)nb * count * 4, hipMemcpyDeviceToHost, st));
            JSTSP_HIP(hipStreamSynchronize(st));        // (the staging arrays are reused by the next chunk)
        }
    }
    return 0;
}

extern "C" int jstsp_support_top_f64(jstsp_ctx *ctx, int Gr, int G2, int batch, const double *V, int count, int32_t *indx_top, int memspace)
{
    return support_top_entry(ctx, Gr, G2, batch, reinterpret_cast<const double2 *>(V), count, indx_top, memspace);
}

// the head of jstsp_support_order_c32 on the bits: the 32-bit key of support_key.h, four radix passes
extern "C" int jstsp_support_top_c32(jstsp_ctx *ctx, int Gr, int G2, int batch, const jstsp_c32 *S, int count, int32_t *indx_top, int memspace)
{
    return support_top_entry(ctx, Gr, G2, batch, reinterpret_cast<const float2 *>(S), count, indx_top, memspace);
}
