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
//
//   jstsp_support_order_wide_c32 / _f64: the order over neighbouring angle cells.  S is (Gr, Gt*L), column c = l*Gt + g, so a delay
//                            block l is Gr*Gt contiguous entries and both of its axes are DFT grids - rings.  own = the key,
//                            nbr = the smallest key (largest magnitude) of the (2wr+1) x (2wt+1) ring window inside the block;
//                            the order is ascending (nbr, own, index) (primary 0) or (own, nbr, index) (primary 1).
//                            sow_filter_kernel computes both in one read of S: a tile of keys in LDS, the separable minimum along
//                            the rows, then along the columns.  Every nbr is an own key of its trial, so ONE sorted list of the
//                            own keys gives the class of both, and the words (class_a << 2w | class_b << w | index) are sorted as
//                            the _f64 route above sorts its own: 3w <= 63 bits, Gr*Gt*L <= 2^21.  wr = wt = 0 is the plain order
//                            and takes its route.
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

// first position with seg[pos] >= k; k is in seg, so the result is < nz
__device__ __forceinline__ long long so_lower_bound(const uint64_t *seg, long long nz, uint64_t k)
{
    long long lo = 0, hi = nz;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (seg[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// _f64: (class << w) | index, class = lower bound of the entry's key in the sorted keys of its trial
__global__ __launch_bounds__(256) void so_class_kernel(long long total, long long nz, int w, const uint64_t *keys,
                                                       const uint64_t *sorted, uint64_t *words)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / nz, idx = i - t * nz;
        words[i] = ((uint64_t)so_lower_bound(sorted + t * nz, nz, keys[i]) << w) | (uint64_t)idx;
    }
}

// _wide: (class_a << 2w) | (class_b << w) | index; (a, b) = (nbr, own) for primary 0, (own, nbr) for primary 1.  nbr is an own key
// of the same trial, so both classes are lower bounds in the one sorted list of own keys.
__global__ __launch_bounds__(256) void sow_class_kernel(long long total, long long nz, int w, int primary, const uint64_t *own,
                                                        const uint64_t *nbr, const uint64_t *sorted, uint64_t *words)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / nz, idx = i - t * nz;
        const uint64_t *seg = sorted + t * nz;
        const uint64_t co = (uint64_t)so_lower_bound(seg, nz, own[i]), cn = (uint64_t)so_lower_bound(seg, nz, nbr[i]);
        words[i] = ((primary ? co : cn) << (2 * w)) | ((primary ? cn : co) << w) | (uint64_t)idx;
    }
}

// ---- the circular 2-D minimum filter of a delay block's keys ------------------------------------------------------------------------
// One workgroup per (trial, delay block, tile).  The tile's keys sit in LDS, SOW_TILE x SOW_TILE at most (32 KiB: five workgroups
// per CU by LDS, 20 waves).  Per axis, one of two layouts:
//   the axis fits (G <= SOW_TILE): the tile spans it, no halo, and the window wraps by its LDS index;
//   the axis is tiled:             n = SOW_TILE - 2p interior cells and a halo of p cells each side, read through the ring
//                                  ((r0 - p + i) mod G) - the wrap-around is a halo read; the window never leaves the tile.
// A tiled axis takes at most SOW_HALO cells of radius per launch; a larger radius is the composition of several launches (the
// minimum over a window of minima over windows is the minimum over the sum of the windows), the later ones reading nbr.
constexpr int SOW_TILE = 64;
constexpr int SOW_HALO = 8;
constexpr int SOW_CELLS = SOW_TILE * SOW_TILE;

struct SowAxis {
    int G;          // cells of the ring
    int n;          // interior cells of a full tile
    int tiles;
    int p;          // radius of this launch
    int wrap;       // 1: the tile is the ring
};

inline SowAxis sow_axis(int G, int radius_left)
{
    SowAxis a;
    a.G = G;
    a.wrap = G <= SOW_TILE;
    a.p = a.wrap ? radius_left : std::min(radius_left, SOW_HALO);
    a.n = a.wrap ? G : SOW_TILE - 2 * a.p;
    a.tiles = (G + a.n - 1) / a.n;
    return a;
}

__device__ __forceinline__ uint64_t sow_key(const float2 *S, long long i) { return (uint64_t)support_key(S[i]); }
__device__ __forceinline__ uint64_t sow_key(const double2 *S, long long i) { return support_key(S[i]); }
__device__ __forceinline__ uint64_t sow_key(const uint64_t *S, long long i) { return S[i]; }

template <class Src>
__global__ __launch_bounds__(256) void sow_filter_kernel(SowAxis R, SowAxis C, const Src *S, uint64_t *own, uint64_t *nbr)
{
    __shared__ uint64_t tile[SOW_CELLS];
    const int tiles = R.tiles * C.tiles;
    const long long blk = blockIdx.x / tiles;                       // trial * L + delay block: Gr*Gt contiguous entries
    const int tl = (int)(blockIdx.x - blk * tiles);
    const long long base = blk * (long long)R.G * C.G;
    const int r0 = (tl % R.tiles) * R.n, g0 = (tl / R.tiles) * C.n;
    const int nr = min(R.n, R.G - r0), nc = min(C.n, C.G - g0);
    const int hr = R.wrap ? 0 : R.p, hc = C.wrap ? 0 : C.p;
    const int LR = nr + 2 * hr, LC = nc + 2 * hc;                   // LR, LC <= SOW_TILE
    const int cells = LR * LC;
    uint64_t v[SOW_CELLS / 256];

    for (int c = threadIdx.x; c < cells; c += 256) {                // the keys of the tile and its halo; own of the interior
        const int i = c % LR, j = c / LR;
        int r = r0 - hr + i, g = g0 - hc + j;                       // (hr <= SOW_HALO < G on a tiled axis: one wrap is enough)
        r += r < 0 ? R.G : 0;  r -= r >= R.G ? R.G : 0;
        g += g < 0 ? C.G : 0;  g -= g >= C.G ? C.G : 0;
        const long long at = base + (long long)g * R.G + r;
        const uint64_t k = sow_key(S, at);
        tile[c] = k;
        if (own && i >= hr && i < hr + nr && j >= hc && j < hc + nc) own[at] = k;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SOW_CELLS / 256; ++q) {                     // along the rows, every column of the tile
        const int c = threadIdx.x + 256 * q;
        if (c >= cells) break;
        const int i = c % LR, j = c / LR;
        uint64_t m = tile[c];
        if (i >= hr && i < hr + nr)
            for (int d = -R.p; d <= R.p; ++d) {
                int ii = i + d;                                     // a tiled axis stays inside its halo; a ring wraps (2p < LR)
                ii += ii < 0 ? LR : 0;  ii -= ii >= LR ? LR : 0;
                const uint64_t x = tile[ii + j * LR];
                m = x < m ? x : m;
            }
        v[q] = m;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SOW_CELLS / 256; ++q) {
        const int c = threadIdx.x + 256 * q;
        if (c >= cells) break;
        tile[c] = v[q];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += 256) {                // along the columns, the interior only
        const int i = c % LR, j = c / LR;
        if (i < hr || i >= hr + nr || j < hc || j >= hc + nc) continue;
        uint64_t m = tile[c];
        for (int d = -C.p; d <= C.p; ++d) {
            int jj = j + d;
            jj += jj < 0 ? LC : 0;  jj -= jj >= LC ? LC : 0;
            const uint64_t x = tile[i + jj * LR];
            m = x < m ? x : m;
        }
        int r = r0 - hr + i, g = g0 - hc + j;                       // interior: inside the ring already
        nbr[base + (long long)g * R.G + r] = m;
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

template <class Z> int support_order_wide_impl(jstsp_ctx *ctx, int Gr, int Gt, int L, int batch, const Z *S, int wr, int wt, int primary,
                                               int32_t *indx_S, int memspace)
{
    constexpr bool F64 = sizeof(Z) == sizeof(double2);
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "support_order_wide: NULL context");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "support_order_wide: bad memspace");
    JSTSP_REQUIRE(Gr > 0 && Gt > 0 && L > 0 && batch > 0, JSTSP_E_SHAPE,
                  "support_order_wide: Gr, Gt, L and batch must be positive (got %d, %d, %d, %d)", Gr, Gt, L, batch);
    JSTSP_REQUIRE((long long)Gr * Gt <= (1ll << 21) && (long long)Gr * Gt * L <= (1ll << 21), JSTSP_E_SHAPE,
                  "support_order_wide: Gr * Gt * L = %lld exceeds 2^21 (three fields of one 63-bit sort word)", (long long)Gr * Gt * L);
    JSTSP_REQUIRE(wr >= 0 && wt >= 0, JSTSP_E_ARG, "support_order_wide: the radii must not be negative (got %d, %d)", wr, wt);
    JSTSP_REQUIRE(2ll * wr + 1 <= Gr && 2ll * wt + 1 <= Gt, JSTSP_E_ARG,
                  "support_order_wide: a window of %lld x %lld cells meets itself round a ring of %d x %d", 2ll * wr + 1, 2ll * wt + 1, Gr, Gt);
    JSTSP_REQUIRE(primary == 0 || primary == 1, JSTSP_E_ARG, "support_order_wide: primary must be 0 (neighbourhood) or 1 (ties), not %d",
                  primary);
    JSTSP_REQUIRE(S && indx_S, JSTSP_E_NULL, "support_order_wide: NULL array");
    if (wr == 0 && wt == 0)                                 // nbr == own: the plain order, on its own route
        return support_order_impl(ctx, Gr, Gt * L, batch, S, indx_S, memspace);
    JSTSP_ENTER(ctx);
    const long long nz = (long long)Gr * Gt * L;
    const int chunk = (int)std::min<long long>(batch, ((1ll << 31) - 1) / nz);
    const size_t ce = (size_t)chunk * (size_t)nz;
    int w = 1;
    while ((1ll << w) < nz) ++w;                            // index, class_a, class_b < 2^w; w <= 21
    size_t sort_tmp = 0;
    JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)ce, chunk,
                                                         (const int *)nullptr, (const int *)nullptr, 0, 64, ctx->stream));
    const bool host = memspace == JSTSP_HOST;
    JSTSP_TRY(ctx->arena.reserve(4 * rnd256(ce * 8) + rnd256(sort_tmp ? sort_tmp : 1) + rnd256(((size_t)chunk + 1) * 4) +
                                 (host ? rnd256(ce * sizeof(Z)) + rnd256(ce * 4) : 0) + 4096));
    ctx->arena.reset();
    Arena &ar = ctx->arena;
    hipStream_t st = ctx->stream;
    uint64_t *k0 = ar.get<uint64_t>(ce), *k1 = ar.get<uint64_t>(ce), *k2 = ar.get<uint64_t>(ce), *k3 = ar.get<uint64_t>(ce);
    void *tmp = ar.get<char>(sort_tmp ? sort_tmp : 1);
    int *off = ar.get<int>((size_t)chunk + 1);
    Z *Sdev = host ? ar.get<Z>(ce) : nullptr;
    int32_t *idev = host ? ar.get<int32_t>(ce) : nullptr;
    JSTSP_REQUIRE(k0 && k1 && k2 && k3 && tmp && off && (!host || (Sdev && idev)), JSTSP_E_NOMEM, "support_order_wide: workspace exhausted");
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
        // own -> k0, nbr -> k1 (a radius above SOW_HALO on a tiled axis: further launches between k1 and k3)
        uint64_t *nbr = k1, *spare = k3;
        for (int left_r = wr, left_t = wt, pass = 0; pass == 0 || left_r > 0 || left_t > 0; ++pass) {
            const SowAxis R = sow_axis(Gr, left_r), C = sow_axis(Gt, left_t);
            const unsigned grid = (unsigned)((long long)nb * L * R.tiles * C.tiles);        // <= total < 2^31
            if (pass == 0) {
                sow_filter_kernel<<<grid, 256, 0, st>>>(R, C, src, k0, nbr);
            } else {
                sow_filter_kernel<<<grid, 256, 0, st>>>(R, C, (const uint64_t *)nbr, (uint64_t *)nullptr, spare);
                std::swap(nbr, spare);
            }
            left_r -= R.p;
            left_t -= C.p;
        }
        JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, sort_tmp, k0, k2, (int)total, nb, off, off + 1, 0, F64 ? 64 : 32, st));
        sow_class_kernel<<<so_grid(total), 256, 0, st>>>(total, nz, w, primary, k0, nbr, k2, spare);
        JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, sort_tmp, spare, k0, (int)total, nb, off, off + 1, 0, 3 * w, st));
        so_index_kernel<<<so_grid(total), 256, 0, st>>>(total, (1ull << w) - 1, k0, out);
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

extern "C" int jstsp_support_order_wide_c32(jstsp_ctx *ctx, int Gr, int Gt, int L, int batch, const jstsp_c32 *S, int wr, int wt,
                                            int primary, int32_t *indx_S, int memspace)
{
    return support_order_wide_impl(ctx, Gr, Gt, L, batch, reinterpret_cast<const float2 *>(S), wr, wt, primary, indx_S, memspace);
}

extern "C" int jstsp_support_order_wide_f64(jstsp_ctx *ctx, int Gr, int Gt, int L, int batch, const double *S, int wr, int wt,
                                            int primary, int32_t *indx_S, int memspace)
{
    return support_order_wide_impl(ctx, Gr, Gt, L, batch, reinterpret_cast<const double2 *>(S), wr, wt, primary, indx_S, memspace);
}
