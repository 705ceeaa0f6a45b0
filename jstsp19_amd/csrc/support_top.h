// The first `count` entries of jstsp_support_order_f64 / _c32 of a trial without sorting the trial: ONE selection body over the
// element type (double2 / float2) for jstsp_support_top_f64 / _c32 (csrc/support_top.hip) and for the refresh inside the ADMM
// loops (float64: csrc/proposed64.hip; fp32: csrc/admm.hip, launch_support_top), which read the solver's own v and write the rank
// its mask needs.  One workgroup of 1024 threads per trial, four steps:
//   1. radix select on the key of support_key.h (64 bits for double2, 32 for float2), top byte first (eight / four histogram
//      passes over the trial, which stays in L2): thr = the count-th smallest key, need = how many entries equal to thr belong
//      to the list;
//   2. the entries with key < thr (ns = count - need of them, at most count - 1) are compacted into LDS in index order;
//   3. the entries with key == thr are admitted in ascending index by an ordered ballot count until `need` is reached, and written
//      straight to their places ns, ns + 1, ... of the list: a tie class of any size - the exact zeros of a thresholded S - costs
//      no LDS;
//   4. the strict part is sorted in LDS by (key, index), a bitonic network over the next power of two, and written out.
// Every count is an integer sum and every position follows from (key, index) alone: a trial's list depends on no batch, no
// launch and no memspace.  Static LDS: 4096 keys of 8 (4) bytes and 4096 indices of 4 - 48 KiB (32 KiB) - plus the histogram;
// no dynamic LDS.
// Two writers: list[p] (1-based index of position p, p < count; may be NULL) and rank[e] for EVERY entry e of the trial (its
// position in the list, or ST_UNLISTED; may be NULL) - what step_v64_kernel / soft_mask64_kernel (soft_kernel in fp32) compare
// with the mask count.
#pragma once
#include "support_key.h"

namespace {

constexpr int ST_MAX = 4096;                    // JSTSP_SUPPORT_TOP_MAX of include/jstsp.h
constexpr int ST_THREADS = 1024;                // the workgroup of every caller but the fp32 loop beside a resident Jacobi (512)
constexpr int32_t ST_UNLISTED = 0x7fffffff;     // the rank rank64_init_kernel gives an entry that no indx_S lists

// exclusive prefix counts of two flags over the workgroup's threads in thread order, and their totals (wave64 ballots, NT / 64 waves)
template <int NT>
__device__ __forceinline__ void st_block_rank2(bool fa, bool fb, int (*wsum)[NT / 64], int &ra, int &rb, int &ta, int &tb)
{
    const unsigned long long ma = __ballot(fa), mb = __ballot(fb);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    __syncthreads();
    if (lane == 0) { wsum[0][wave] = __popcll(ma); wsum[1][wave] = __popcll(mb); }
    __syncthreads();
    int ba = 0, bb = 0, sa = 0, sb = 0;
    for (int w = 0; w < NT / 64; ++w) {
        const int ca = wsum[0][w], cb = wsum[1][w];
        if (w < wave) { ba += ca; bb += cb; }
        sa += ca; sb += cb;
    }
    ra = ba + __popcll(ma & below); rb = bb + __popcll(mb & below);
    ta = sa; tb = sb;
}

// g entries per trial (g < 2^31), 1 <= count <= min(g, ST_MAX): checked by the callers.  Z: double2 or float2; NT threads (a
// list does not depend on NT: the chunks of NT entries are walked in index order)
template <class Z, int NT = ST_THREADS>
__global__ __launch_bounds__(NT) void support_top_kernel(int g, int count, const Z *V, int32_t *list, int32_t *rank)
{
    using Key = decltype(support_key(Z{}));            // uint64_t / uint32_t
    constexpr int TOP = 8 * (int)sizeof(Key) - 8;       // shift of the key's top byte
    constexpr Key KMAX = ~(Key)0;
    __shared__ Key ck[ST_MAX];
    __shared__ int32_t ci[ST_MAX];
    __shared__ unsigned hist[256];
    __shared__ int wsum[2][NT / 64];
    __shared__ Key s_prefix;
    __shared__ int s_need;
    const int tid = threadIdx.x, lane = tid & 63;
    const Z *v = V + (long long)blockIdx.x * g;
    int32_t *lst = list ? list + (long long)blockIdx.x * count : nullptr;
    int32_t *rk = rank ? rank + (long long)blockIdx.x * g : nullptr;

    // 1. thr: the count-th smallest key.  A wave adds each of its distinct bytes once (most entries share their top bytes).
    Key prefix = 0;
    int need = count;
    for (int shift = TOP; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (long long c = 0; c < g; c += NT) {
            const long long i = c + tid;
            Key key = 0;
            bool act = false;
            if (i < g) {
                key = support_key(v[i]);
                act = shift == TOP || (key >> (shift + 8)) == (prefix >> (shift + 8));
            }
            const unsigned b = (unsigned)(key >> shift) & 255u;
            unsigned long long rem = __ballot(act);
            while (rem) {
                const int src = __ffsll(rem) - 1;
                const unsigned bs = __shfl(b, src);
                const unsigned long long m = __ballot(act && b == bs);
                if (lane == src) atomicAdd(&hist[bs], (unsigned)__popcll(m));
                rem &= ~m;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int cum = 0, b = 0;
            for (; b < 255; ++b) { if (cum + (int)hist[b] >= need) break; cum += hist[b]; }
            s_prefix = prefix | ((Key)b << shift); s_need = need - cum;
        }
        __syncthreads();
        prefix = s_prefix; need = s_need;
        __syncthreads();
    }
    const Key thr = prefix;
    const int ns = count - need;                    // entries with key < thr; 1 <= need: at least one entry holds thr

    // 2. and 3. one pass in index order: the strict part to LDS, the tie class to its places, everything else unlisted
    int base_s = 0, base_e = 0;
    for (long long c = 0; c < g; c += NT) {
        const long long i = c + tid;
        const Key key = i < g ? support_key(v[i]) : KMAX;
        const bool strict = i < g && key < thr, eq = i < g && key == thr;
        int rs, re, ts, te;
        st_block_rank2<NT>(strict, eq, wsum, rs, re, ts, te);
        if (strict) {
            const int p = base_s + rs;
            if (p < ST_MAX) { ck[p] = key; ci[p] = (int32_t)i; }
        } else if (i < g) {
            const int r = base_e + re;
            const bool in = eq && r < need;
            if (in && lst) lst[ns + r] = (int32_t)i + 1;                // 1-based as MATLAB
            if (rk) rk[i] = in ? ns + r : ST_UNLISTED;
        }
        base_s += ts; base_e += te;
    }

    // 4. the strict part by (key, index): bitonic over n2 = the next power of two, the padding above every entry
    int n2 = 1;
    while (n2 < ns) n2 <<= 1;
    for (int p = ns + tid; p < n2; p += NT) { ck[p] = KMAX; ci[p] = 0x7fffffff; }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = tid; x < n2; x += NT) {
                const int y = x ^ j;
                if (y > x) {
                    const Key kx = ck[x], ky = ck[y];
                    const int32_t ix = ci[x], iy = ci[y];
                    const bool gt = kx > ky || (kx == ky && ix > iy);
                    if (gt == ((x & k) == 0)) { ck[x] = ky; ck[y] = kx; ci[x] = iy; ci[y] = ix; }
                }
            }
            __syncthreads();
        }
    for (int p = tid; p < ns; p += NT) {
        const int32_t e = ci[p];
        if (lst) lst[p] = e + 1;
        if (rk) rk[e] = p;
    }
}

}  // namespace
