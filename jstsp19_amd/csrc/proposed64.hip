// jstsp_proposed_algorithm_f64 / jstsp_svt_f64 - proposed_algorithm.m:1-73 and proposed_algorithm_angles.m:1-85 ('approximate')
// evaluated in FLOAT64 on the device: storage, products, reductions, eigen-decompositions, thresholds and every scalar.  This is
// the reference path of the library (what MATLAB would have returned, to more digits than the fp32 solver carries, and the float64
// side of a parity fixture at device speed); it is written for clarity, one kernel per step of the iteration:
//   G_A = A^H A, G_B = B B^H once per call (G_B once for the batch when B is shared)                                   (:25)
//   per iteration  Z = X - V1/rho;  G = Z Z^H (or Z^H Z, the smaller side n = min(N, M));  G = U diag(lambda) U^H;
//                  Y = U diag(max(0, 1 - tau/sigma)) U^H Z,  sigma = sqrt(lambda)                                      (:35, svt.m)
//                  X = (V1 + rho Y + subY + V2 + rho C + rho Xs) ./ (Omega + 2 rho);  K = X - V2/rho - C               (:38-43)
//                  Res = A^H K B^H - G_A V G_B;  alpha = <Res, Res> / <Res, G_A Res G_B>;  V += alpha Res              (:47-51)
//                  S = soft(V, tau_S/rho) (.* the cumulative mask of _angles);  Xs = A S B                             (:56-58)
//                  C = rho/(rho+1) (X - Xs - V2/rho);  V1 += rho (Y - X);  V2 += rho (C - X + Xs)                      (:61-65)
//                  convergence_error(i, 1:2) = lambda_max of the Grams of V1, V2 over that of X                        (:67-69)
// All products go through zgemm64.hip (f64 MFMA).  The svt guard is the one the float64 host port uses (the committed
// fixtures were solved with it): a non-positive eigenvalue of the Gram is a singular value at rounding level and is dropped, so
// the output is all zeros exactly when NO eigenvalue is positive (the zero argument of iteration 1, svt.m:8-12).
// Eigen-decomposition: for n <= 64 a two-sided cyclic Jacobi with H and U in LDS, one workgroup per trial, that stops on the
// device when a sweep rotates nothing (at most 30 sweeps) - nothing is read back inside the iteration loop.  For 64 < n <= 512 the
// global-memory Jacobi of vamp64.hip, which reads one norm per sweep on the host: such a call synchronises the stream.
// Every reduction is a fixed-order sum inside one workgroup per trial: a trial's bits depend neither on the batch nor on the run.
//
// jstsp_proposed_std_f64 - Alg. 1, the 'std' branch of the same two files (:29, :53; angles :29, :64) in float64: the gradient step
// on V is replaced by the least-squares solve v = U\(L\k), which for a K2 = kron(B.', A) of full column rank is
//                  V = pinv(A) K pinv(B)                                                                                (:53)
// two products of the shapes of A^H K and T B^H.  The factors come from the Hestenes route of pinv64.hip (pinv64.h), once per
// call - once for the batch when a factor is shared - or from the caller, who may hand them from one call to the next.  The
// rest of the iteration is the list above, kernel for kernel; G_A, G_B, the carried V, Res and RRes do not exist and
// convergence_error(:, 3) stays 0 (:6).  The two entries share one host frame, Admm64 below: parameters, the shared layout, the
// zeroing, head (Z, svt, X, K) and tail (A S B, C, V1, V2, convergence_error); each writes its own S-step between the two.
//
// jstsp_proposed_refresh_f64 - Alg. 2 with a support policy in its problem record (solver_common.h): at the refresh iterations the mask is the top of the
// solver's own new v, taken by the selection kernel of support_top.h between the gradient step and A S B - one launch for the
// batch, nothing read back, no vendor sort and none of its workspace inside the slab.  The body is admm64_approx; with no policy
// (every other entry) not one launch differs.
//  Asserted (tests/test_gpu_refresh64.py): without a refresh in the call the bits of jstsp_proposed_resume_f64; with one, the bits
//  of the chain of one-iteration calls with jstsp_support_order_f64 between them; legs; tests/refresh_ref.py within 1e-10 / 1e-8.
//
// jstsp_proposed_until_f64 - Alg. 2 that stops each trial when its own iterate has settled (the rule in its problem record):
// trial t stops after the first iteration i with i - it0 >= min_iters and convergence_error(i, 3) <= tol[t], the column that
// step_v64_kernel writes per trial in one workgroup.  The body is admm64_approx again, with four more kernels and nothing changed
// in the others:
//   stop test   one thread per slot after the iteration's tail: flag, iters and ce3_out through the slot -> trial map;
//   capture     the same iteration, for the slots whose flag was just set: S, the iteration's Y, the packed state and the order go
//               to the trial's own place in the outputs.  So a trial is CAPTURED AT THE ITERATION WHERE IT STOPS, whatever `check`
//               is; a stopped trial that runs on until the next compaction writes nothing more (its rows of ce stay NaN);
//   compact     every `check` iterations: an ordered ballot count over the flags gives each survivor's new slot and the active
//               count, the one int the host reads (one stream synchronisation per `check` iterations);
//   gather      one launch moves every per-trial array of the survivors to its new slot in a SHADOW set (never in place; the
//               caller's device inputs are only read), the host swaps the pointers and sizes every later launch to the count.
//               It runs when at least a sixteenth of the slots have stopped since the last one (UNTIL_GATHER_SHARE below).
// A trial's bits depend neither on its slot nor on its batch (min(N, M) <= 64), so they are those of the sibling run for that
// trial alone over iters[t] iterations.  With no positive tol nothing is read back and the launches added are the map's
// initialisation and the last iteration's test and capture.
#include "pinv64.h"
#include "solver_common.h"
#include "support_top.h"
#include "svt64.h"

#include <algorithm>
#include <climits>
#include <functional>
#include <vector>

namespace jstsp {
namespace {

struct Par64 {          // per-trial scalars, all derived in float64 from the caller's doubles
    double rho, ir, cc, tY, tS;
};

// fixed-order sum over the 256 threads of a workgroup
__device__ __forceinline__ double wg_sum(double v, double *sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- element-wise steps --------------------------------------------------------------------------------------------------------
inline dim3 egrid(long long per, int batch) { return dim3((unsigned)std::max<long long>(1, std::min<long long>((per + 255) / 256, 2048)), batch); }

// Z = X - V1 / rho                                                                                                       (:35)
__global__ __launch_bounds__(256) void form_z64_kernel(long long nm, const Par64 *par, const double2 *X, const double2 *V1, double2 *Z)
{
    const long long o = (long long)blockIdx.y * nm;
    const double ir = par[blockIdx.y].ir;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const double2 x = X[o + e], v = V1[o + e];
        Z[o + e] = make_double2(x.x - ir * v.x, x.y - ir * v.y);
    }
}

// X = (V1 + rho Y + subY + V2 + rho C + rho Xs) ./ (Omega + 2 rho);  K = X - V2/rho - C                                    (:38-43)
__global__ __launch_bounds__(256) void update_x64_kernel(long long nm, const Par64 *par, const double2 *V1, const double2 *Y, const double2 *subY,
                                                         const double2 *V2, const double2 *Cm, const double2 *Xs, const double *Omega, double2 *X,
                                                         double2 *K)
{
    const long long o = (long long)blockIdx.y * nm;
    const Par64 p = par[blockIdx.y];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const double2 v1 = V1[o + e], y = Y[o + e], sy = subY[o + e], v2 = V2[o + e], c = Cm[o + e], xs = Xs[o + e];
        const double invd = 1.0 / (Omega[o + e] + 2.0 * p.rho);
        const double2 x = make_double2((v1.x + p.rho * y.x + sy.x + v2.x + p.rho * c.x + p.rho * xs.x) * invd,
                                       (v1.y + p.rho * y.y + sy.y + v2.y + p.rho * c.y + p.rho * xs.y) * invd);
        X[o + e] = x;
        K[o + e] = make_double2(x.x - p.ir * v2.x - c.x, x.y - p.ir * v2.y - c.y);
    }
}

// C = rho/(rho+1) (X - Xs - V2/rho);  V1 += rho (Y - X);  V2 += rho (C - X + Xs)                                           (:61-65)
__global__ __launch_bounds__(256) void update_c64_kernel(long long nm, const Par64 *par, const double2 *X, const double2 *Xs, const double2 *Y,
                                                         double2 *Cm, double2 *V1, double2 *V2)
{
    const long long o = (long long)blockIdx.y * nm;
    const Par64 p = par[blockIdx.y];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const double2 x = X[o + e], xs = Xs[o + e], y = Y[o + e];
        double2 v1 = V1[o + e], v2 = V2[o + e];
        const double2 c = make_double2(p.cc * (x.x - xs.x - p.ir * v2.x), p.cc * (x.y - xs.y - p.ir * v2.y));
        v1.x += p.rho * (y.x - x.x); v1.y += p.rho * (y.y - x.y);
        v2.x += p.rho * (c.x - x.x + xs.x); v2.y += p.rho * (c.y - x.y + xs.y);
        Cm[o + e] = c; V1[o + e] = v1; V2[o + e] = v2;
    }
}

__global__ __launch_bounds__(256) void sub64_kernel(long long n, double2 *R, const double2 *Q)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double2 r = R[e], q = Q[e];
        R[e] = make_double2(r.x - q.x, r.y - q.y);
    }
}

// rank[e] = position of entry e (0-based) in indx_S (1-based linear indices, n per trial); an index outside 1 .. g is ignored
__global__ __launch_bounds__(256) void rank64_init_kernel(long long n, int32_t *rank)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) rank[e] = 0x7fffffff;
}
__global__ __launch_bounds__(256) void rank64_kernel(int g, int n, const int32_t *indx, int32_t *rank)
{
    const long long o = (long long)blockIdx.y * g, oi = (long long)blockIdx.y * n;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        const int32_t e = indx[oi + p] - 1;
        if (e >= 0 && e < g) atomicMin(&rank[o + e], p);
    }
}

// alpha = <Res, Res> / <Res, RRes> (complex);  V += alpha Res;  ce(i, 3) = |dV|^2 / |V_prev|^2;  S = soft(V, tau_S/rho) (.* mask)
// One workgroup per trial; every sum in a fixed order.                                                                     (:48-56, angles :68)
__global__ __launch_bounds__(256) void step_v64_kernel(int g, const Par64 *par, const double2 *Res, const double2 *RRes, double2 *V, double2 *S,
                                                       const int32_t *rank, int cnt, double *ce3)
{
    __shared__ double sh[4];
    const int t = blockIdx.x;
    const long long o = (long long)t * g;
    double nr = 0.0, dr = 0.0, di = 0.0, nv = 0.0;
    for (int e = threadIdx.x; e < g; e += 256) {
        const double2 r = Res[o + e], q = RRes[o + e], v = V[o + e];
        nr += r.x * r.x + r.y * r.y;
        dr += r.x * q.x + r.y * q.y;
        di += r.x * q.y - r.y * q.x;
        nv += v.x * v.x + v.y * v.y;
    }
    nr = wg_sum(nr, sh); dr = wg_sum(dr, sh); di = wg_sum(di, sh); nv = wg_sum(nv, sh);
    const double den = dr * dr + di * di;
    const double ar = den == 0.0 ? nr / 0.0 : nr * dr / den, ai = den == 0.0 ? 0.0 : -nr * di / den;
    const double ts = par[t].tS;
    double dv = 0.0;
    for (int e = threadIdx.x; e < g; e += 256) {
        const double2 r = Res[o + e];
        const double sr = ar * r.x - ai * r.y, si = ar * r.y + ai * r.x;
        double2 v = V[o + e];
        v.x += sr; v.y += si;
        dv += sr * sr + si * si;
        V[o + e] = v;
        const double mr = fmax(fabs(v.x) - ts, 0.0), mi = fmax(fabs(v.y) - ts, 0.0);
        double2 s = make_double2(v.x > 0.0 ? mr : (v.x < 0.0 ? -mr : 0.0), v.y > 0.0 ? mi : (v.y < 0.0 ? -mi : 0.0));      // sign(0) = 0
        if (rank && !(rank[o + e] < cnt)) s = make_double2(0.0, 0.0);
        S[o + e] = s;
    }
    dv = wg_sum(dv, sh);
    if (threadIdx.x == 0 && ce3) ce3[t] = dv / nv;              // Inf at i = 1 (V_prev = 0), NaN for 0 / 0 as the reference
}

// 'std': S = soft(V, tau_S/rho) (.* the cumulative mask of _angles), V = pinv(A) K pinv(B)                               (:56, angles :68)
__global__ __launch_bounds__(256) void soft_mask64_kernel(long long g, const Par64 *par, const double2 *V, double2 *S, const int32_t *rank, int cnt)
{
    const long long o = (long long)blockIdx.y * g;
    const double ts = par[blockIdx.y].tS;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g; e += (long long)gridDim.x * 256) {
        const double2 v = V[o + e];
        const double mr = fmax(fabs(v.x) - ts, 0.0), mi = fmax(fabs(v.y) - ts, 0.0);
        double2 s = make_double2(v.x > 0.0 ? mr : (v.x < 0.0 ? -mr : 0.0), v.y > 0.0 ? mi : (v.y < 0.0 ? -mi : 0.0));      // sign(0) = 0
        if (rank && !(rank[o + e] < cnt)) s = make_double2(0.0, 0.0);
        S[o + e] = s;
    }
}

__global__ void fill64_kernel(int n, double *p, double v)
{
    if ((int)threadIdx.x < n) p[threadIdx.x] = v;
}

// ce(i, 1) = lambda_max(V1) / lambda_max(X), ce(i, 2) = lambda_max(V2) / lambda_max(X); ce laid out Imax x 3 per trial
__global__ __launch_bounds__(256) void ce64_kernel(int batch, int Imax, int it, const double *lx, const double *l1, const double *l2, const double *ce3,
                                                   double *ce)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch) return;
    double *c = ce + (long long)t * 3 * Imax + it;
    c[0] = l1[t] / lx[t]; c[Imax] = l2[t] / lx[t]; c[2 * Imax] = ce3[t];
}

// ---- the state of a resumed call (jstsp.h: jstsp_admm_state_elems) ----------------------------------------------------------------
// One block per trial, [X | V1 | V2 | C] (nm each) then [V | S] (g each); the solver keeps each of the six as one array over the
// batch.  a[k]: the six arrays in the order of the block.
struct State64 {
    double2 *a[6];
};
__global__ __launch_bounds__(256) void state_unpack64_kernel(long long nm, long long g, const double2 *state, State64 w)
{
    const double2 *src = state + (long long)blockIdx.y * (4 * nm + 2 * g);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const long long len = k < 4 ? nm : g;
        double2 *dst = w.a[k] + (long long)blockIdx.y * len;
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < len; e += (long long)gridDim.x * 256) dst[e] = src[e];
        src += len;
    }
}
__global__ __launch_bounds__(256) void state_pack64_kernel(long long nm, long long g, State64 w, double2 *state)
{
    double2 *dst = state + (long long)blockIdx.y * (4 * nm + 2 * g);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const long long len = k < 4 ? nm : g;
        const double2 *src = w.a[k] + (long long)blockIdx.y * len;
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < len; e += (long long)gridDim.x * 256) dst[e] = src[e];
        dst += len;
    }
}

// ---- the stopping rule of jstsp_proposed_until_f64 ---------------------------------------------------------------------------------
// flag of a slot: 0 running, 1 stopped by this iteration (the capture kernel's cue), 2 stopped earlier and not yet compacted away
__global__ __launch_bounds__(256) void until_init64_kernel(int batch, long long nce, int32_t *map, int32_t *flag, double *ce)
{
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i0 < batch) { map[i0] = (int32_t)i0; flag[i0] = 0; }
    for (long long e = i0; e < nce; e += (long long)gridDim.x * 256) ce[e] = __builtin_nan("");
}

// ce(i, 1:3) of the running slots, through the map (the rows of a stopped trial stay NaN)
__global__ __launch_bounds__(256) void ce64_map_kernel(int nact, int Imax, int it, const double *lx, const double *l1, const double *l2, const double *ce3,
                                                       const int32_t *map, const int32_t *flag, double *ce)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nact || flag[s] != 0) return;
    double *c = ce + (long long)map[s] * 3 * Imax + it;
    c[0] = l1[s] / lx[s]; c[Imax] = l2[s] / lx[s]; c[2 * Imax] = ce3[s];
}

// after iteration k of the call (1-based): a running slot stops when k >= min_iters and ce3 <= tol (tol > 0; false for a NaN or
// an Inf on the left), or when the iteration was the call's last
__global__ __launch_bounds__(256) void until_test64_kernel(int nact, int k, int min_iters, int last, const double *ce3, const double *tol,
                                                           const int32_t *map, int32_t *flag, int32_t *iters, double *ce3_out)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nact) return;
    const int32_t f = flag[s];
    if (f == 1) flag[s] = 2;
    if (f != 0) return;
    const double c = ce3[s], tl = tol[s];
    if (!(last || (k >= min_iters && tl > 0.0 && c <= tl))) return;
    const int32_t t = map[s];
    flag[s] = 1; iters[t] = k;
    if (ce3_out) ce3_out[t] = c;
}

// the slots the test has just stopped: S, Y, the state block (state_pack64_kernel's layout) and the order, to trial map[slot]
__global__ __launch_bounds__(256) void until_capture64_kernel(long long nm, long long g, int R, State64 w, const double2 *Y, const int32_t *top, int have_top,
                                                              const int32_t *flag, const int32_t *map, double2 *S_out, double2 *Y_out, double2 *state,
                                                              int32_t *top_out)
{
    const int s = blockIdx.y;
    if (flag[s] != 1) return;
    const long long t = map[s], e0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    const double2 *Ss = w.a[5] + s * g;
    for (long long e = e0; e < g; e += step) S_out[t * g + e] = Ss[e];
    if (Y_out)
        for (long long e = e0; e < nm; e += step) Y_out[t * nm + e] = Y[s * nm + e];
    if (state) {
        double2 *dst = state + t * (4 * nm + 2 * g);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const long long len = k < 4 ? nm : g;
            const double2 *src = w.a[k] + s * len;
            for (long long e = e0; e < len; e += step) dst[e] = src[e];
            dst += len;
        }
    }
    if (top_out)
        for (long long e = e0; e < R; e += step) top_out[t * R + e] = have_top ? top[(long long)s * R + e] : 0;
}

// newslot[s] = the number of running slots below s (-1 for a stopped one), *count = the number of running slots; one workgroup
__global__ __launch_bounds__(ST_THREADS) void until_compact64_kernel(int nact, const int32_t *flag, int32_t *newslot, int32_t *count)
{
    __shared__ int wsum[2][ST_THREADS / 64];
    int base = 0;
    for (int c = 0; c < nact; c += ST_THREADS) {
        const int i = c + threadIdx.x;
        const bool keep = i < nact && flag[i] == 0;
        int r, r2, tot, tot2;
        st_block_rank2<ST_THREADS>(keep, false, wsum, r, r2, tot, tot2);
        if (i < nact) newslot[i] = keep ? base + r : -1;
        base += tot;
    }
    if (threadIdx.x == 0) *count = base;
}

// every per-trial array of the survivors from its slot to its new one, between two buffers (src != dst); one launch
struct GItem64 {
    const void *src; void *dst;
    long long n, stride;                // elements per trial, elements between trials
    int esz;                            // 16 (double2), 8 (double) or 4 (int32_t)
};
constexpr int UNTIL_ITEMS = 20;
// A gather streams every array of every survivor once - measured at BASELINE configs[1], 256 trials, about a sixth of an iteration
// (profiles/until64_rate.json) - while a stopped slot that runs on costs 1 / active of one per iteration: the survivors are moved
// only when at least one slot in UNTIL_GATHER_SHARE has stopped since the last gather.
constexpr int UNTIL_GATHER_SHARE = 16;
struct Gather64 {
    GItem64 it[UNTIL_ITEMS];
    int cnt;
};
template <class T>
__device__ __forceinline__ void gather_one(const GItem64 &q, long long from, long long to)
{
    const T *src = static_cast<const T *>(q.src) + from * q.stride;
    T *dst = static_cast<T *>(q.dst) + to * q.stride;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < q.n; e += (long long)gridDim.x * 256) dst[e] = src[e];
}
__global__ __launch_bounds__(256) void until_gather64_kernel(Gather64 gt, const int32_t *newslot)
{
    const int32_t to = newslot[blockIdx.y];
    if (to < 0) return;
    for (int k = 0; k < gt.cnt; ++k) {
        const GItem64 &q = gt.it[k];
        if (q.esz == 16) gather_one<double2>(q, blockIdx.y, to);
        else if (q.esz == 8) gather_one<double>(q, blockIdx.y, to);
        else gather_one<int32_t>(q, blockIdx.y, to);
    }
}

// elements of the scratch array that the split products of one solve share (the largest need among its products)
size_t solver_ws_elems(int N, int M, int Gr, int G2, int batch, int nA, int nB)
{
    size_t e = std::max(zgemm64_ws_elems(Gr, Gr, N, nA), zgemm64_ws_elems(G2, G2, M, nB));
    const int shp[6][3] = {{Gr, M, N}, {Gr, G2, M}, {Gr, G2, Gr}, {Gr, G2, G2}, {N, G2, Gr}, {N, M, G2}};
    for (const auto &q : shp) e = std::max(e, zgemm64_ws_elems(q[0], q[1], q[2], batch));
    return std::max<size_t>(1, e);
}

// What Alg. 2 ('approximate') and Alg. 1 ('std') share - everything of the iteration but the S-step.  An entry fills in the call,
// states its own arrays after layout() inside the same ws64_open() lambda (gws among them: it knows its products), and writes its
// S-step inline between head() and tail().
struct Admm64 {
    const AdmmProblem64 &p;                         // the call
    int batch;                                      // the trials still in the loop: the call's, until the stopping rule compacts them
    bool host;
    std::vector<Par64> hp;                          // the arrays: parameters, shared inputs, outputs, state of the iteration
    const Par64 *par; const double2 *subY, *A, *B; const double *Omega; const int32_t *indx = nullptr;
    double2 *Sd, *Yd, *X, *V1, *V2, *Cm, *Xs, *Y, *Z, *K, *T, *W, *gws = nullptr;
    double *ced, *lx, *l1, *l2, *ce3;
    int32_t *rank = nullptr;
    const int32_t *map = nullptr, *flag = nullptr;  // jstsp_proposed_until_f64: slot -> trial and the slots' flags (ce goes through them)
    Svt64 sv;

    explicit Admm64(const AdmmProblem64 &q) : p(q), batch(q.batch), host(q.memspace == JSTSP_HOST)
    {
        for (int t = 0; t < batch; ++t)
            hp.push_back(Par64{p.rho[t], 1.0 / p.rho[t], p.rho[t] / (p.rho[t] + 1.0), p.tau_Y[t] / p.rho[t], p.tau_S[t] / p.rho[t]});
    }
    bool angles() const { return p.indx_S != nullptr; }
    bool want_ce() const { return p.ce_out != nullptr; }
    Mat64 Am() const { return Mat64{A, p.strideA, p.N}; }
    Mat64 Bm() const { return Mat64{B, p.strideB, p.G2}; }
    dim3 gnm() const { return egrid((long long)p.nm(), batch); }
    int mask_count(int it) const { return (int)std::min<long long>(10 + 5ll * (it + 1), (long long)p.g()); }     // angles :36

    void layout(Slab &w, int b)
    {
        const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2;
        const size_t enm = p.nm() * b, eg = p.g() * b;
        par = w.in(hp.data(), b, true);
        subY = w.in(reinterpret_cast<const double2 *>(p.subY), enm, host);
        Omega = w.in(p.Omega, enm, host);
        A = w.in(reinterpret_cast<const double2 *>(p.A), dict_elems(p.strideA, (size_t)N * Gr, b), host);
        B = w.in(reinterpret_cast<const double2 *>(p.B), dict_elems(p.strideB, (size_t)G2 * M, b), host);
        if (angles()) indx = w.in(p.indx_S, p.listed() * b, host);
        Sd = w.out(reinterpret_cast<double2 *>(p.S_out), eg, host);
        Yd = w.out(reinterpret_cast<double2 *>(p.Y_out), enm, host);
        ced = w.out(p.ce_out, (size_t)3 * p.Imax * b, host);
        for (double2 **q : {&X, &V1, &V2, &Cm, &Xs, &Y, &Z, &K}) *q = w.get<double2>(enm);
        T = w.get<double2>((size_t)Gr * M * b); W = w.get<double2>((size_t)N * G2 * b);
        if (angles() || p.policy) rank = w.get<int32_t>(eg);          // (the refreshed solve: a rank array even without indx_S)
        for (double **q : {&lx, &l1, &l2, &ce3}) *q = w.get<double>(b);
        sv.layout(w, N, M, b);
    }
    // X = V1 = V2 = C = Xs = 0; the rank of every entry in indx_S (_angles)
    int begin(hipStream_t st)
    {
        const size_t g = p.g() * batch;
        for (double2 *q : {X, V1, V2, Cm, Xs}) JSTSP_HIP(hipMemsetAsync(q, 0, p.nm() * batch * sizeof(double2), st));
        if (angles()) {
            hipLaunchKernelGGL(rank64_init_kernel, dim3((unsigned)std::min<size_t>((g + 255) / 256, 4096)), dim3(256), 0, st, (long long)g, rank);
            hipLaunchKernelGGL(rank64_kernel, egrid((long long)p.listed(), batch), dim3(256), 0, st, (int)p.g(), (int)p.listed(), indx, rank);
        }
        return 0;
    }
    // Z, Y = svt(Z), X; leaves K = X - V2/rho - C for the S-step                                                           (:35-43)
    int head(hipStream_t st)
    {
        hipLaunchKernelGGL(form_z64_kernel, gnm(), dim3(256), 0, st, (long long)p.nm(), par, X, V1, Z);
        JSTSP_TRY(sv.apply(st, Z, &par->tY, (long long)(sizeof(Par64) / sizeof(double)), Y));          // :35
        hipLaunchKernelGGL(update_x64_kernel, gnm(), dim3(256), 0, st, (long long)p.nm(), par, V1, Y, subY, V2, Cm, Xs, Omega, X, K);
        return 0;
    }
    // Xs = A S B by two products
    int synthesize(hipStream_t st, const double2 *S)
    {
        const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2;
        JSTSP_TRY(zgemm64(st, 'N', 'N', N, G2, Gr, batch, Am(), Mat64{S, (long long)p.g(), Gr}, W, (long long)N * G2, N, gws));      // A S
        return zgemm64(st, 'N', 'N', N, M, G2, batch, Mat64{W, (long long)N * G2, N}, Bm(), Xs, (long long)p.nm(), N, gws);          // ... B
    }
    // Xs = A S B, C, V1, V2 and row `it` of convergence_error (its third column is what ce3 holds)                          (:58-69)
    int tail(hipStream_t st, const double2 *S, int it)
    {
        JSTSP_TRY(synthesize(st, S));
        hipLaunchKernelGGL(update_c64_kernel, gnm(), dim3(256), 0, st, (long long)p.nm(), par, X, Xs, Y, Cm, V1, V2);
        if (want_ce()) {
            JSTSP_TRY(sv.lambda_max(st, X, lx));
            JSTSP_TRY(sv.lambda_max(st, V1, l1));
            JSTSP_TRY(sv.lambda_max(st, V2, l2));
            if (map) hipLaunchKernelGGL(ce64_map_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, p.Imax, it, lx, l1, l2, ce3, map, flag, ced);
            else hipLaunchKernelGGL(ce64_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, p.Imax, it, lx, l1, l2, ce3, ced);
        }
        JSTSP_HIP(hipGetLastError());
        return 0;
    }
    // Y to the caller; for a host call S (in Sd by now), Y and convergence_error go back and the stream is synchronised
    int deliver(const Slab &s)
    {
        const size_t nm = p.nm() * batch;
        if (p.Y_out) JSTSP_HIP(hipMemcpyAsync(Yd, Y, nm * sizeof(double2), hipMemcpyDeviceToDevice, s.st));
        if (host) {
            JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(p.S_out), Sd, p.g() * batch));
            if (p.Y_out) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(p.Y_out), Yd, nm));
            if (want_ce()) JSTSP_TRY(s.copy_back(p.ce_out, ced, (size_t)3 * p.Imax * batch));
            JSTSP_HIP(hipStreamSynchronize(s.st));
        }
        return 0;
    }
    // ---- a resumed call (jstsp_proposed_resume_f64, jstsp_proposed_std_resume_f64) ----
    // X, V1, V2, C, V, S from the caller's state and Xs = A S B by the two products of tail(): what begin() zeroes, loaded
    int load_state(hipStream_t st, const double2 *state, double2 *V, double2 *S)
    {
        hipLaunchKernelGGL(state_unpack64_kernel, gnm(), dim3(256), 0, st, (long long)p.nm(), (long long)p.g(), state, State64{{X, V1, V2, Cm, V, S}});
        JSTSP_HIP(hipGetLastError());
        return synthesize(st, S);
    }
    int store_state(hipStream_t st, double2 *state, double2 *V, double2 *S)
    {
        hipLaunchKernelGGL(state_pack64_kernel, gnm(), dim3(256), 0, st, (long long)p.nm(), (long long)p.g(), State64{{X, V1, V2, Cm, V, S}}, state);
        JSTSP_HIP(hipGetLastError());
        return 0;
    }
};

// the limits the two entries share
int admm64_limits(const char *nmf, int N, int M, int Gr, int G2, int batch)
{
    JSTSP_REQUIRE(std::min(N, M) <= P64_MAX_ORDER, JSTSP_E_UNSUPPORTED, "%s: min(N, M) = %d: the float64 eigen-decomposition is limited to order %d", nmf,
                  std::min(N, M), P64_MAX_ORDER);
    JSTSP_REQUIRE((long long)Gr * G2 < (1ll << 31) && (long long)N * M < (1ll << 31) && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: more than 2^31 entries per trial or more than 65535 trials", nmf);
    return 0;
}

// One per-trial array that a compaction moves: `cur` is the pointer the loop uses (the caller's own array for a device input until
// the first gather), alt the buffer the next gather writes, spare the second buffer of an array whose first `cur` is not the slab's.
struct Shadow64 {
    std::function<const void *()> cur;
    std::function<void(void *)> set;
    void *alt, *spare;
    long long n, stride; int esz;
    bool owned;                                     // cur points into the slab: it becomes the next alt
    GItem64 item() const { return GItem64{cur(), alt, n, stride, esz}; }
    void swap()
    {
        void *old = const_cast<void *>(cur());
        set(alt);
        alt = owned ? old : spare;
        owned = true;
    }
};
template <class T> Shadow64 shadow_of(T *&p, void *alt, void *spare, long long n, long long stride, int esz, bool owned)
{
    return Shadow64{[&p] { return static_cast<const void *>(p); }, [&p](void *q) { p = static_cast<T *>(q); }, alt, spare, n, stride, esz, owned};
}

// Alg. 2 ('approximate'), the body of jstsp_proposed_algorithm_f64 (it0 = 0, no state), of jstsp_proposed_resume_f64, - with a
// support policy in the record - of jstsp_proposed_refresh_f64 and - with a stopping rule in it - of jstsp_proposed_until_f64 (the
// head of this file says what each adds): iterations it0 + 1 .. it0 + Imax from state_in, or from zero.  At a refresh iteration - a
// function of the GLOBAL index, p.refresh_at(), never of a call boundary - the gradient step runs without a mask, the selection
// kernel of support_top.h ranks the top R entries of the new v, and soft_mask64_kernel rewrites S from the stored v under that rank:
// the expression of step_v64_kernel on the value it stored, hence the bits a masked step would have written.  nmf names the entry in
// every message; std_entry is where its 'std' refusal points.
int admm64_approx(jstsp_ctx *ctx, const char *nmf, const char *std_entry, const AdmmProblem64 &p)
{
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2, batch = p.batch, Imax = p.Imax, it0 = p.it0;
    const long long strideA = p.strideA, strideB = p.strideB;
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(p.memspace == JSTSP_HOST || p.memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", p.memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0 && Imax > 0 && strideA >= 0 && strideB >= 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE(p.subY && p.Omega && p.A && p.B && p.tau_Y && p.tau_S && p.rho && p.S_out, JSTSP_E_NULL, "%s: NULL argument", nmf);
    JSTSP_REQUIRE(p.type == JSTSP_TYPE_APPROXIMATE || p.type == JSTSP_TYPE_STD, JSTSP_E_ARG, "%s: bad type %d", nmf, p.type);
    JSTSP_REQUIRE(p.type == JSTSP_TYPE_APPROXIMATE, JSTSP_E_UNSUPPORTED,
                  "%s: 'std' has no float64 path (its least-squares solve is fp32 work): use %s", nmf, std_entry);
    JSTSP_TRY(check_resumed(nmf, p));
    JSTSP_TRY(admm64_limits(nmf, N, M, Gr, G2, batch));
    if (p.policy) JSTSP_TRY(check_policy(nmf, p));
    if (p.rule) {
        JSTSP_TRY(check_rule_arrays(nmf, p));
        JSTSP_TRY(check_rule_counts(nmf, p));
        if (!p.policy) JSTSP_TRY(check_rule_list(nmf, p));
    }
    const bool un = p.rule, rule_on = p.live();                     // live: some tol is positive, trials can stop and the loop compacts
    Admm64 f(p);
    hipStream_t st = ctx->stream;
    const size_t g1 = p.g();
    const int nA = strideA ? batch : 1, nB = strideB ? batch : 1;
    const int R = (int)p.R();                                       // entries of a refreshed order
    int32_t *top = nullptr;                                         // the list of the call's last refresh, for indx_out
    const bool want_top = p.indx_out && p.runs_refresh();

    double2 *V, *S, *Res, *RRes, *T2, *GA, *GB, *sout = nullptr;
    const double2 *sin = nullptr;
    // the stopping rule's arrays: tol, slot -> trial, flags, new slots, the active count; the outputs; the order by slot and by trial
    const double *tolp = nullptr;
    int32_t *map = nullptr, *flag = nullptr, *newslot = nullptr, *count = nullptr, *itd = nullptr, *top_out = nullptr;
    double *c3d = nullptr;
    std::vector<Shadow64> sh;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nmf, batch, [&](Slab &w, int b) {
        const int bA = strideA ? b : 1, bB = strideB ? b : 1;
        f.layout(w, b);
        for (double2 **p : {&V, &S, &Res, &RRes, &T2}) *p = w.get<double2>(g1 * b);
        GA = w.get<double2>((size_t)Gr * Gr * bA); GB = w.get<double2>((size_t)G2 * G2 * bB);
        f.gws = w.get<double2>(solver_ws_elems(N, M, Gr, G2, b, bA, bB));
        if (p.state_in) sin = w.in(reinterpret_cast<const double2 *>(p.state_in), p.state_elems() * b, f.host);
        if (p.state_out) sout = w.out(reinterpret_cast<double2 *>(p.state_out), p.state_elems() * b, f.host);
        if (want_top) top = w.out(p.indx_out, (size_t)R * b, f.host);
        if (!un) return;
        tolp = w.in(p.tol, b, true);
        for (int32_t **p : {&map, &flag, &newslot}) *p = w.get<int32_t>(b);
        count = w.get<int32_t>(1);
        itd = w.out(p.iters_out, b, f.host);
        if (p.ce3_out) c3d = w.out(p.ce3_out, b, f.host);
        if (want_top) { top_out = top; top = w.get<int32_t>((size_t)R * b); }   // the loop's list is by slot; the caller's by trial
        if (!rule_on) return;
        // the shadow set of a compaction: every array that lives from one iteration to the next, and the inputs
        sh.clear();
        const long long nm = (long long)p.nm(), gl = (long long)g1;
        auto add = [&](auto *&p, long long n, long long stride, size_t total, int esz, bool owned) {
            const size_t words = (total * esz + 15) / 16;
            void *alt = w.get<double2>(words), *spare = owned ? nullptr : (void *)w.get<double2>(words);
            sh.push_back(shadow_of(p, alt, spare, n, stride, esz, owned));
        };
        for (double2 **p : {&f.X, &f.V1, &f.V2, &f.Cm, &f.Xs}) add(*p, nm, nm, (size_t)nm * b, 16, true);
        for (double2 **p : {&V, &S}) add(*p, gl, gl, (size_t)gl * b, 16, true);
        add(f.subY, nm, nm, (size_t)nm * b, 16, f.host);
        add(f.Omega, nm, nm, (size_t)nm * b, 8, f.host);
        add(f.par, 5, 5, (size_t)5 * b, 8, true);
        add(tolp, 1, 1, b, 8, true);
        add(map, 1, 1, b, 4, true);
        if (f.angles() || p.policy) add(f.rank, gl, gl, (size_t)gl * b, 4, true);
        if (want_top) add(top, R, R, (size_t)R * b, 4, true);
        if (strideA) {
            add(f.A, (long long)N * Gr, strideA, dict_elems(strideA, (size_t)N * Gr, b), 16, f.host);
            add(GA, (long long)Gr * Gr, (long long)Gr * Gr, (size_t)Gr * Gr * b, 16, true);
        }
        if (strideB) {
            add(f.B, (long long)G2 * M, strideB, dict_elems(strideB, (size_t)G2 * M, b), 16, f.host);
            add(GB, (long long)G2 * G2, (long long)G2 * G2, (size_t)G2 * G2 * b, 16, true);
        }
    }));
    static_assert(sizeof(Par64) == 5 * sizeof(double), "the gather moves a Par64 as five doubles");
    JSTSP_HIP(hipStreamSynchronize(st));            // (f.hp and tol are read from the host: copied before the call returns on any path)

    if (!sin) JSTSP_HIP(hipMemsetAsync(V, 0, g1 * batch * sizeof(double2), st));
    JSTSP_TRY(f.begin(st));
    if (sin) JSTSP_TRY(f.load_state(st, sin, V, S));               // (state_out may be state_in: read whole before anything is written)
    const long long sNM = (long long)p.nm(), sG = (long long)g1, sGA = strideA ? (long long)Gr * Gr : 0, sGB = strideB ? (long long)G2 * G2 : 0;
    double2 *T = f.T, *gws = f.gws;
    JSTSP_TRY(zgemm64(st, 'C', 'N', Gr, Gr, N, nA, f.Am(), f.Am(), GA, (long long)Gr * Gr, Gr, gws));      // G_A = A^H A
    JSTSP_TRY(zgemm64(st, 'N', 'C', G2, G2, M, nB, f.Bm(), f.Bm(), GB, (long long)G2 * G2, G2, gws));      // G_B = B B^H
    if (un) {
        hipLaunchKernelGGL(until_init64_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch,
                           f.want_ce() ? (long long)3 * Imax * batch : 0ll, map, flag, f.ced);
        f.map = map; f.flag = flag;
    }
    bool in_force = f.angles();                                     // a rank masks S: that of indx_S, then that of the last refresh
    bool listed = false;                                            // the call has run a refresh: `top` holds a list
    for (int it = 0; it < Imax; ++it) {
        const bool fresh = p.refresh_at((long long)it0 + it + 1);
        const int batch = f.batch;                                  // the trials still in the loop (the call's batch without a rule)
        const size_t g = g1 * batch;
        const Mat64 Am = f.Am(), Bm = f.Bm(), GAm{GA, sGA, Gr}, GBm{GB, sGB, G2};
        JSTSP_TRY(f.head(st));
        JSTSP_TRY(zgemm64(st, 'C', 'N', Gr, M, N, batch, Am, Mat64{f.K, sNM, N}, T, (long long)Gr * M, Gr, gws));      // A^H K
        JSTSP_TRY(zgemm64(st, 'N', 'C', Gr, G2, M, batch, Mat64{T, (long long)Gr * M, Gr}, Bm, Res, sG, Gr, gws));     // ... B^H
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, Gr, batch, GAm, Mat64{V, sG, Gr}, T2, sG, Gr, gws));                   // G_A V
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, G2, batch, Mat64{T2, sG, Gr}, GBm, RRes, sG, Gr, gws));                // ... G_B
        hipLaunchKernelGGL(sub64_kernel, dim3((unsigned)std::min<size_t>((g + 255) / 256, 4096)), dim3(256), 0, st, (long long)g, Res, RRes);
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, Gr, batch, GAm, Mat64{Res, sG, Gr}, T2, sG, Gr, gws));                 // G_A Res
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, G2, batch, Mat64{T2, sG, Gr}, GBm, RRes, sG, Gr, gws));                // ... G_B
        hipLaunchKernelGGL(step_v64_kernel, dim3(batch), dim3(256), 0, st, (int)g1, f.par, Res, RRes, V, S,
                           in_force && !fresh ? f.rank : (const int32_t *)nullptr, f.mask_count(it0 + it), f.want_ce() || un ? f.ce3 : nullptr);
        if (fresh) {                                                // the order of the new v, and S again under it
            hipLaunchKernelGGL(support_top_kernel<double2>, dim3(batch), dim3(ST_THREADS), 0, st, (int)g1, R, V, top, f.rank);
            hipLaunchKernelGGL(soft_mask64_kernel, egrid((long long)g1, batch), dim3(256), 0, st, (long long)g1, f.par, V, S, f.rank,
                               f.mask_count(it0 + it));
            in_force = listed = true;
        }
        JSTSP_TRY(f.tail(st, S, it));
        if (!un) continue;
        // ---- the stopping rule: test, capture what has just stopped, and every `check` iterations compact the survivors ----
        const bool last = it == Imax - 1;
        if (!rule_on && !last) continue;                            // no trial can stop before the last iteration
        hipLaunchKernelGGL(until_test64_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, it + 1, p.min_iters, (int)last, f.ce3, tolp, map,
                           flag, itd, c3d);
        // (few workgroups per slot: in most iterations every one of them only reads its flag)
        hipLaunchKernelGGL(until_capture64_kernel, dim3(std::min(egrid((long long)std::max(p.nm(), g1), 1).x, 64u), batch), dim3(256), 0, st, sNM, sG, R,
                           State64{{f.X, f.V1, f.V2, f.Cm, V, S}}, f.Y, top, (int)listed, flag, map, f.Sd, p.Y_out ? f.Yd : (double2 *)nullptr, sout,
                           top_out);
        JSTSP_HIP(hipGetLastError());
        if (last || (it + 1) % p.check) continue;
        int32_t left = 0;                                           // the one number that comes back, once per `check` iterations
        hipLaunchKernelGGL(until_compact64_kernel, dim3(1), dim3(ST_THREADS), 0, st, batch, flag, newslot, count);
        JSTSP_HIP(hipMemcpyAsync(&left, count, sizeof left, hipMemcpyDeviceToHost, st));
        JSTSP_HIP(hipStreamSynchronize(st));
        if (left == 0) break;                                       // every trial has stopped and is captured
        if ((batch - left) * UNTIL_GATHER_SHARE < batch) continue;  // too few have stopped to pay for moving the others
        Gather64 gt;
        gt.cnt = 0;
        for (const Shadow64 &q : sh) gt.it[gt.cnt++] = q.item();
        hipLaunchKernelGGL(until_gather64_kernel, egrid((long long)std::max(p.nm(), g1), batch), dim3(256), 0, st, gt, newslot);
        JSTSP_HIP(hipGetLastError());
        for (Shadow64 &q : sh) q.swap();
        JSTSP_HIP(hipMemsetAsync(flag, 0, (size_t)left * sizeof(int32_t), st));
        f.map = map; f.batch = f.sv.batch = left;
    }
    if (un) {                                       // every trial was captured into the outputs at its own last iteration
        if (f.host) {
            JSTSP_TRY(s.copy_back(p.iters_out, itd, (size_t)batch));
            if (c3d) JSTSP_TRY(s.copy_back(p.ce3_out, c3d, (size_t)batch));
            if (top_out) JSTSP_TRY(s.copy_back(p.indx_out, top_out, (size_t)R * batch));
            if (sout) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(p.state_out), sout, p.state_elems() * batch));
            JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(p.S_out), f.Sd, g1 * batch));
            if (p.Y_out) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(p.Y_out), f.Yd, p.nm() * batch));
            if (f.want_ce()) JSTSP_TRY(s.copy_back(p.ce_out, f.ced, (size_t)3 * Imax * batch));
            JSTSP_HIP(hipStreamSynchronize(st));
        }
        return 0;
    }
    const size_t g = g1 * batch;
    JSTSP_HIP(hipMemcpyAsync(f.Sd, S, g * sizeof(double2), hipMemcpyDeviceToDevice, st));
    if (sout) JSTSP_TRY(f.store_state(st, sout, V, S));
    if (sout && f.host) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(p.state_out), sout, p.state_elems() * batch));
    if (top && f.host) JSTSP_TRY(s.copy_back(p.indx_out, top, (size_t)R * batch));
    return f.deliver(s);
}

// One side of Alg. 1's least-squares step: the rank and rcond of the cnt factors the call inverted (rk NULL: the caller gave pinv).
// A factor that holds a NaN or is not of full column rank ends the call.
int inverted64_check(hipStream_t st, const char *nmf, const char *side, int cnt, int full, int batch, const double *rc, const int32_t *rk)
{
    if (!rk) return 0;
    std::vector<int32_t> hk(cnt);
    std::vector<double> hr(cnt);
    JSTSP_HIP(hipMemcpyAsync(hk.data(), rk, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    JSTSP_HIP(hipMemcpyAsync(hr.data(), rc, cnt * sizeof(double), hipMemcpyDeviceToHost, st));
    JSTSP_HIP(hipStreamSynchronize(st));
    const char *shared = cnt == 1 && batch > 1 ? " (shared by the batch)" : "";
    for (int t = 0; t < cnt; ++t) {
        JSTSP_REQUIRE(hr[t] == hr[t], JSTSP_E_ILLCOND, "%s: factor %s of trial %d%s holds a NaN or Inf", nmf, side, t, shared);
        JSTSP_REQUIRE(hk[t] >= full, JSTSP_E_ILLCOND,
                      "%s: factor %s of trial %d%s has rank %d < %d (rcond of the kept part %.3g): K2 = kron(B.', A) is not of full column rank", nmf,
                      side, t, shared, (int)hk[t], full, hr[t]);
    }
    return 0;
}
// its entry of rcond_out: the smallest rcond over the factors the call inverted, NaN for a side that was given
int rcond64_fill(hipStream_t st, int cnt, const double *rc, double *dst)
{
    if (rc) return pinv64_min(st, cnt, rc, dst);
    hipLaunchKernelGGL(fill64_kernel, dim3(1), dim3(64), 0, st, 1, dst, __builtin_nan(""));
    return 0;
}

// Alg. 1 ('std'), the body of jstsp_proposed_std_f64 (it0 = 0, no state) and of jstsp_proposed_std_resume_f64; PA_, PB_: the caller's
// least-squares factors, or NULL
int admm64_std(jstsp_ctx *ctx, const char *nmf, const AdmmProblem64 &p, const jstsp_c64 *PA_, const jstsp_c64 *PB_, double *rcond_out)
{
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2, batch = p.batch, Imax = p.Imax, it0 = p.it0;
    const long long strideA = p.strideA, strideB = p.strideB;
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(p.memspace == JSTSP_HOST || p.memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", p.memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0 && Imax > 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE(p.subY && p.Omega && p.A && p.B && p.tau_Y && p.tau_S && p.rho && p.S_out, JSTSP_E_NULL, "%s: NULL argument", nmf);
    JSTSP_REQUIRE((strideA == 0 || strideA >= (long long)N * Gr) && (strideB == 0 || strideB >= (long long)G2 * M), JSTSP_E_SHAPE,
                  "%s: a factor stride is 0 (shared) or at least the size of one factor", nmf);
    JSTSP_REQUIRE(N >= Gr && M >= G2, JSTSP_E_UNSUPPORTED,
                  "%s: K2 = kron(B.', A) must have full column rank (N >= Gr, M >= G2); the under-determined U\\(L\\k) of the reference "
                  "returns a basic, not least-squares, solution", nmf);
    JSTSP_TRY(check_resumed(nmf, p));
    JSTSP_TRY(admm64_limits(nmf, N, M, Gr, G2, batch));
    JSTSP_REQUIRE((PA_ || pinv64_shape_ok(N, Gr)) && (PB_ || pinv64_shape_ok(G2, M)), JSTSP_E_UNSUPPORTED,
                  "%s: A %d x %d, B %d x %d: a factor the call inverts needs min(rows, cols) <= %d and max(rows, cols) <= %d", nmf, N, Gr, G2, M,
                  PV_MAX_ORDER, PV_MAX_LONG);
    Admm64 f(p);
    const bool host = f.host;
    hipStream_t st = ctx->stream;
    const size_t g1 = p.g();
    const int nA = strideA ? batch : 1, nB = strideB ? batch : 1;

    const double2 *PA, *PB;
    double2 *V, *PAc = nullptr, *PBc = nullptr, *sout = nullptr;
    const double2 *sin = nullptr;
    double *rcA = nullptr, *rcB = nullptr, *rcd;
    int32_t *rkA = nullptr, *rkB = nullptr;
    Pinv64 pvA, pvB;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nmf, batch, [&](Slab &w, int b) {
        const int bA = strideA ? b : 1, bB = strideB ? b : 1;
        f.layout(w, b);
        if (PA_) PA = w.in(reinterpret_cast<const double2 *>(PA_), (size_t)Gr * N * bA, host);
        else {
            PA = PAc = w.get<double2>((size_t)Gr * N * bA); rcA = w.get<double>(bA); rkA = w.get<int32_t>(bA);
            pvA.layout(w, N, Gr, bA);
        }
        if (PB_) PB = w.in(reinterpret_cast<const double2 *>(PB_), (size_t)M * G2 * bB, host);
        else {
            PB = PBc = w.get<double2>((size_t)M * G2 * bB); rcB = w.get<double>(bB); rkB = w.get<int32_t>(bB);
            pvB.layout(w, G2, M, bB);
        }
        rcd = w.out(rcond_out, 2, host);
        V = w.get<double2>(g1 * b);
        const int shp[4][3] = {{Gr, M, N}, {Gr, G2, M}, {N, G2, Gr}, {N, M, G2}};
        size_t e = 1;
        for (const auto &q : shp) e = std::max(e, zgemm64_ws_elems(q[0], q[1], q[2], b));
        f.gws = w.get<double2>(e);
        if (p.state_in) sin = w.in(reinterpret_cast<const double2 *>(p.state_in), p.state_elems() * b, host);
        if (p.state_out) sout = w.out(reinterpret_cast<double2 *>(p.state_out), p.state_elems() * b, host);
    }));
    JSTSP_HIP(hipStreamSynchronize(st));            // (f.hp is this call's own: copied before it goes out of scope on any path)

    // the factors: a shared one is inverted once for the call; one that is not of full column rank ends the call
    if (PAc) JSTSP_TRY(pinv64_run(st, pvA, N, Gr, nA, f.A, strideA, PAc, rcA, rkA));
    if (PBc) JSTSP_TRY(pinv64_run(st, pvB, G2, M, nB, f.B, strideB, PBc, rcB, rkB));
    JSTSP_TRY(inverted64_check(st, nmf, "A", nA, Gr, batch, rcA, rkA));
    JSTSP_TRY(inverted64_check(st, nmf, "B", nB, G2, batch, rcB, rkB));
    if (rcond_out) {
        JSTSP_TRY(rcond64_fill(st, nA, rcA, rcd));
        JSTSP_TRY(rcond64_fill(st, nB, rcB, rcd + 1));
        JSTSP_HIP(hipGetLastError());
    }

    JSTSP_HIP(hipMemsetAsync(f.ce3, 0, batch * sizeof(double), st));                                   // convergence_error(:, 3) = 0 (:6)
    JSTSP_TRY(f.begin(st));
    // (Alg. 1 does not carry V - :53 recomputes it: the V of the state is loaded and overwritten by the first iteration)
    if (sin) JSTSP_TRY(f.load_state(st, sin, V, f.Sd));            // (state_out may be state_in: read whole before anything is written)
    const long long sNM = (long long)p.nm(), sG = (long long)g1;
    const Mat64 PAm{PA, strideA ? (long long)Gr * N : 0, Gr}, PBm{PB, strideB ? (long long)M * G2 : 0, M};
    for (int it = 0; it < Imax; ++it) {
        JSTSP_TRY(f.head(st));
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, M, N, batch, PAm, Mat64{f.K, sNM, N}, f.T, (long long)Gr * M, Gr, f.gws));     // pinv(A) K
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, M, batch, Mat64{f.T, (long long)Gr * M, Gr}, PBm, V, sG, Gr, f.gws));      // ... pinv(B)   (:53)
        hipLaunchKernelGGL(soft_mask64_kernel, egrid((long long)g1, batch), dim3(256), 0, st, (long long)g1, f.par, V, f.Sd, f.rank,
                           f.mask_count(it0 + it));
        JSTSP_TRY(f.tail(st, f.Sd, it));
    }
    if (host && rcond_out) JSTSP_TRY(s.copy_back(rcond_out, rcd, 2));
    if (sout) JSTSP_TRY(f.store_state(st, sout, V, f.Sd));
    if (sout && host) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(p.state_out), sout, p.state_elems() * batch));
    return f.deliver(s);
}

}  // namespace
}  // namespace jstsp

using namespace jstsp;

extern "C" {

int jstsp_svt_f64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *Y_, const double *tau, jstsp_c64 *X_, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(Mr > 0 && Mt > 0 && batch > 0, JSTSP_E_SHAPE, "svt (float64): bad shape");
    JSTSP_REQUIRE(Y_ && tau && X_, JSTSP_E_NULL, "svt (float64): NULL argument");
    JSTSP_REQUIRE(std::min(Mr, Mt) <= P64_MAX_ORDER && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "svt (float64): min(Mr, Mt) = %d, batch = %d: the float64 eigen-decomposition is limited to order %d (batch 65535)", std::min(Mr, Mt), batch,
                  P64_MAX_ORDER);
    hipStream_t st = ctx->stream;
    const bool host = memspace == JSTSP_HOST;
    const size_t nm = (size_t)Mr * Mt * batch;
    const double *thr;
    const double2 *Y;
    double2 *X;
    Svt64 sv;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, "svt (float64)", batch, [&](Slab &w, int b) {
        const size_t e = (size_t)Mr * Mt * b;
        thr = w.in(tau, b, true);
        Y = w.in(reinterpret_cast<const double2 *>(Y_), e, host);
        X = w.out(reinterpret_cast<double2 *>(X_), e, host);
        sv.layout(w, Mr, Mt, b);
    }));
    JSTSP_TRY(sv.apply(st, Y, thr, 1, X));
    if (host) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(X_), X, nm));
    JSTSP_HIP(hipStreamSynchronize(st));            // (also for a device call: tau was read from the caller's host array)
    return 0;
}

// The six ADMM entries: each fills a problem record (solver_common.h) and calls its body.
#define ADMM64_RECORD(type_, it0_, state_in_, state_out_)                                                                                   \
    AdmmProblem64 p{N, M, Gr, G2, batch, subY_, Omega_, A_, B_, tau_Y, tau_S, rho, strideA, strideB, Imax, type_, indx_S_, S_out, Y_out, ce_out, \
                    it0_, state_in_, state_out_, memspace}

int jstsp_proposed_algorithm_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                                 const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, int Imax, const double *tau_Y,
                                 const double *tau_S, const double *rho, int type, const int32_t *indx_S_, jstsp_c64 *S_out, jstsp_c64 *Y_out,
                                 double *ce_out, int memspace)
{
    ADMM64_RECORD(type, 0, nullptr, nullptr);
    return admm64_approx(ctx, "proposed_algorithm (float64)", "jstsp_proposed_algorithm_c64", p);
}

int jstsp_proposed_std_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                           const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, const jstsp_c64 *PA_,
                           const jstsp_c64 *PB_, int Imax, const double *tau_Y, const double *tau_S, const double *rho,
                           const int32_t *indx_S_, jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, double *rcond_out, int memspace)
{
    ADMM64_RECORD(JSTSP_TYPE_STD, 0, nullptr, nullptr);
    return admm64_std(ctx, "proposed_algorithm 'std' (float64)", p, PA_, PB_, rcond_out);
}

// elements of one trial's state block: [X | V1 | V2 | C] (N M each) then [v | S] (Gr G2 each); 0 for a bad shape
size_t jstsp_admm_state_elems(int N, int M, int Gr, int G2)
{
    if (N <= 0 || M <= 0 || Gr <= 0 || G2 <= 0) return 0;
    return 4 * (size_t)N * M + 2 * (size_t)Gr * G2;
}

// ---- the two solvers above, resumed: the same two bodies, admm64_approx and admm64_std, from the caller's it0 and state ----
int jstsp_proposed_resume_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                              const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, int Imax, const double *tau_Y,
                              const double *tau_S, const double *rho, int type, const int32_t *indx_S_, jstsp_c64 *S_out, jstsp_c64 *Y_out,
                              double *ce_out, int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out, int memspace)
{
    ADMM64_RECORD(type, it0, state_in, state_out);
    return admm64_approx(ctx, "proposed_algorithm resume (float64)", "jstsp_proposed_std_resume_f64", p);
}

// Alg. 2 with the support refreshed from its own iterate (the record's policy); the limit of a refreshed order is ST_MAX entries
int jstsp_proposed_refresh_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                               const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, int Imax, const double *tau_Y,
                               const double *tau_S, const double *rho, const int32_t *indx_S_, int n_indx, int refresh_start,
                               int refresh_period, jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, int it0, const jstsp_c64 *state_in,
                               jstsp_c64 *state_out, int32_t *indx_out, int memspace)
{
    ADMM64_RECORD(JSTSP_TYPE_APPROXIMATE, it0, state_in, state_out);
    p.set_policy(n_indx, refresh_start, refresh_period, indx_out);
    return admm64_approx(ctx, "proposed_algorithm refresh (float64)", "jstsp_proposed_std_resume_f64", p);
}

// Alg. 2 that stops each trial when its own iterate has settled (the record's rule); refresh_period < 0: no support policy
int jstsp_proposed_until_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                             const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, int Imax, const double *tau_Y,
                             const double *tau_S, const double *rho, const int32_t *indx_S_, int n_indx, int refresh_start, int refresh_period,
                             const double *tol, int min_iters, int check, jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, int it0,
                             const jstsp_c64 *state_in, jstsp_c64 *state_out, int32_t *indx_out, int32_t *iters_out, double *ce3_out, int memspace)
{
    ADMM64_RECORD(JSTSP_TYPE_APPROXIMATE, it0, state_in, state_out);
    p.n_indx = n_indx;
    if (refresh_period >= 0) p.set_policy(n_indx, refresh_start, refresh_period, indx_out);
    p.set_rule(tol, min_iters, check, iters_out, ce3_out);
    return admm64_approx(ctx, "proposed_algorithm until (float64)", "jstsp_proposed_std_resume_f64", p);
}

int jstsp_proposed_std_resume_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                                  const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, const jstsp_c64 *PA_,
                                  const jstsp_c64 *PB_, int Imax, const double *tau_Y, const double *tau_S, const double *rho,
                                  const int32_t *indx_S_, jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, double *rcond_out,
                                  int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out, int memspace)
{
    ADMM64_RECORD(JSTSP_TYPE_STD, it0, state_in, state_out);
    return admm64_std(ctx, "proposed_algorithm 'std' resume (float64)", p, PA_, PB_, rcond_out);
}

}  // extern "C"
#undef ADMM64_RECORD
