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
#include "zgemm64.h"
#include "solver_common.h"

#include <algorithm>
#include <vector>

namespace jstsp {
namespace {

constexpr int P64_LDS_ORDER = 64;        // largest Gram order of the in-LDS Jacobi
constexpr int P64_MAX_ORDER = 512;       // largest Gram order at all
constexpr int P64_SWEEPS = 30;
constexpr size_t P64_WS_LIMIT = (size_t)24 << 30;

struct Par64 {          // per-trial scalars, all derived in float64 from the caller's doubles
    double rho, ir, cc, tY, tS;
};

__device__ __forceinline__ double2 zmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 zconj(double2 a) { return make_double2(a.x, -a.y); }

// fixed-order sum over the 256 threads of a workgroup
__device__ __forceinline__ double wg_sum(double v, double *sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- two-sided cyclic Jacobi in LDS ------------------------------------------------------------------------------------------
// round r of the circle ordering of n players (n even): slot s meets slot n - 1 - s, player 0 fixed, the others rotate by r
__device__ __forceinline__ void pair_of(int n, int r, int s, int &p, int &q)
{
    const int nm = n - 1;
    const int a = s == 0 ? 0 : 1 + (s - 1 + r) % nm, b = 1 + (n - 2 - s + r) % nm;
    p = min(a, b); q = max(a, b);
}

// G (n0 x n0 Hermitian, leading dimension n0) = U diag(lam) U^H.  VECS: U and all lam are written; otherwise lam[t] = lambda_max.
// LDS: H (n x n), [U (n x n)], n / 2 rotations (c, s), n even >= n0 (an odd order gets a decoupled zero row and column).
// A pair is rotated when |h_pq| > eps sqrt(|h_pp h_qq|) and |h_pq| > eps^2 dmax, dmax the largest diagonal entry of G (entries below
// the second level are rounding residue of a rank-deficient G: rotating them moves no eigenvalue by more than eps^2 dmax).
template <bool VECS>
__global__ __launch_bounds__(256) void jacobi64_lds_kernel(int n0, const double2 *G, long long sG, double2 *Uout, double *lam)
{
    extern __shared__ double2 sm[];
    const int n = (n0 + 1) & ~1, h2 = n / 2, t = blockIdx.x, tid = threadIdx.x;
    double2 *H = sm, *U = sm + (size_t)n * n, *rs = U + (VECS ? (size_t)n * n : 0);
    double *rc = reinterpret_cast<double *>(rs + h2), *red = rc + h2;
    const double EPS = 1.1102230246251565e-16;
    const double2 *g = G + (long long)t * sG;
    double dm = 0.0;
    for (int e = tid; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        double2 x = make_double2(0.0, 0.0);
        if (i < n0 && j < n0) x = g[i + (long long)n0 * j];
        if (i == j) { x.y = 0.0; dm = fmax(dm, fabs(x.x)); }
        H[e] = x;
        if (VECS) U[e] = make_double2(i == j ? 1.0 : 0.0, 0.0);
    }
    for (int o = 32; o > 0; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o));
    if ((tid & 63) == 0) red[tid >> 6] = dm;
    __syncthreads();
    const double floor_abs = EPS * EPS * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    for (int sweep = 0; sweep < P64_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < n - 1; ++r) {
            if (tid < h2) {
                int p, q;
                pair_of(n, r, tid, p, q);
                const double hpp = H[p + n * p].x, hqq = H[q + n * q].x;
                const double2 hpq = H[p + n * q];
                const double a = hypot(hpq.x, hpq.y);
                double c = 1.0;
                double2 sn = make_double2(0.0, 0.0);
                if (a > floor_abs && a > EPS * sqrt(fabs(hpp) * fabs(hqq))) {
                    // the real rotation of [hpp, a; a, hqq] after the phase e = hpq / |hpq| is pulled out
                    const double tau = (hqq - hpp) / (2.0 * a);
                    const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + tt * tt);
                    const double sr = tt * c;
                    sn = make_double2(sr * hpq.x / a, sr * hpq.y / a);
                    rotated = 1;
                }
                rc[tid] = c; rs[tid] = sn;
            }
            __syncthreads();
            // H <- J^H H J on the 2 x 2 block (row pair k, column pair l), J = [c, s; -conj(s), c] on the coordinates (p, q)
            for (int idx = tid; idx < h2 * h2; idx += 256) {
                const int l = idx % h2, k = idx / h2;
                const double cl = rc[l], ck = rc[k];
                const double2 sl = rs[l], sk = rs[k];
                if (sl.x == 0.0 && sl.y == 0.0 && sk.x == 0.0 && sk.y == 0.0) continue;        // neither pair rotates (s = 0: identity)
                int pl, ql, pk, qk;
                pair_of(n, r, l, pl, ql);
                pair_of(n, r, k, pk, qk);
                const double2 a00 = H[pk + n * pl], a01 = H[pk + n * ql], a10 = H[qk + n * pl], a11 = H[qk + n * ql];
                // columns: [x_p, x_q] J_l = [c x_p - conj(s) x_q, s x_p + c x_q]
                const double2 u0 = zmul(zconj(sl), a01), u1 = zmul(sl, a00), u2 = zmul(zconj(sl), a11), u3 = zmul(sl, a10);
                const double2 b00 = make_double2(cl * a00.x - u0.x, cl * a00.y - u0.y), b01 = make_double2(u1.x + cl * a01.x, u1.y + cl * a01.y);
                const double2 b10 = make_double2(cl * a10.x - u2.x, cl * a10.y - u2.y), b11 = make_double2(u3.x + cl * a11.x, u3.y + cl * a11.y);
                // rows: J_k^H [y_p; y_q] = [c y_p - s y_q; conj(s) y_p + c y_q]
                const double2 v0 = zmul(sk, b10), v1 = zmul(sk, b11), w0 = zmul(zconj(sk), b00), w1 = zmul(zconj(sk), b01);
                double2 c00 = make_double2(ck * b00.x - v0.x, ck * b00.y - v0.y), c01 = make_double2(ck * b01.x - v1.x, ck * b01.y - v1.y);
                double2 c10 = make_double2(w0.x + ck * b10.x, w0.y + ck * b10.y), c11 = make_double2(w1.x + ck * b11.x, w1.y + ck * b11.y);
                if (k == l) { c01 = make_double2(0.0, 0.0); c10 = c01; c00.y = 0.0; c11.y = 0.0; }       // the annihilated pair, exactly
                H[pk + n * pl] = c00; H[pk + n * ql] = c01; H[qk + n * pl] = c10; H[qk + n * ql] = c11;
            }
            if (VECS)
                for (int idx = tid; idx < n * h2; idx += 256) {          // U <- U J: row i, column pair l
                    const int i = idx % n, l = idx / n;
                    const double cl = rc[l];
                    const double2 sl = rs[l];
                    if (sl.x == 0.0 && sl.y == 0.0) continue;
                    int pl, ql;
                    pair_of(n, r, l, pl, ql);
                    const double2 xp = U[i + n * pl], xq = U[i + n * ql];
                    const double2 u0 = zmul(zconj(sl), xq), u1 = zmul(sl, xp);
                    U[i + n * pl] = make_double2(cl * xp.x - u0.x, cl * xp.y - u0.y);
                    U[i + n * ql] = make_double2(u1.x + cl * xq.x, u1.y + cl * xq.y);
                }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) break;
    }
    if (VECS) {
        for (int e = tid; e < n0 * n0; e += 256) Uout[(long long)t * n0 * n0 + e] = U[(e % n0) + n * (e / n0)];
        for (int i = tid; i < n0; i += 256) lam[(long long)t * n0 + i] = H[i + n * i].x;
    } else if (tid == 0) {
        double m = H[0].x;
        for (int i = 1; i < n0; ++i) m = fmax(m, H[i + n * i].x);
        lam[t] = m;
    }
}

size_t jacobi_lds_bytes(int n0, bool vecs)
{
    const size_t n = (size_t)((n0 + 1) & ~1);
    return (vecs ? 2 : 1) * n * n * sizeof(double2) + (n / 2) * (sizeof(double2) + sizeof(double)) + 4 * sizeof(double);
}

__global__ __launch_bounds__(256) void lam_max_kernel(int n, int nmat, const double *lam, double *out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nmat) return;
    double m = lam[(long long)t * n];
    for (int i = 1; i < n; ++i) m = fmax(m, lam[(long long)t * n + i]);
    out[t] = m;
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

// Uf(:, c) = max(0, 1 - tau / sigma_c) U(:, c), sigma_c = sqrt(lambda_c); a non-positive lambda_c gives 0
__global__ __launch_bounds__(256) void svt_scale64_kernel(int n, const double *thr, long long thr_stride5, const double *lam, const double2 *U, double2 *Uf)
{
    const int t = blockIdx.y;
    const double tau = thr[(long long)t * thr_stride5];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n * n; e += gridDim.x * 256) {
        const double l = lam[(long long)t * n + e / n];
        const double sg = l > 0.0 ? sqrt(l) : 0.0;
        const double f = sg > tau ? 1.0 - tau / sg : 0.0;
        const double2 u = U[(long long)t * n * n + e];
        Uf[(long long)t * n * n + e] = make_double2(f * u.x, f * u.y);
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

// rank[e] = position of entry e (0-based) in indx_S (1-based linear indices); an index outside 1 .. g is ignored
__global__ __launch_bounds__(256) void rank64_init_kernel(long long n, int32_t *rank)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) rank[e] = 0x7fffffff;
}
__global__ __launch_bounds__(256) void rank64_kernel(int g, const int32_t *indx, int32_t *rank)
{
    const long long o = (long long)blockIdx.y * g;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < g; p += gridDim.x * 256) {
        const int32_t e = indx[o + p] - 1;
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

// ce(i, 1) = lambda_max(V1) / lambda_max(X), ce(i, 2) = lambda_max(V2) / lambda_max(X); ce laid out Imax x 3 per trial
__global__ __launch_bounds__(256) void ce64_kernel(int batch, int Imax, int it, const double *lx, const double *l1, const double *l2, const double *ce3,
                                                   double *ce)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch) return;
    double *c = ce + (long long)t * 3 * Imax + it;
    c[0] = l1[t] / lx[t]; c[Imax] = l2[t] / lx[t]; c[2 * Imax] = ce3[t];
}

// ---- workspace: one stream-ordered slab, bump allocation ----------------------------------------------------------------------
struct Slab {
    hipStream_t st;
    char *base = nullptr;
    size_t cap = 0, off = 0;
    explicit Slab(hipStream_t s) : st(s) {}
    ~Slab() { if (base) (void)hipFreeAsync(base, st); }
    static size_t rnd(size_t b) { return (b + 255) & ~(size_t)255; }
    int reserve(size_t bytes, const char *nm)
    {
        const hipError_t e = hipMallocAsync((void **)&base, std::max<size_t>(bytes, 256), st);
        if (e != hipSuccess) { base = nullptr; set_error("%s: hipMallocAsync(%zu) failed: %s", nm, bytes, hipGetErrorString(e)); return JSTSP_E_NOMEM; }
        cap = bytes;
        return 0;
    }
    template <class T> T *get(size_t n)
    {
        const size_t b = rnd(n * sizeof(T));
        if (off + b > cap) return nullptr;          // (the sizes are counted by the same Sizer below: cannot happen)
        T *p = reinterpret_cast<T *>(base + off);
        off += b;
        return p;
    }
};

// svt of `batch` matrices Z (N x M) with thresholds thr[t * thr_stride]: the arrays it needs and the steps
struct Svt64 {
    int N, M, n, batch;
    bool left;              // n = N: G = Z Z^H, Y = Q Z; otherwise G = Z^H Z, Y = Z Q
    double2 *G, *U, *Uf, *Q, *ws;
    double *lam;
    static size_t bytes(int N, int M, int batch)
    {
        const size_t n = std::min(N, M), nn = n * n * batch;
        return 4 * Slab::rnd(nn * sizeof(double2)) + Slab::rnd(std::max<size_t>(1, ws_elems(N, M, batch)) * sizeof(double2)) +
               Slab::rnd(n * batch * sizeof(double));
    }
    static size_t ws_elems(int N, int M, int batch)
    {
        const int n = std::min(N, M), k = std::max(N, M);
        return std::max(std::max(zgemm64_ws_elems(n, n, k, batch), zgemm64_ws_elems(n, n, n, batch)), zgemm64_ws_elems(N, M, n, batch));
    }
    void init(Slab &s, int N_, int M_, int batch_)
    {
        N = N_; M = M_; batch = batch_; n = std::min(N, M); left = N <= M;
        const size_t nn = (size_t)n * n * batch;
        G = s.get<double2>(nn); U = s.get<double2>(nn); Uf = s.get<double2>(nn); Q = s.get<double2>(nn);
        ws = s.get<double2>(std::max<size_t>(1, ws_elems(N, M, batch)));
        lam = s.get<double>((size_t)n * batch);
    }
    int gram(hipStream_t st, const double2 *Z, double2 *Gout) const
    {
        const Mat64 z{Z, (long long)N * M, N};
        return left ? zgemm64(st, 'N', 'C', n, n, M, batch, z, z, Gout, (long long)n * n, n, ws)
                    : zgemm64(st, 'C', 'N', n, n, N, batch, z, z, Gout, (long long)n * n, n, ws);
    }
    // U, lam of G (n <= 64: in LDS, asynchronous; above: vamp64.hip's Jacobi, synchronises)
    int eig(hipStream_t st) const
    {
        if (n <= P64_LDS_ORDER) {
            const size_t sh = jacobi_lds_bytes(n, true);
            JSTSP_HIP(hipFuncSetAttribute((const void *)jacobi64_lds_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            hipLaunchKernelGGL(jacobi64_lds_kernel<true>, dim3(batch), dim3(256), sh, st, n, G, (long long)n * n, U, lam);
            JSTSP_HIP(hipGetLastError());
            return 0;
        }
        return eig64_global(st, n, batch, G, (long long)n * n, U, lam);
    }
    // lmax[t] = lambda_max of the Gram of Z[t]
    int lambda_max(hipStream_t st, const double2 *Z, double *lmax) const
    {
        JSTSP_TRY(gram(st, Z, G));
        if (n <= P64_LDS_ORDER) {
            const size_t sh = jacobi_lds_bytes(n, false);
            JSTSP_HIP(hipFuncSetAttribute((const void *)jacobi64_lds_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            hipLaunchKernelGGL(jacobi64_lds_kernel<false>, dim3(batch), dim3(256), sh, st, n, G, (long long)n * n, (double2 *)nullptr, lmax);
        } else {
            JSTSP_TRY(eig64_global(st, n, batch, G, (long long)n * n, U, lam));
            hipLaunchKernelGGL(lam_max_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, n, batch, lam, lmax);
        }
        JSTSP_HIP(hipGetLastError());
        return 0;
    }
    // Y = svt(Z, thr)
    int apply(hipStream_t st, const double2 *Z, const double *thr, long long thr_stride, double2 *Y) const
    {
        const long long snn = (long long)n * n, snm = (long long)N * M;
        JSTSP_TRY(gram(st, Z, G));
        JSTSP_TRY(eig(st));
        hipLaunchKernelGGL(svt_scale64_kernel, dim3((unsigned)std::min((n * n + 255) / 256, 64), batch), dim3(256), 0, st, n, thr, thr_stride, lam, U, Uf);
        JSTSP_HIP(hipGetLastError());
        JSTSP_TRY(zgemm64(st, 'N', 'C', n, n, n, batch, Mat64{Uf, snn, n}, Mat64{U, snn, n}, Q, snn, n, ws));
        return left ? zgemm64(st, 'N', 'N', N, M, N, batch, Mat64{Q, snn, n}, Mat64{Z, snm, N}, Y, snm, N, ws)
                    : zgemm64(st, 'N', 'N', N, M, M, batch, Mat64{Z, snm, N}, Mat64{Q, snn, n}, Y, snm, N, ws);
    }
};

// elements of the scratch array that the split products of one solve share (the largest need among its products)
size_t solver_ws_elems(int N, int M, int Gr, int G2, int batch, int nA, int nB)
{
    size_t e = std::max(zgemm64_ws_elems(Gr, Gr, N, nA), zgemm64_ws_elems(G2, G2, M, nB));
    const int shp[6][3] = {{Gr, M, N}, {Gr, G2, M}, {Gr, G2, Gr}, {Gr, G2, G2}, {N, G2, Gr}, {N, M, G2}};
    for (const auto &q : shp) e = std::max(e, zgemm64_ws_elems(q[0], q[1], q[2], batch));
    return std::max<size_t>(1, e);
}

// bytes of the solver's workspace for `batch` trials (the allocations of proposed64_run in the same order)
size_t proposed64_bytes(int N, int M, int Gr, int G2, int batch, bool host, long long strideA, long long strideB, bool angles, bool want_ce, int Imax)
{
    auto r = [](size_t n, size_t sz) { return Slab::rnd(n * sz); };
    const size_t nm = (size_t)N * M * batch, g = (size_t)Gr * G2 * batch, z2 = sizeof(double2);
    const int nA = strideA ? batch : 1, nB = strideB ? batch : 1;
    size_t b = r(batch, sizeof(Par64));
    if (host) {
        b += r(nm, z2) + r(nm, sizeof(double)) + r((strideA ? (size_t)strideA * (batch - 1) : 0) + (size_t)N * Gr, z2) +
             r((strideB ? (size_t)strideB * (batch - 1) : 0) + (size_t)G2 * M, z2);
        if (angles) b += r(g, sizeof(int32_t));
        b += r(g, z2) + r(nm, z2) + r((size_t)3 * Imax * batch, sizeof(double));
    }
    b += 8 * r(nm, z2);                                                     // X V1 V2 C Xs Y Z K
    b += 5 * r(g, z2);                                                      // V S Res RRes T2
    b += r((size_t)Gr * M * batch, z2) + r((size_t)N * G2 * batch, z2);     // T W
    b += r((size_t)Gr * Gr * nA, z2) + r((size_t)G2 * G2 * nB, z2);         // G_A G_B
    b += r(solver_ws_elems(N, M, Gr, G2, batch, nA, nB), z2);
    if (angles) b += r(g, sizeof(int32_t));
    b += 4 * r(batch, sizeof(double));
    (void)want_ce;
    return b + Svt64::bytes(N, M, batch);
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
    const size_t nm = (size_t)Mr * Mt * batch;
    const size_t need = Svt64::bytes(Mr, Mt, batch) + Slab::rnd(batch * sizeof(double)) + (memspace == JSTSP_HOST ? 2 * Slab::rnd(nm * sizeof(double2)) : 0);
    JSTSP_REQUIRE(need <= P64_WS_LIMIT, JSTSP_E_UNSUPPORTED, "svt (float64): the float64 workspace would be %.1f GiB (limit 24)",
                  (double)need / (double)((size_t)1 << 30));
    Slab s(st);
    JSTSP_TRY(s.reserve(need, "svt (float64)"));
    double *thr = s.get<double>(batch);
    JSTSP_HIP(hipMemcpyAsync(thr, tau, batch * sizeof(double), hipMemcpyHostToDevice, st));
    const double2 *Y = reinterpret_cast<const double2 *>(Y_);
    double2 *X = reinterpret_cast<double2 *>(X_);
    if (memspace == JSTSP_HOST) {
        double2 *y = s.get<double2>(nm);
        X = s.get<double2>(nm);
        JSTSP_HIP(hipMemcpyAsync(y, Y_, nm * sizeof(double2), hipMemcpyHostToDevice, st));
        Y = y;
    }
    Svt64 sv;
    sv.init(s, Mr, Mt, batch);
    JSTSP_TRY(sv.apply(st, Y, thr, 1, X));
    if (memspace == JSTSP_HOST) {
        JSTSP_HIP(hipMemcpyAsync(X_, X, nm * sizeof(double2), hipMemcpyDeviceToHost, st));
        JSTSP_HIP(hipStreamSynchronize(st));
    } else {
        JSTSP_HIP(hipStreamSynchronize(st));        // (tau was read from the caller's host array by the copy above)
    }
    return 0;
}

int jstsp_proposed_algorithm_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                                 const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, int Imax, const double *tau_Y,
                                 const double *tau_S, const double *rho, int type, const int32_t *indx_S_, jstsp_c64 *S_out, jstsp_c64 *Y_out,
                                 double *ce_out, int memspace)
{
    const char *nmf = "proposed_algorithm (float64)";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0 && Imax > 0 && strideA >= 0 && strideB >= 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE(subY_ && Omega_ && A_ && B_ && tau_Y && tau_S && rho && S_out, JSTSP_E_NULL, "%s: NULL argument", nmf);
    JSTSP_REQUIRE(type == JSTSP_TYPE_APPROXIMATE || type == JSTSP_TYPE_STD, JSTSP_E_ARG, "%s: bad type %d", nmf, type);
    JSTSP_REQUIRE(type == JSTSP_TYPE_APPROXIMATE, JSTSP_E_UNSUPPORTED,
                  "%s: 'std' has no float64 path (its least-squares solve is fp32 work): use jstsp_proposed_algorithm_c64", nmf);
    JSTSP_REQUIRE(std::min(N, M) <= P64_MAX_ORDER, JSTSP_E_UNSUPPORTED, "%s: min(N, M) = %d: the float64 eigen-decomposition is limited to order %d", nmf,
                  std::min(N, M), P64_MAX_ORDER);
    JSTSP_REQUIRE((long long)Gr * G2 < (1ll << 31) && (long long)N * M < (1ll << 31) && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: more than 2^31 entries per trial or more than 65535 trials", nmf);
    const bool host = memspace == JSTSP_HOST, angles = indx_S_ != nullptr, want_ce = ce_out != nullptr;
    const size_t need = proposed64_bytes(N, M, Gr, G2, batch, host, strideA, strideB, angles, want_ce, Imax);
    if (need > P64_WS_LIMIT) {
        int fit = batch;
        while (fit > 1 && proposed64_bytes(N, M, Gr, G2, fit, host, strideA ? strideA : 0, strideB ? strideB : 0, angles, want_ce, Imax) > P64_WS_LIMIT)
            fit = fit > 64 ? fit - fit / 16 : fit - 1;
        set_error("%s: the float64 workspace would be %.1f GiB (limit 24); the largest batch that fits is about %d", nmf,
                  (double)need / (double)((size_t)1 << 30), fit);
        return JSTSP_E_UNSUPPORTED;
    }
    hipStream_t st = ctx->stream;
    Slab s(st);
    JSTSP_TRY(s.reserve(need, nmf));
    const size_t nm1 = (size_t)N * M, g1 = (size_t)Gr * G2, nm = nm1 * batch, g = g1 * batch;
    const int nA = strideA ? batch : 1, nB = strideB ? batch : 1;

    std::vector<Par64> hp(batch);
    for (int t = 0; t < batch; ++t) hp[t] = Par64{rho[t], 1.0 / rho[t], rho[t] / (rho[t] + 1.0), tau_Y[t] / rho[t], tau_S[t] / rho[t]};
    Par64 *par = s.get<Par64>(batch);
    JSTSP_HIP(hipMemcpyAsync(par, hp.data(), batch * sizeof(Par64), hipMemcpyHostToDevice, st));
    JSTSP_HIP(hipStreamSynchronize(st));            // (hp is this call's own: copied before it goes out of scope on any path)

    const double2 *subY = reinterpret_cast<const double2 *>(subY_), *A = reinterpret_cast<const double2 *>(A_), *B = reinterpret_cast<const double2 *>(B_);
    const double *Omega = Omega_;
    const int32_t *indx = indx_S_;
    double2 *Sd = reinterpret_cast<double2 *>(S_out), *Yd = reinterpret_cast<double2 *>(Y_out);
    double *ced = ce_out;
    if (host) {
        const size_t szA = (strideA ? (size_t)strideA * (batch - 1) : 0) + (size_t)N * Gr, szB = (strideB ? (size_t)strideB * (batch - 1) : 0) + (size_t)G2 * M;
        double2 *y = s.get<double2>(nm);
        double *om = s.get<double>(nm);
        double2 *a = s.get<double2>(szA), *b = s.get<double2>(szB);
        JSTSP_HIP(hipMemcpyAsync(y, subY_, nm * sizeof(double2), hipMemcpyHostToDevice, st));
        JSTSP_HIP(hipMemcpyAsync(om, Omega_, nm * sizeof(double), hipMemcpyHostToDevice, st));
        JSTSP_HIP(hipMemcpyAsync(a, A_, szA * sizeof(double2), hipMemcpyHostToDevice, st));
        JSTSP_HIP(hipMemcpyAsync(b, B_, szB * sizeof(double2), hipMemcpyHostToDevice, st));
        subY = y; Omega = om; A = a; B = b;
        if (angles) {
            int32_t *ix = s.get<int32_t>(g);
            JSTSP_HIP(hipMemcpyAsync(ix, indx_S_, g * sizeof(int32_t), hipMemcpyHostToDevice, st));
            indx = ix;
        }
        Sd = s.get<double2>(g); Yd = s.get<double2>(nm); ced = s.get<double>((size_t)3 * Imax * batch);
    }
    double2 *X = s.get<double2>(nm), *V1 = s.get<double2>(nm), *V2 = s.get<double2>(nm), *Cm = s.get<double2>(nm), *Xs = s.get<double2>(nm),
            *Y = s.get<double2>(nm), *Z = s.get<double2>(nm), *K = s.get<double2>(nm);
    double2 *V = s.get<double2>(g), *S = s.get<double2>(g), *Res = s.get<double2>(g), *RRes = s.get<double2>(g), *T2 = s.get<double2>(g);
    double2 *T = s.get<double2>((size_t)Gr * M * batch), *W = s.get<double2>((size_t)N * G2 * batch);
    double2 *GA = s.get<double2>((size_t)Gr * Gr * nA), *GB = s.get<double2>((size_t)G2 * G2 * nB);
    double2 *gws = s.get<double2>(solver_ws_elems(N, M, Gr, G2, batch, nA, nB));
    int32_t *rank = angles ? s.get<int32_t>(g) : nullptr;
    double *lx = s.get<double>(batch), *l1 = s.get<double>(batch), *l2 = s.get<double>(batch), *ce3 = s.get<double>(batch);
    Svt64 sv;
    sv.init(s, N, M, batch);
    JSTSP_REQUIRE(sv.lam != nullptr && ce3 != nullptr, JSTSP_E_NOMEM, "%s: workspace accounting error", nmf);

    for (double2 *p : {X, V1, V2, Cm, Xs}) JSTSP_HIP(hipMemsetAsync(p, 0, nm * sizeof(double2), st));
    JSTSP_HIP(hipMemsetAsync(V, 0, g * sizeof(double2), st));
    if (angles) {
        hipLaunchKernelGGL(rank64_init_kernel, dim3((unsigned)std::min<size_t>((g + 255) / 256, 4096)), dim3(256), 0, st, (long long)g, rank);
        hipLaunchKernelGGL(rank64_kernel, egrid((long long)g1, batch), dim3(256), 0, st, (int)g1, indx, rank);
    }
    const long long sNM = (long long)nm1, sG = (long long)g1, sGA = strideA ? (long long)Gr * Gr : 0, sGB = strideB ? (long long)G2 * G2 : 0;
    const Mat64 Am{A, strideA, N}, Bm{B, strideB, G2}, GAm{GA, sGA, Gr}, GBm{GB, sGB, G2};
    JSTSP_TRY(zgemm64(st, 'C', 'N', Gr, Gr, N, nA, Am, Am, GA, (long long)Gr * Gr, Gr, gws));          // G_A = A^H A
    JSTSP_TRY(zgemm64(st, 'N', 'C', G2, G2, M, nB, Bm, Bm, GB, (long long)G2 * G2, G2, gws));          // G_B = B B^H
    const dim3 gnm = egrid((long long)nm1, batch);
    for (int it = 0; it < Imax; ++it) {
        const int cnt = (int)std::min<long long>(10 + 5ll * (it + 1), (long long)g1);                  // angles :36
        hipLaunchKernelGGL(form_z64_kernel, gnm, dim3(256), 0, st, (long long)nm1, par, X, V1, Z);
        JSTSP_TRY(sv.apply(st, Z, &par->tY, (long long)(sizeof(Par64) / sizeof(double)), Y));          // :35
        hipLaunchKernelGGL(update_x64_kernel, gnm, dim3(256), 0, st, (long long)nm1, par, V1, Y, subY, V2, Cm, Xs, Omega, X, K);
        JSTSP_TRY(zgemm64(st, 'C', 'N', Gr, M, N, batch, Am, Mat64{K, sNM, N}, T, (long long)Gr * M, Gr, gws));        // A^H K
        JSTSP_TRY(zgemm64(st, 'N', 'C', Gr, G2, M, batch, Mat64{T, (long long)Gr * M, Gr}, Bm, Res, sG, Gr, gws));     // ... B^H
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, Gr, batch, GAm, Mat64{V, sG, Gr}, T2, sG, Gr, gws));                   // G_A V
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, G2, batch, Mat64{T2, sG, Gr}, GBm, RRes, sG, Gr, gws));                // ... G_B
        hipLaunchKernelGGL(sub64_kernel, dim3((unsigned)std::min<size_t>((g + 255) / 256, 4096)), dim3(256), 0, st, (long long)g, Res, RRes);
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, Gr, batch, GAm, Mat64{Res, sG, Gr}, T2, sG, Gr, gws));                 // G_A Res
        JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, G2, batch, Mat64{T2, sG, Gr}, GBm, RRes, sG, Gr, gws));                // ... G_B
        hipLaunchKernelGGL(step_v64_kernel, dim3(batch), dim3(256), 0, st, (int)g1, par, Res, RRes, V, S, rank, cnt, want_ce ? ce3 : nullptr);
        JSTSP_TRY(zgemm64(st, 'N', 'N', N, G2, Gr, batch, Am, Mat64{S, sG, Gr}, W, (long long)N * G2, N, gws));        // A S
        JSTSP_TRY(zgemm64(st, 'N', 'N', N, M, G2, batch, Mat64{W, (long long)N * G2, N}, Bm, Xs, sNM, N, gws));        // ... B
        hipLaunchKernelGGL(update_c64_kernel, gnm, dim3(256), 0, st, (long long)nm1, par, X, Xs, Y, Cm, V1, V2);
        if (want_ce) {
            JSTSP_TRY(sv.lambda_max(st, X, lx));
            JSTSP_TRY(sv.lambda_max(st, V1, l1));
            JSTSP_TRY(sv.lambda_max(st, V2, l2));
            hipLaunchKernelGGL(ce64_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, Imax, it, lx, l1, l2, ce3, ced);
        }
        JSTSP_HIP(hipGetLastError());
    }
    JSTSP_HIP(hipMemcpyAsync(Sd, S, g * sizeof(double2), hipMemcpyDeviceToDevice, st));
    if (Y_out) JSTSP_HIP(hipMemcpyAsync(Yd, Y, nm * sizeof(double2), hipMemcpyDeviceToDevice, st));
    if (host) {
        JSTSP_HIP(hipMemcpyAsync(S_out, Sd, g * sizeof(double2), hipMemcpyDeviceToHost, st));
        if (Y_out) JSTSP_HIP(hipMemcpyAsync(Y_out, Yd, nm * sizeof(double2), hipMemcpyDeviceToHost, st));
        if (want_ce) JSTSP_HIP(hipMemcpyAsync(ce_out, ced, (size_t)3 * Imax * batch * sizeof(double), hipMemcpyDeviceToHost, st));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

}  // extern "C"
