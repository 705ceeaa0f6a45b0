// jstsp_omp_f64 / jstsp_omp_kron_f64 — benchmark_algorithms/OMP.m:1-32 in FLOAT64, batched over problems: the algorithm and the
// conventions of jstsp_omp_c32 / jstsp_omp_kron_c32 (omp.hip states them) with every stored value and every sum a double - residual,
// basis, triangular factor, correlations, scores, the back-substitution and x_hat.  Nothing is narrowed.
//     repeat m times:  idx = argmax |Phi' r| (first index on ties; chosen atoms are NOT excluded, OMP.m:18)
//                      targetMatrix = [targetMatrix, Phi(:, idx)];  x = pinv(targetMatrix) v;  r = v - targetMatrix x
// The least squares is carried in measurement space, the structure of mmv_omp64.hip with S = 1: an orthonormal basis Q of the
// selected atoms (two passes of classical Gram-Schmidt per new atom: cgs2_append of ws64.h, the code mmv_omp64.hip runs), the
// triangular factor, z = Q^H v, one back-substitution at the end.  An index that is already in the index set leaves span and residual alone and raises the atom's multiplicity: pinv
// splits the coefficient equally over the copies and the scatter of OMP.m:29-32 leaves the last copy in x_hat.  A NEW index whose
// atom lies in the span already (||a - Q Q' a||^2 <= 1e-20 ||a||^2 after the two passes, or a = 0) adds nothing either and keeps
// the coefficient 0, as in omp.hip.
// Launches per iteration for the whole batch; nothing is read back on the host inside the loop:
//   1. c = Phi' r.  Dense: one wave per atom, the four real fma chains (xx, yy, xy, yx) of mmv_omp64.hip joined at the end, grid
//      over atoms x problems.  Kronecker Phi = kron(Bf.', Af): Af^H R Bf^H by two zgemm64 products, Phi is never formed.
//   2. selection and update, one workgroup per problem: score x*x + y*y with contraction off (columns equal up to a factor -1 or
//      +-1i tie on the bits), strided scan per thread, xor tree per wave, the four waves in order - the first index among equal
//      scores, a NaN never wins; then gather, orthogonalise, append, downdate.
// Each problem is solved on v * 2^-e, e the exponent of its largest finite component, and x_hat is scaled back by 2^e: index sets
// do not depend on the scale of v and x_hat of v 2^k is x_hat 2^k on the bits.  No atomics, every sum in a fixed order by a fixed
// thread: a repeated call returns the same bits and a problem's result does not depend on its batch mates, on whether the
// dictionary is shared, or on the memspace.
#include "ws64.h"
#include "zgemm64.h"

#include <algorithm>
#include <cfloat>

namespace jstsp {
namespace {

constexpr int OMP64_MAX_M = 1024;                  // iterations (the basis coefficients of one atom live in LDS)
constexpr int OMP64_MAX_MEAS = 1 << 16;            // measurements per problem (dense: measures; Kronecker: N M)
constexpr int OMP64_MAX_ATOMS = 1 << 20;           // atoms (dense: size_d; Kronecker: Gr G2)

struct Omp64 {
    double2 *r;        // [batch][meas]        residual of the scaled problem
    double2 *Q;        // [batch][meas][m]     orthonormal basis of the distinct selected atoms
    double2 *Rm;       // [batch][m][m]        upper-triangular factor (column-major): atoms = Q Rm
    double2 *z;        // [batch][m]           Q^H v
    int *uniq;         // [batch][m]           0-based atom of basis vector j
    int *mult;         // [batch][m]           its multiplicity in the index set
    int *sel;          // [batch][m]           0-based atom selected in iteration it
    int *nu;           // [batch]              basis vectors so far
    int *ex;           // [batch]              e: the problem is solved on v 2^-e
};

// r = v 2^-e, e the exponent of the largest finite component (exact unless a component underflows); nu = 0
__global__ __launch_bounds__(256) void omp64_init_kernel(int meas, const double2 *V, Omp64 s)
{
    __shared__ double red[4];
    const int t = blockIdx.x, tid = threadIdx.x;
    const double2 *v = V + (long long)t * meas;
    double2 *r = s.r + (long long)t * meas;
    const int ev = finite_max_exponent(v, meas, red);
    for (int e = tid; e < meas; e += 256) r[e] = make_double2(ldexp(v[e].x, -ev), ldexp(v[e].y, -ev));
    if (tid == 0) { s.nu[t] = 0; s.ex[t] = ev; }
}

// dense dictionary: c[t][j] = A(:, j)^H r, one wave per atom j (lane l sums the measurements l, l + 64, ... in four chains)
__global__ __launch_bounds__(256) void omp64_corr_kernel(int meas, int size_d, const double2 *A, long long strideA, const double2 *R,
                                                         double2 *corr)
{
    const int t = blockIdx.y, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= size_d) return;                                      // (whole waves; no barrier below)
    const double2 *a = A + (long long)t * strideA + (long long)meas * j, *r = R + (long long)t * meas;
    Dot4 d = {0.0, 0.0, 0.0, 0.0};
    for (int e = lane; e < meas; e += 64) dot4_step(d, a[e], r[e]);
    const double cx = wave_sum64(d.xx + d.yy), cy = wave_sum64(d.xy - d.yx);
    if (lane == 0) corr[(long long)t * size_d + j] = make_double2(cx, cy);
}

// MATLAB max: the larger value, the smaller index among equal ones
__device__ __forceinline__ void omp64_best(double &b, int &bi, double ob, int oi)
{
    if (ob > b || (ob == b && oi < bi)) { b = ob; bi = oi; }
}

// One workgroup per problem: idx = argmax |c|^2 (OMP.m:17), then the atom is appended (:18-21).
// Dense dictionary (Bf == nullptr): atom = A(:, idx).  Kronecker: atom(i + N k) = Af(i, g) Bf(h, k), idx = g + Gr h.
__global__ __launch_bounds__(256) void omp64_step_kernel(int meas, int size_d, int m, int it, const double2 *corr, const double2 *A,
                                                         long long strideA, const double2 *Bf, long long strideB, int N, int Gr, int G2,
                                                         Omp64 s)
{
    __shared__ double sh[4];
    __shared__ double sbv[4];
    __shared__ int sbi[4];
    __shared__ int s_idx, s_dup;
    __shared__ double2 D[OMP64_MAX_M];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- selection: strided scan (strict >: the smallest index per thread), xor tree per wave, the four waves in order
    const double2 *c = corr + (long long)t * size_d;
    double best = -1.0;
    int bi = 0x7fffffff;
    for (int i = tid; i < size_d; i += 256) {
        const double a = abs2_sym(c[i].x, c[i].y);
        if (a > best) { best = a; bi = i; }                       // (a NaN compares false: it never wins)
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bi, o);
        omp64_best(best, bi, ob, oi);
    }
    if (lane == 0) { sbv[wave] = best; sbi[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        best = sbv[0]; bi = sbi[0];
        for (int k = 1; k < 4; ++k) omp64_best(best, bi, sbv[k], sbi[k]);
        if (bi == 0x7fffffff) bi = 0;                             // every score a NaN: any index
        s_idx = bi;
        s.sel[(long long)t * m + it] = bi;
        int dup = -1;
        const int nu = s.nu[t];
        for (int j = 0; j < nu; ++j)
            if (s.uniq[(long long)t * m + j] == bi) { dup = j; break; }
        s_dup = dup;
        if (dup >= 0) s.mult[(long long)t * m + dup] += 1;
    }
    __syncthreads();
    if (s_dup >= 0) return;                                       // re-selected atom: span and residual unchanged
    const int idx = s_idx, u = s.nu[t];
    double2 *Q = s.Q + (long long)t * meas * m, *q = Q + (long long)meas * u;
    double2 *Rc = s.Rm + (long long)t * m * m + (long long)u * m; // column u of the triangular factor
    double2 *r = s.r + (long long)t * meas;
    // ---- gather the atom
    double n0 = 0.0;
    if (Bf) {
        const double2 *a = A + (long long)t * strideA + (long long)N * (idx % Gr);   // Af(:, g)
        const double2 *b = Bf + (long long)t * strideB + idx / Gr;                   // Bf(h, :), stride G2
        for (int e = tid; e < meas; e += 256) {
            const double2 v = zmul(a[e % N], b[(long long)G2 * (e / N)]);
            q[e] = v;
            n0 = fma(v.x, v.x, n0);
            n0 = fma(v.y, v.y, n0);
        }
    } else {
        const double2 *a = A + (long long)t * strideA + (long long)meas * idx;
        for (int e = tid; e < meas; e += 256) {
            const double2 v = a[e];
            q[e] = v;
            n0 = fma(v.x, v.x, n0);
            n0 = fma(v.y, v.y, n0);
        }
    }
    for (int j = tid; j < m; j += 256) Rc[j] = make_double2(0.0, 0.0);
    n0 = block_sum64(n0, sh);                                      // (its barriers publish q and Rc)
    const double n1 = cgs2_append(q, Q, meas, u, Rc, D, sh);       // two passes of classical Gram-Schmidt, then ||q||^2
    if (!(n1 > 1e-20 * n0) || !(n0 > 0.0)) return;                // inside the span of the chosen atoms (or NaN): adds nothing
    const double nrm = sqrt(n1), inv = 1.0 / nrm;
    // ---- q_u = w / |w|;  z_u = q_u^H r (r is orthogonal to the old basis);  r -= z_u q_u
    Dot4 d = {0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < meas; e += 256) {
        double2 v = q[e];
        v.x *= inv; v.y *= inv;
        q[e] = v;
        dot4_step(d, v, r[e]);
    }
    double2 zu;
    zu.x = block_sum64(d.xx + d.yy, sh);
    zu.y = block_sum64(d.xy - d.yx, sh);
    for (int e = tid; e < meas; e += 256) {
        const double2 w = q[e];
        double2 v = r[e];
        v.x -= zu.x * w.x - zu.y * w.y;
        v.y -= zu.x * w.y + zu.y * w.x;
        r[e] = v;
    }
    if (tid == 0) {
        Rc[u] = make_double2(nrm, 0.0);
        s.z[(long long)t * m + u] = zu;
        s.uniq[(long long)t * m + u] = idx;
        s.mult[(long long)t * m + u] = 1;
        s.nu[t] = u + 1;
    }
}

// x_unique = Rm^-1 z (column-oriented back-substitution: x_i is final once the columns i + 1 .. u - 1 have been subtracted, in
// that order), x_hat(atom) = x_unique / multiplicity * 2^e, indexSet (1-based), targetMatrix = the selected columns (OMP.m:18, 27-32)
__global__ __launch_bounds__(256) void omp64_finish_kernel(int meas, int size_d, int m, const double2 *A, long long strideA, Omp64 s,
                                                           double2 *x_hat, int32_t *index_out, double2 *target_out)
{
    extern __shared__ double2 xs[];                                // [m]
    const int t = blockIdx.x, tid = threadIdx.x;
    const int u = s.nu[t], ev = s.ex[t];
    const double2 *R = s.Rm + (long long)t * m * m;
    for (int i = tid; i < u; i += 256) xs[i] = s.z[(long long)t * m + i];
    for (int i = tid; i < size_d; i += 256) x_hat[(long long)t * size_d + i] = make_double2(0.0, 0.0);
    __syncthreads();
    for (int i = u - 1; i >= 0; --i) {
        if (tid == 0) {
            const double rii = R[i + (long long)m * i].x;
            xs[i] = make_double2(xs[i].x / rii, xs[i].y / rii);
        }
        __syncthreads();
        const double2 xi = xs[i];
        for (int j = tid; j < i; j += 256) {
            const double2 rji = R[j + (long long)m * i];
            xs[j] = make_double2(xs[j].x - (rji.x * xi.x - rji.y * xi.y), xs[j].y - (rji.x * xi.y + rji.y * xi.x));
        }
        __syncthreads();
    }
    for (int j = tid; j < u; j += 256) {                           // (distinct atoms: no two threads write one entry)
        const double mu = (double)s.mult[(long long)t * m + j];
        x_hat[(long long)t * size_d + s.uniq[(long long)t * m + j]] = make_double2(ldexp(xs[j].x / mu, ev), ldexp(xs[j].y / mu, ev));
    }
    for (int it = tid; it < m; it += 256) index_out[(long long)t * m + it] = s.sel[(long long)t * m + it] + 1;
    if (target_out)
        for (int it = 0; it < m; ++it) {
            const double2 *a = A + (long long)t * strideA + (long long)meas * s.sel[(long long)t * m + it];
            double2 *o = target_out + ((long long)t * m + it) * meas;
            for (int e = tid; e < meas; e += 256) o[e] = a[e];
        }
}

struct Omp64Shape {
    bool kron;
    int N, M, Gr, G2;              // Kronecker factors (dense: N = meas, M = 1, Gr = size_d, G2 = 1)
    int meas, size_d, m;
    long long strideA, strideB;
    bool host, want_target;
};

size_t omp64_zws(const Omp64Shape &p, int batch)
{
    return p.kron ? std::max<size_t>(1, std::max(zgemm64_ws_elems(p.Gr, p.M, p.N, batch), zgemm64_ws_elems(p.Gr, p.G2, p.M, batch))) : 0;
}

int omp64_run(jstsp_ctx *ctx, const char *nmf, const Omp64Shape &p, int batch, const jstsp_c64 *A_, const jstsp_c64 *B_, const jstsp_c64 *v_,
              jstsp_c64 *x_hat, int32_t *index_out, jstsp_c64 *target_out)
{
    hipStream_t st = ctx->stream;
    const size_t b = (size_t)batch, z2 = sizeof(double2), m = (size_t)p.m, meas = (size_t)p.meas, sd = (size_t)p.size_d;
    const double2 *A, *B = nullptr, *v;
    double2 *xh, *to = nullptr, *corr, *T = nullptr, *zws = nullptr;
    int32_t *io;
    Omp64 s;
    Slab sl(st);
    JSTSP_TRY(ws64_open(sl, nmf, batch, [&](Slab &w, int nb) {
        const size_t n = (size_t)nb;
        A = w.in(reinterpret_cast<const double2 *>(A_), dict_elems(p.strideA, (size_t)p.N * p.Gr, nb), p.host);
        v = w.in(reinterpret_cast<const double2 *>(v_), n * meas, p.host);
        if (p.kron) B = w.in(reinterpret_cast<const double2 *>(B_), dict_elems(p.strideB, (size_t)p.G2 * p.M, nb), p.host);
        xh = w.out(reinterpret_cast<double2 *>(x_hat), n * sd, p.host);
        io = w.out(index_out, n * m, p.host);
        if (p.want_target) to = w.out(reinterpret_cast<double2 *>(target_out), n * meas * m, p.host);
        s.r = w.get<double2>(n * meas); s.Q = w.get<double2>(n * meas * m); s.Rm = w.get<double2>(n * m * m); s.z = w.get<double2>(n * m);
        corr = w.get<double2>(n * sd);
        s.uniq = w.get<int>(n * m); s.mult = w.get<int>(n * m); s.sel = w.get<int>(n * m);
        s.nu = w.get<int>(n); s.ex = w.get<int>(n);
        if (p.kron) { T = w.get<double2>(n * p.Gr * p.M); zws = w.get<double2>(omp64_zws(p, nb)); }
    }));
    hipLaunchKernelGGL(omp64_init_kernel, dim3(batch), dim3(256), 0, st, p.meas, v, s);
    for (int it = 0; it < p.m; ++it) {                                                                 // OMP.m:16
        if (p.kron) {
            // Phi' r = vec(Af^H R Bf^H), R = reshape(r, N, M): what jstsp_correlate_f64 computes
            JSTSP_TRY(zgemm64(st, 'C', 'N', p.Gr, p.M, p.N, batch, Mat64{A, p.strideA, p.N}, Mat64{s.r, (long long)meas, p.N}, T,
                              (long long)p.Gr * p.M, p.Gr, zws));
            JSTSP_TRY(zgemm64(st, 'N', 'C', p.Gr, p.G2, p.M, batch, Mat64{T, (long long)p.Gr * p.M, p.Gr}, Mat64{B, p.strideB, p.G2}, corr,
                              (long long)sd, p.Gr, zws));
        } else
            hipLaunchKernelGGL(omp64_corr_kernel, dim3((p.size_d + 3) / 4, batch), dim3(256), 0, st, p.meas, p.size_d, A, p.strideA, s.r, corr);
        hipLaunchKernelGGL(omp64_step_kernel, dim3(batch), dim3(256), 0, st, p.meas, p.size_d, p.m, it, corr, A, p.strideA, B, p.strideB, p.N,
                           p.Gr, p.G2, s);
    }
    hipLaunchKernelGGL(omp64_finish_kernel, dim3(batch), dim3(256), m * z2, st, p.meas, p.size_d, p.m, A, p.strideA, s, xh, io, to);
    JSTSP_HIP(hipGetLastError());
    if (p.host) {
        JSTSP_TRY(sl.copy_back(reinterpret_cast<double2 *>(x_hat), xh, b * sd));
        JSTSP_TRY(sl.copy_back(index_out, io, b * m));
        if (p.want_target) JSTSP_TRY(sl.copy_back(reinterpret_cast<double2 *>(target_out), to, b * meas * m));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

}  // namespace
}  // namespace jstsp

using namespace jstsp;

extern "C" {

int jstsp_omp_f64(jstsp_ctx *ctx, int meas, int size_d, int batch, const jstsp_c64 *A, long long strideA, const jstsp_c64 *v, int m,
                  jstsp_c64 *x_hat, int32_t *index_out, jstsp_c64 *target_out, int memspace)
{
    const char *nmf = "OMP (float64)";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(A && v && x_hat && index_out, JSTSP_E_NULL, "%s: NULL array argument", nmf);
    JSTSP_REQUIRE(meas > 0 && size_d > 0 && batch > 0 && m > 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE(m <= OMP64_MAX_M, JSTSP_E_UNSUPPORTED, "%s: m = %d > %d", nmf, m, OMP64_MAX_M);
    JSTSP_REQUIRE(meas <= OMP64_MAX_MEAS && size_d <= OMP64_MAX_ATOMS && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: measures = %d, size_d = %d, batch = %d (limits %d, %d, 65535)", nmf, meas, size_d, batch, OMP64_MAX_MEAS, OMP64_MAX_ATOMS);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_REQUIRE(strideA == 0 || strideA >= (long long)meas * size_d, JSTSP_E_SHAPE, "strideA too small");
    JSTSP_ENTER(ctx);
    const Omp64Shape p{false, meas, 1, size_d, 1, meas, size_d, m, strideA, 0, memspace == JSTSP_HOST, target_out != nullptr};
    return omp64_run(ctx, nmf, p, batch, A, nullptr, v, x_hat, index_out, target_out);
}

int jstsp_omp_kron_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *Af, long long strideA, const jstsp_c64 *Bf,
                       long long strideB, const jstsp_c64 *y, int m, jstsp_c64 *x_hat, int32_t *index_out, int memspace)
{
    const char *nmf = "omp_kron (float64)";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(Af && Bf && y && x_hat && index_out, JSTSP_E_NULL, "%s: NULL array argument", nmf);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0 && m > 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE(m <= OMP64_MAX_M, JSTSP_E_UNSUPPORTED, "%s: m = %d > %d", nmf, m, OMP64_MAX_M);
    JSTSP_REQUIRE((long long)N * M <= OMP64_MAX_MEAS && (long long)Gr * G2 <= OMP64_MAX_ATOMS && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: N M = %lld, Gr G2 = %lld, batch = %d (limits %d, %d, 65535)", nmf, (long long)N * M, (long long)Gr * G2, batch,
                  OMP64_MAX_MEAS, OMP64_MAX_ATOMS);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_REQUIRE((strideA == 0 || strideA >= (long long)N * Gr) && (strideB == 0 || strideB >= (long long)G2 * M), JSTSP_E_SHAPE,
                  "%s: a dictionary stride is smaller than its factor", nmf);
    JSTSP_ENTER(ctx);
    const Omp64Shape p{true, N, M, Gr, G2, N * M, Gr * G2, m, strideA, strideB, memspace == JSTSP_HOST, false};
    return omp64_run(ctx, nmf, p, batch, Af, Bf, y, x_hat, index_out, nullptr);
}

}  // extern "C"
