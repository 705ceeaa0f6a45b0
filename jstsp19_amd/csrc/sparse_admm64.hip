// jstsp_sparse_admm_f64 — benchmark_algorithms/sparse_admm.m:1-36 evaluated in FLOAT64 on the device, in the structured form of
// sparse_admm.hip and oracle/solvers.py sparse_admm: every stored value, product, eigenvalue and scalar is a double.
// The reference builds A = kron(conj(Dt), Dr) (:15), B = A'A - rho I (:16) and solves B \ rhs in every iteration (:26).  With
//     Gr_ = Dr^H Dr = Ur diag(lr) Ur^H,    Gt_ = Dt^T conj(Dt) = conj(Dt^H Dt) = conj(Uc) diag(lt) conj(Uc)^H   (Dt^H Dt = Uc diag(lt) Uc^H)
// A'A = Gt_ (x) Gr_ and the solve is diagonal in the factors' eigenbases:
//     R = Ur [ (Ur^H RHS Uc) ./ (lr lt^T - rho) ] Uc^H                      (Ut = conj(Uc): conj(Ut) = Uc, Ut^T = Uc^H)
// so every product is an 'N' or a 'C' product of zgemm64.  A'*vec(OH) = vec(Dr^H OH Dt), once.  rho = 0.01, tau_s = 1e-4 (:12-13).
// The two eigen-decompositions run once per call: the in-LDS Jacobi of svt64.h up to order 64, eig64_global above (one matrix each,
// freeze = true); their eigenvalues are read on the host once, where a non-finite one (a NaN or Inf in Dr / Dt, which the Jacobi
// reports as converged) ends the call with JSTSP_E_ILLCOND.  A denominator lr lt - rho that is exactly 0 gives what IEEE gives,
// the reference's singular B \ .  Per iteration: one element-wise kernel (V = R + Z/rho, S = soft(V, tau_s/rho), RHS = Z - rho S +
// A'OH), four products around the element-wise divide, one kernel Z += rho (R - S); convergence_error from Svt64::lambda_max.
// Every reduction lives in the products and the Jacobi, which sum in a fixed order inside one trial: a repeated call returns the
// same bits and a trial's result does not depend on the batch around it or on the memspace.
#include "svt64.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace jstsp {
namespace {

constexpr int SADMM64_MAX_ORDER = 512;

inline dim3 sa_grid(long long n) { return dim3((unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8192))); }

__device__ __forceinline__ double sa_soft1(double v, double thr)
{
    const double m = fmax(fabs(v) - thr, 0.0);
    return (v > 0.0) ? m : ((v < 0.0) ? -m : v * 0.0);            // max(|v| - t, 0) sign(v); a NaN stays a NaN
}

// :21-23, :26   V = R + Z/rho;  S = soft(V, thr) (separable in real and imaginary part);  RHS = Z - rho S + A'OH
__global__ __launch_bounds__(256) void sadmm64_soft_rhs_kernel(long long n, const double2 *R, const double2 *Z, const double2 *AhOH, double2 *S,
                                                               double2 *RHS, double rho, double thr)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double2 r = R[e], z = Z[e], a = AhOH[e];
        const double2 s = make_double2(sa_soft1(r.x + z.x / rho, thr), sa_soft1(r.y + z.y / rho, thr));
        S[e] = s;
        RHS[e] = make_double2((z.x - rho * s.x) + a.x, (z.y - rho * s.y) + a.y);
    }
}

// T(i, j) /= lr(i) lt(j) - rho, Mr x Mt per trial
__global__ __launch_bounds__(256) void sadmm64_divide_kernel(long long n, int Mr, int Mt, const double *lr, const double *lt, double rho, double2 *T)
{
    const long long nm = (long long)Mr * Mt;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long k = e % nm;
        const double den = lr[k % Mr] * lt[k / Mr] - rho;
        const double2 t = T[e];
        T[e] = make_double2(t.x / den, t.y / den);
    }
}

// :30   Z = Z + rho (R - S)
__global__ __launch_bounds__(256) void sadmm64_dual_kernel(long long n, const double2 *R, const double2 *S, double2 *Z, double rho)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double2 r = R[e], s = S[e];
        double2 z = Z[e];
        z.x += rho * (r.x - s.x);
        z.y += rho * (r.y - s.y);
        Z[e] = z;
    }
}

size_t sadmm64_zws(int Mr, int Mt, int batch)
{
    return std::max<size_t>(1, std::max(std::max(zgemm64_ws_elems(Mr, Mr, Mr, 1), zgemm64_ws_elems(Mt, Mt, Mt, 1)),
                                        std::max(zgemm64_ws_elems(Mr, Mt, Mr, batch), zgemm64_ws_elems(Mr, Mt, Mt, batch))));
}

}  // namespace
}  // namespace jstsp

using namespace jstsp;

extern "C" int jstsp_sparse_admm_f64(jstsp_ctx *ctx, int Mr, int Mt, int Gr, int Gt, int batch, const jstsp_c64 *Htrue_, const jstsp_c64 *OH_,
                                     const jstsp_c64 *Dr_, const jstsp_c64 *Dt_, int Imax, jstsp_c64 *S_out, double *ce_out, int memspace)
{
    const char *nmf = "sparse_admm (float64)";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(OH_ && Dr_ && Dt_ && S_out, JSTSP_E_NULL, "%s: NULL array argument", nmf);
    JSTSP_REQUIRE(!ce_out || Htrue_, JSTSP_E_NULL, "%s: convergence_error needs Htrue", nmf);
    JSTSP_REQUIRE(Mr > 0 && Mt > 0 && batch > 0 && Imax >= 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE(Gr == Mr && Gt == Mt, JSTSP_E_SHAPE,
                  "%s: the reference adds R (Gr x Gt) to Z (Mr x Mt) (sparse_admm.m:21) and forms A'A - rho*eye(Mr*Mt) (:16): Gr must "
                  "equal Mr and Gt must equal Mt (got %dx%d vs %dx%d)", nmf, Gr, Gt, Mr, Mt);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_REQUIRE(std::max(Mr, Mt) <= SADMM64_MAX_ORDER && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: max(Mr, Mt) = %d, batch = %d: the float64 eigen-decomposition of the factor Grams is limited to order %d (batch 65535)", nmf,
                  std::max(Mr, Mt), batch, SADMM64_MAX_ORDER);
    JSTSP_ENTER(ctx);
    const bool host = memspace == JSTSP_HOST, want_ce = ce_out != nullptr;
    hipStream_t st = ctx->stream;
    const size_t z2 = sizeof(double2), nm1 = (size_t)Mr * Mt, nm = nm1 * batch;
    const double rho = 0.01, tau_s = 0.0001, thr = tau_s / rho;                                          // :12-13
    const double2 *OH, *Dr, *Dt, *Htrue = nullptr;
    double2 *Sdev, *R, *Z, *RHS, *P, *T, *AhOH, *Gg, *Ur, *Gc, *Uc, *zws, *Dd = nullptr;
    double *ce = nullptr, *lr, *lt, *num = nullptr, *den = nullptr;
    Svt64 sv;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nmf, batch, [&](Slab &w, int b) {
        const size_t e = nm1 * b, rr = (size_t)Mr * Mr, tt = (size_t)Mt * Mt;
        OH = w.in(reinterpret_cast<const double2 *>(OH_), e, host);
        Dr = w.in(reinterpret_cast<const double2 *>(Dr_), rr, host);
        Dt = w.in(reinterpret_cast<const double2 *>(Dt_), tt, host);
        Sdev = w.out(reinterpret_cast<double2 *>(S_out), e, host);
        for (double2 **p : {&R, &Z, &RHS, &P, &T, &AhOH}) *p = w.get<double2>(e);
        Gg = w.get<double2>(rr); Ur = w.get<double2>(rr); Gc = w.get<double2>(tt); Uc = w.get<double2>(tt);
        lr = w.get<double>(Mr); lt = w.get<double>(Mt);
        zws = w.get<double2>(sadmm64_zws(Mr, Mt, b));
        if (want_ce) {
            Htrue = w.in(reinterpret_cast<const double2 *>(Htrue_), e, host);
            ce = w.out(ce_out, (size_t)b * std::max(Imax, 1), host);
            Dd = w.get<double2>(e); num = w.get<double>(b); den = w.get<double>(b);
            sv.layout(w, Mr, Mt, b);
        }
    }));
    sv.freeze = true;                       // a trial's bits do not depend on the batch around it, also for 64 < min(Mr, Mt)
    const long long snm = (long long)nm1, tot = (long long)nm;
    const Mat64 Drm{Dr, 0, Mr}, Dtm{Dt, 0, Mt}, Urm{Ur, 0, Mr}, Ucm{Uc, 0, Mt};

    // ---- setup: the factor Grams and their eigen-decompositions, shared by the batch
    JSTSP_TRY(zgemm64(st, 'C', 'N', Mr, Mr, Mr, 1, Drm, Drm, Gg, 0, Mr, zws));                           // Dr^H Dr
    JSTSP_TRY(zgemm64(st, 'C', 'N', Mt, Mt, Mt, 1, Dtm, Dtm, Gc, 0, Mt, zws));                           // Dt^H Dt = conj(Gt_)
    JSTSP_TRY(eig64(st, Mr, 1, Gg, Ur, lr, true));
    JSTSP_TRY(eig64(st, Mt, 1, Gc, Uc, lt, true));
    {
        std::vector<double> hl((size_t)Mr + Mt);
        JSTSP_HIP(hipMemcpyAsync(hl.data(), lr, Mr * sizeof(double), hipMemcpyDeviceToHost, st));
        JSTSP_HIP(hipMemcpyAsync(hl.data() + Mr, lt, Mt * sizeof(double), hipMemcpyDeviceToHost, st));
        JSTSP_HIP(hipStreamSynchronize(st));
        for (size_t i = 0; i < hl.size(); ++i)
            JSTSP_REQUIRE(std::isfinite(hl[i]), JSTSP_E_ILLCOND, "%s: eigenvalue %zu of the Gram of %s is not finite (a NaN or Inf in the dictionary)",
                          nmf, i < (size_t)Mr ? i : i - Mr, i < (size_t)Mr ? "Dr" : "Dt");
    }
    // A'*vec(OH) = vec(Dr^H OH Dt)
    JSTSP_TRY(zgemm64(st, 'C', 'N', Mr, Mt, Mr, batch, Drm, Mat64{OH, snm, Mr}, P, snm, Mr, zws));
    JSTSP_TRY(zgemm64(st, 'N', 'N', Mr, Mt, Mt, batch, Mat64{P, snm, Mr}, Dtm, AhOH, snm, Mr, zws));
    for (double2 *p : {R, Z, Sdev}) JSTSP_HIP(hipMemsetAsync(p, 0, nm * z2, st));                        // :8-9
    if (want_ce) JSTSP_TRY(sv.lambda_max(st, Htrue, den));

    for (int it = 0; it < Imax; ++it) {                                                                  // :18
        hipLaunchKernelGGL(sadmm64_soft_rhs_kernel, sa_grid(tot), dim3(256), 0, st, tot, R, Z, AhOH, Sdev, RHS, rho, thr);     // :21-23
        if (want_ce) {                                                                                   // :32
            JSTSP_TRY(zgemm64(st, 'N', 'N', Mr, Mt, Mr, batch, Drm, Mat64{Sdev, snm, Mr}, P, snm, Mr, zws));
            JSTSP_TRY(zgemm64(st, 'N', 'C', Mr, Mt, Mt, batch, Mat64{P, snm, Mr}, Dtm, T, snm, Mr, zws));
            hipLaunchKernelGGL(diff64_kernel, sa_grid(tot), dim3(256), 0, st, tot, T, Htrue, Dd);
            JSTSP_TRY(sv.lambda_max(st, Dd, num));
            hipLaunchKernelGGL(ratio64_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, Imax, it, num, den, ce);
        }
        // (the last iteration's R and Z feed nothing that is returned: S and convergence_error are complete before them)
        if (it + 1 < Imax) {
            // :26  R = Ur [ (Ur^H RHS Uc) ./ (lr lt^T - rho) ] Uc^H
            JSTSP_TRY(zgemm64(st, 'C', 'N', Mr, Mt, Mr, batch, Urm, Mat64{RHS, snm, Mr}, P, snm, Mr, zws));
            JSTSP_TRY(zgemm64(st, 'N', 'N', Mr, Mt, Mt, batch, Mat64{P, snm, Mr}, Ucm, T, snm, Mr, zws));
            hipLaunchKernelGGL(sadmm64_divide_kernel, sa_grid(tot), dim3(256), 0, st, tot, Mr, Mt, lr, lt, rho, T);
            JSTSP_TRY(zgemm64(st, 'N', 'N', Mr, Mt, Mr, batch, Urm, Mat64{T, snm, Mr}, P, snm, Mr, zws));
            JSTSP_TRY(zgemm64(st, 'N', 'C', Mr, Mt, Mt, batch, Mat64{P, snm, Mr}, Ucm, R, snm, Mr, zws));
            hipLaunchKernelGGL(sadmm64_dual_kernel, sa_grid(tot), dim3(256), 0, st, tot, R, Sdev, Z, rho);                     // :30
        }
        JSTSP_HIP(hipGetLastError());
    }
    if (host) {
        JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(S_out), Sdev, nm));
        if (want_ce && Imax > 0) JSTSP_TRY(s.copy_back(ce_out, ce, (size_t)batch * Imax));
    }
    JSTSP_HIP(hipStreamSynchronize(st));
    return 0;
}
