// jstsp_mc_svt_f64 / jstsp_mc_admm_f64 - benchmark_algorithms/mc_svt.m:1-12 and mc_admm.m:1-34 evaluated in FLOAT64 on the device:
// the first stage of the drivers' TSSR recipe (plot_errorVSsnr.m:151-162) and its ADMM sibling, to the digits MATLAB carries.
//   mc_svt   Y = 0;  repeat Imax times:  X = svt(Y, tau/rho);  Y = Y + rho (OH - Omega .* X)                          (:5-9)
//   mc_admm  X = Y = Z = 0;  repeat:  X = svt(Y - Z/rho, tau/rho);  Y = (OH + Z + rho X) ./ (Omega + rho);            (:22-25)
//                                     Z = Z + rho (X - Y);  ce(i) = sigma_max(X - Htrue)^2 / sigma_max(Htrue)^2       (:26-28)
// (the reference's dense solve A \ b has A = diag(vec(Omega)) + rho I: an entrywise division).  The svt is Svt64 of svt64.h - the
// one jstsp_svt_f64 and jstsp_proposed_algorithm_f64 use: Gram on the smaller side, in-LDS Jacobi for n <= 64, the global-memory
// Jacobi of vamp64.hip for 64 < n <= 512, non-positive eigenvalues dropped - and runs to convergence in every iteration: no warm
// start, no early stop, no environment switch.  sigma_max^2 is lambda_max of the same Gram (Svt64::lambda_max).  The two updates
// are element-wise kernels; every reduction lives in the products and the Jacobi, which sum in a fixed order inside one trial: a
// repeated call returns the same bits and a trial's result does not depend on the batch around it (for 64 < n the global Jacobi is
// told to leave a converged matrix alone while its batch mates are still swept: Svt64::freeze).
#include "svt64.h"

#include <algorithm>
#include <vector>

namespace jstsp {
namespace {

struct McPar {          // per-trial scalars: rho and the threshold tau / rho, both formed in float64
    double rho, thr;
};

inline dim3 mc_grid(long long per, int batch) { return dim3((unsigned)std::max<long long>(1, std::min<long long>((per + 255) / 256, 2048)), batch); }

// mc_svt.m:9   Y = Y + rho (OH - Omega .* X)
__global__ __launch_bounds__(256) void mc_svt_update64_kernel(long long nm, const McPar *par, double2 *Y, const double2 *OH, const double *Omega,
                                                              const double2 *X)
{
    const long long o = (long long)blockIdx.y * nm;
    const double rho = par[blockIdx.y].rho;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const double om = Omega[o + e];
        const double2 x = X[o + e], oh = OH[o + e];
        double2 y = Y[o + e];
        y.x += rho * (oh.x - om * x.x);
        y.y += rho * (oh.y - om * x.y);
        Y[o + e] = y;
    }
}

// mc_admm.m:24-26   Y = (OH + Z + rho X) ./ (Omega + rho);  Z = Z + rho (X - Y);  Zn = Y - Z/rho (the next svt argument, :22)
__global__ __launch_bounds__(256) void mc_admm_update64_kernel(long long nm, const McPar *par, double2 *Y, double2 *Z, const double2 *OH,
                                                               const double *Omega, const double2 *X, double2 *Zn)
{
    const long long o = (long long)blockIdx.y * nm;
    const double rho = par[blockIdx.y].rho;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const double den = Omega[o + e] + rho;
        const double2 x = X[o + e], oh = OH[o + e];
        double2 z = Z[o + e];
        const double2 y = make_double2((oh.x + z.x + rho * x.x) / den, (oh.y + z.y + rho * x.y) / den);
        z.x += rho * (x.x - y.x);
        z.y += rho * (x.y - y.y);
        Y[o + e] = y;
        Z[o + e] = z;
        Zn[o + e] = make_double2(y.x - z.x / rho, y.y - z.y / rho);
    }
}

int mc64_check(jstsp_ctx *ctx, const char *nm, int Mr, int Mt, int batch, int Imax, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_REQUIRE(Mr > 0 && Mt > 0 && batch > 0 && Imax >= 0, JSTSP_E_SHAPE, "%s: bad shape", nm);
    JSTSP_REQUIRE(std::min(Mr, Mt) <= P64_MAX_ORDER && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: min(Mr, Mt) = %d, batch = %d: the float64 eigen-decomposition is limited to order %d (batch 65535)", nm, std::min(Mr, Mt), batch,
                  P64_MAX_ORDER);
    return 0;
}

// rho and tau / rho of every trial
std::vector<McPar> mc64_params(int batch, const double *tau, const double *rho)
{
    std::vector<McPar> hp(batch);
    for (int t = 0; t < batch; ++t) hp[t] = McPar{rho[t], tau[t] / rho[t]};
    return hp;
}

}  // namespace
}  // namespace jstsp

using namespace jstsp;

extern "C" {

int jstsp_mc_svt_f64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *OH_, const double *Omega_, int Imax, const double *tau,
                     const double *rho, jstsp_c64 *X_out, int memspace)
{
    const char *nmf = "mc_svt (float64)";
    JSTSP_TRY(mc64_check(ctx, nmf, Mr, Mt, batch, Imax, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(OH_ && Omega_ && tau && rho && X_out, JSTSP_E_NULL, "%s: NULL argument", nmf);
    const bool host = memspace == JSTSP_HOST;
    const size_t nm1 = (size_t)Mr * Mt, nm = nm1 * batch, z2 = sizeof(double2);
    hipStream_t st = ctx->stream;
    const std::vector<McPar> hp = mc64_params(batch, tau, rho);
    const McPar *par;
    const double2 *OH;
    const double *Omega;
    double2 *X, *Y;
    Svt64 sv;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nmf, batch, [&](Slab &w, int b) {
        const size_t e = nm1 * b;
        par = w.in(hp.data(), b, true);
        OH = w.in(reinterpret_cast<const double2 *>(OH_), e, host);
        Omega = w.in(Omega_, e, host);
        X = w.out(reinterpret_cast<double2 *>(X_out), e, host);
        Y = w.get<double2>(e);
        sv.layout(w, Mr, Mt, b);
    }));
    JSTSP_HIP(hipStreamSynchronize(st));    // (hp is this call's own: copied before it goes out of scope on any path)
    sv.freeze = true;                       // a trial's bits do not depend on the batch around it, also for 64 < n
    JSTSP_HIP(hipMemsetAsync(Y, 0, nm * z2, st));                                                      // mc_svt.m:5
    JSTSP_HIP(hipMemsetAsync(X, 0, nm * z2, st));
    const dim3 g = mc_grid((long long)nm1, batch);
    for (int it = 0; it < Imax; ++it) {                                                                // :7
        JSTSP_TRY(sv.apply(st, Y, &par->thr, (long long)(sizeof(McPar) / sizeof(double)), X));        // :8
        hipLaunchKernelGGL(mc_svt_update64_kernel, g, dim3(256), 0, st, (long long)nm1, par, Y, OH, Omega, X);     // :9
        JSTSP_HIP(hipGetLastError());
    }
    if (host) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(X_out), X, nm));
    JSTSP_HIP(hipStreamSynchronize(st));
    return 0;
}

int jstsp_mc_admm_f64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *Htrue_, const jstsp_c64 *OH_, const double *Omega_, int Imax,
                      const double *tau, const double *rho, jstsp_c64 *X_out, double *ce_out, int memspace)
{
    const char *nmf = "mc_admm (float64)";
    JSTSP_TRY(mc64_check(ctx, nmf, Mr, Mt, batch, Imax, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(OH_ && Omega_ && tau && rho && X_out, JSTSP_E_NULL, "%s: NULL argument", nmf);
    JSTSP_REQUIRE(!ce_out || Htrue_, JSTSP_E_NULL, "%s: convergence_error needs Htrue", nmf);
    const bool host = memspace == JSTSP_HOST, want_ce = ce_out != nullptr;
    const size_t nm1 = (size_t)Mr * Mt, nm = nm1 * batch, z2 = sizeof(double2);
    hipStream_t st = ctx->stream;
    const std::vector<McPar> hp = mc64_params(batch, tau, rho);
    const McPar *par;
    const double2 *OH, *Htrue = nullptr;
    const double *Omega;
    double2 *X, *Y, *Z, *Zn, *D = nullptr;
    double *ce = nullptr, *num = nullptr, *den = nullptr;
    Svt64 sv;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nmf, batch, [&](Slab &w, int b) {
        const size_t e = nm1 * b;
        par = w.in(hp.data(), b, true);
        OH = w.in(reinterpret_cast<const double2 *>(OH_), e, host);
        Omega = w.in(Omega_, e, host);
        X = w.out(reinterpret_cast<double2 *>(X_out), e, host);
        Y = w.get<double2>(e); Z = w.get<double2>(e); Zn = w.get<double2>(e);
        if (want_ce) {
            Htrue = w.in(reinterpret_cast<const double2 *>(Htrue_), e, host);
            ce = w.out(ce_out, (size_t)b * std::max(Imax, 1), host);
            D = w.get<double2>(e); num = w.get<double>(b); den = w.get<double>(b);
        }
        sv.layout(w, Mr, Mt, b);
    }));
    JSTSP_HIP(hipStreamSynchronize(st));    // (hp is this call's own: copied before it goes out of scope on any path)
    sv.freeze = true;                       // a trial's bits do not depend on the batch around it, also for 64 < n
    for (double2 *p : {X, Y, Z, Zn}) JSTSP_HIP(hipMemsetAsync(p, 0, nm * z2, st));                    // mc_admm.m:6-8
    if (want_ce) JSTSP_TRY(sv.lambda_max(st, Htrue, den));
    const dim3 g = mc_grid((long long)nm1, batch);
    for (int it = 0; it < Imax; ++it) {                                                                // :20
        JSTSP_TRY(sv.apply(st, Zn, &par->thr, (long long)(sizeof(McPar) / sizeof(double)), X));       // :22
        hipLaunchKernelGGL(mc_admm_update64_kernel, g, dim3(256), 0, st, (long long)nm1, par, Y, Z, OH, Omega, X, Zn);     // :24-26
        if (want_ce) {                                                                                 // :28
            hipLaunchKernelGGL(diff64_kernel, dim3((unsigned)std::min<size_t>((nm + 255) / 256, 4096)), dim3(256), 0, st, (long long)nm, X, Htrue, D);
            JSTSP_TRY(sv.lambda_max(st, D, num));
            hipLaunchKernelGGL(ratio64_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, Imax, it, num, den, ce);
        }
        JSTSP_HIP(hipGetLastError());
    }
    if (host) {
        JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(X_out), X, nm));
        if (want_ce && Imax > 0) JSTSP_TRY(s.copy_back(ce_out, ce, (size_t)batch * Imax));
    }
    JSTSP_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
