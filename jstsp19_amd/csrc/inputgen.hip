// Device-side construction of the solver inputs for a batch of Monte-Carlo trials — the caller
// side of the hot path (plot_errorVSsnr.m:57-136): channel, pilots, noise, the random spatial
// sampling measurement, the dictionary factors and the hyper-parameters, all born in HBM.
//
//   wideband_mmwave_channel.m:1-39  -> channel_kernel (+ two GEMMs for Zbar = Dr' H_l Dt)
//   qam4mod.m:7-8, plot_errorVSsnr.m:63-67, proposed_hbf.m:15-18 -> pilots_kernel (rows of the Hermitian Toeplitz)
//   proposed_hbf.m:19-22            -> R = [H_1 .. H_L] Psi + sqrt(var/2) noise      (one GEMM, noise as the beta term)
//   proposed_hbf.m:36-42            -> omega_kernel (Mr smallest of Mr_e uniform keys per column), mask_kernel
//   plot_errorVSsnr.m:127-130       -> hyper_kernel (tau_Y, tau_Z, rho from the 6th largest eigenvalue of Y'Y)
//   plot_errorVSsnr.m:132-136       -> A = W_e' Dr, B_l = Dt' Psi_l                   (GEMMs)
//   plot_errorVSsnr.m:143           -> indx_S: stable descending sort of |vec(Zbar)| (64-bit keys, segmented radix sort)
//   plot_errorVSsnr_nyuwireless.m:62-68 -> a channel the caller supplies instead of the drawn one (jstsp_build_trials_from_channel_c32):
//                                      given_channel_sigma_kernel (norm(H_l), the non-finite / zero flag), given_channel_pack_kernel
//   wideband_mmwave_channel.m:19-24 over a sequence of frames (jstsp_build_trials_tracked_c32) -> tracked_gain_kernel: fixed angles,
//                                      gains by a first-order autoregression in closed form; channel_kernel on (g_f, u_r, u_t)
//   wideband_mmwave_channel.m:56-62 with angles that walk (jstsp_build_trials_tracked_drift_c32) -> drift_walk_kernel: phi_f - phi_0,
//                                      channel_drift_kernel on (g_f, phi_f)
//
// Random numbers: Philox4x32-10, key = mix(seed, sweep index, global trial index), counter =
// (element index, stream id) — a trial's inputs do not depend on the batch it is drawn in or
// on how trials are sharded over GPUs.
#include "inputgen.h"
#include "svt64.h"
#include <hipcub/hipcub.hpp>
#include <cstring>

using namespace jstsp;

namespace {

// Omega(:, j): ones on the Mr rows with the smallest of Mr_e uniform keys (= randperm(Mr_e)(1:Mr), proposed_hbf.m:37-40)
__global__ __launch_bounds__(256) void omega_kernel(Model m, uint64_t seed, uint64_t sweep, long long trial0,
                                                    float *Omega)
{
    extern __shared__ uint32_t keys[];
    const int t = blockIdx.y, j = blockIdx.x;
    const uint64_t key = mix_key(seed, sweep, (uint64_t)(trial0 + t));
    for (int i = threadIdx.x; i < m.Mr_e; i += 256)
        keys[i] = philox((uint64_t)j * m.Mr_e + i, ST_OMEGA, key).x;
    __syncthreads();
    for (int i = threadIdx.x; i < m.Mr_e; i += 256) {
        const uint32_t ki = keys[i];
        int rank = 0;
        for (int k = 0; k < m.Mr_e; ++k) {
            const uint32_t kk = keys[k];
            rank += (kk < ki) || (kk == ki && k < i);
        }
        Omega[((size_t)t * m.Tp + j) * m.Mr_e + i] = rank < m.Mr ? 1.f : 0.f;
    }
}

// ---- gains of frame f of a tracked sequence (jstsp_build_trials_tracked_c32): the first-order autoregression
//      g_f = corr g_{f-1} + sqrt(1 - corr^2) w_f in closed form,
//        g_f = corr^f w_0 + sqrt(1 - corr^2) sum_{k=1..f} corr^(f-k) w_k,
//      w_k[i] the draw of draw_small_kernel (wideband_mmwave_channel.m:19) at Philox element i + (k << 32): w_0 is that kernel's
//      gain.  Accumulated in float64 in ascending k, one fma per term and component on the widened fp32 draws, rounded once to
//      fp32.  A term whose coefficient is exactly zero is skipped, so frame 0 and corr = 1 give the bits of w_0 and corr = 0
//      gives w_f.  O(frame) Philox calls per gain; a gain is a function of (seed, sweep, trial, frame, corr) alone.
//      Grid (ceil(L*Np / 64), batch), one gain per thread.
__global__ __launch_bounds__(64) void tracked_gain_kernel(Model m, uint64_t seed, uint64_t sweep, long long trial0, int frame,
                                                          double corr, float2 *gains)
{
    const int t = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
    if (i >= m.L * m.Np) return;
    const uint64_t key = mix_key(seed, sweep, (uint64_t)(trial0 + t));
    const double s = sqrt(1.0 - corr * corr);
    double ax = 0.0, ay = 0.0;
    for (int k = 0; k <= frame; ++k) {
        const double c = (k == 0 ? 1.0 : s) * pow(corr, (double)(frame - k));
        if (c == 0.0) continue;
        const uint4 w = philox((uint64_t)i + ((uint64_t)k << 32), ST_GAIN, key);
        const float2 g = normal2(w.x, w.y);
        ax = fma(c, (double)(g.x * 0.70710678f), ax);
        ay = fma(c, (double)(g.y * 0.70710678f), ay);
        if (s == 0.0) break;                        // corr = 1: only w_0 has a coefficient
    }
    gains[(size_t)t * m.L * m.Np + i] = make_float2((float)ax, (float)ay);
}

// ---- angle offsets of frame f of a drifting sequence (jstsp_build_trials_tracked_drift_c32): a random walk per path and array
//      end, phi_f = phi_0 + drift * sum_{k=1..f} z_k, z_k[p] the first component of normal2 on the Philox word at element
//      p + (k << 32) of the stream ST_UR (receive) / ST_UT (transmit) - element p at k = 0 stays the uniform draw u of
//      draw_small_kernel.  The widened fp32 normals are summed in float64 in ascending k and multiplied ONCE by drift, so the
//      offsets are exactly linear in drift; the one addition to phi_0 is channel_drift_kernel's.  O(frame) Philox calls per angle;
//      an offset is a function of (seed, sweep, trial, frame, drift) alone.  Grid (ceil(2*Np / 64), batch), one (path, end) per
//      thread: i < Np receive, otherwise transmit.
__global__ __launch_bounds__(64) void drift_walk_kernel(Model m, uint64_t seed, uint64_t sweep, long long trial0, int frame,
                                                        double drift, double *dphi_r, double *dphi_t)
{
    const int t = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
    if (i >= 2 * m.Np) return;
    const bool rx = i < m.Np;
    const int p = rx ? i : i - m.Np;
    const uint64_t key = mix_key(seed, sweep, (uint64_t)(trial0 + t));
    double acc = 0.0;
    for (int k = 1; k <= frame; ++k) {
        const uint4 w = philox((uint64_t)p + ((uint64_t)k << 32), rx ? ST_UR : ST_UT, key);
        acc += (double)normal2(w.x, w.y).x;
    }
    (rx ? dphi_r : dphi_t)[(size_t)t * m.Np + p] = drift * acc;
}

// ---- dictionaries (trial-independent): Dr, Dt (wideband_mmwave_channel.m:9-10), ZC beamformer (createBeamformer.m:15-16)
__global__ void dict_kernel(int rows, int cols, int kind, float2 *D)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)rows * cols) return;
    const int n = (int)(i % rows), g = (int)(i / rows);
    float s, c;
    if (kind == 0) {            // 1/sqrt(rows) exp(-j 2 pi n g / cols)
        const long long r = ((long long)n * g) % cols;
        sincospif(-2.0f * (float)r / (float)cols, &s, &c);
    } else {                    // 1/sqrt(N) exp(-j 11 pi n (g+1) / N),  N = rows
        const long long r = (11ll * n * (g + 1)) % (2ll * rows);
        sincospif(-(float)r / (float)rows, &s, &c);
    }
    const float sc = rsqrtf((float)rows);
    D[i] = make_float2(c * sc, s * sc);
}

// ---- pilots: Psi[t] (Nt*L x Tp), row (s + Nt*l), column j = toeplitz(s_s)(l, j): s(|j-l|), conjugated below the diagonal
//      sym: the pilot symbols [t][s][Tp]; scale: 1 (4-QAM values) or 1/sqrt(2) (Gaussian draws, ...training.m:20)
__global__ __launch_bounds__(256) void pilots_kernel(Model m, const float2 *sym, float scale, float2 *Psi)
{
    const int t = blockIdx.y;
    const long long n_el = (long long)m.NtL * m.Tp;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n_el; e += (long long)gridDim.x * 256) {
        const int row = (int)(e % m.NtL), j = (int)(e / m.NtL);
        const int s = row % m.Nt, l = row / m.Nt;
        const int d = j - l;
        const float2 v = sym[((size_t)t * m.Nt + s) * m.Tp + (d < 0 ? -d : d)];
        Psi[(size_t)t * n_el + e] = make_float2(v.x * scale, (d < 0 ? -v.y : v.y) * scale);
    }
}

__global__ __launch_bounds__(256) void mask_kernel(long long nm, const float *Omega, const float2 *WR, float2 *subY)
{
    const long long base = (long long)blockIdx.y * nm;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nm; i += (long long)gridDim.x * 256) {
        const float o = Omega[base + i];
        const float2 w = WR[base + i];
        subY[base + i] = make_float2(o * w.x, o * w.y);                 // proposed_hbf.m:42
    }
}

__device__ __forceinline__ double block_sum256(double v, double *sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// tau_Y = 1/||Y||_F^2, tau_Z = 1/(2 ||Zbar||_F^2), rho = sqrt(lambda_6(Y'Y) / ||Y||_F^2)   (plot_errorVSsnr.m:127-130)
// lam: the n = min(N, M) non-zero-capable eigenvalues of the Gram; eigs() returns the 6 largest of the M x M matrix.
__global__ __launch_bounds__(256) void hyper_kernel(long long nm, long long nz, int n, int Mcols, const float2 *subY,
                                                    const float2 *Zbar, const float *lam, double *hyp, int rho_max,
                                                    double rho_scale)
{
    __shared__ double sh[4];
    __shared__ float sl[128];
    const int t = blockIdx.x;
    double fy = 0, fz = 0;
    for (long long i = threadIdx.x; i < nm; i += 256) {
        const float2 v = subY[(long long)t * nm + i];
        fy += (double)v.x * v.x + (double)v.y * v.y;
    }
    for (long long i = threadIdx.x; i < nz; i += 256) {
        const float2 v = Zbar[(long long)t * nz + i];
        fz += (double)v.x * v.x + (double)v.y * v.y;
    }
    fy = block_sum256(fy, sh);
    fz = block_sum256(fz, sh);
    for (int i = threadIdx.x; i < n; i += 256) sl[i] = lam[(size_t)t * n + i];
    __syncthreads();
    if (threadIdx.x == 0) {
        // 0-based position in the descending list of Mcols eigenvalues: min(eigs(.)) = the 6th, max(eigs(.)) = the 1st
        const int want = rho_max ? 0 : min(5, Mcols - 1);
        double l6 = 0.0;
        if (want < n) {
            // the (want+1)-th largest: rank by counting (n <= 128)
            for (int i = 0; i < n; ++i) {
                int rank = 0;
                for (int k = 0; k < n; ++k) rank += (sl[k] > sl[i]) || (sl[k] == sl[i] && k < i);
                if (rank == want) l6 = fmax((double)sl[i], 0.0);
            }
        }
        hyp[3 * t + 0] = 1.0 / fy;
        hyp[3 * t + 1] = 0.5 / fz;
        hyp[3 * t + 2] = rho_scale * sqrt(l6 / fy);
    }
}

// 64-bit sort keys: high word = ~bits(|z|^2) (ascending key = descending magnitude), low word = index (stable)
__global__ __launch_bounds__(256) void sortkey_kernel(long long total, long long nz, const float2 *Zbar, uint64_t *keys)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        keys[i] = ((uint64_t)support_key(Zbar[i]) << 32) | (uint64_t)(uint32_t)(i % nz);     // (support_key.h)
    }
}
__global__ __launch_bounds__(256) void sortidx_kernel(long long total, const uint64_t *keys, int32_t *indx)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
        indx[i] = (int32_t)(uint32_t)keys[i] + 1;                       // 1-based as MATLAB
}
__global__ void offsets_kernel(int batch, long long nz, int *off)
{
    for (int i = threadIdx.x; i <= batch; i += blockDim.x) off[i] = (int)(i * nz);
}


// ---- a supplied channel (plot_errorVSsnr_nyuwireless.m:62-68) ---------------------------------------------------------------------
// Tap l of channel ch: X = Hsrc + ch * chanStride + l * tapStride, entry (r, s) at r + ldr * s, the leading Nr x Nt block used (:63-64).
// One workgroup per (channel, tap), blockIdx.x = l + L * ch.  s = norm(X) (:65, the largest singular value) from the Hermitian Gram
// of the smaller side in float64: X is first scaled by 2^-e, e the frexp exponent of its largest finite |component| (exact, as
// finite_max_exponent of ws64.h does for OMP), every Gram entry is one fma chain over the long side in index order (a result does
// not depend on the batch it is computed in; G(j, i) = conj(G(i, j)) on the bits), lambda_max by the in-LDS Jacobi of svt64.h and
// s = 2^e sqrt(lambda_max).  A NaN / Inf in the block, or (zero_is_bad) an all-zero block, lowers *flag to 4 * blockIdx.x + 1 / + 2:
// the smallest index wins, so the word is the same from run to run.  want_s = 0: the check only (no LDS, any order).
__global__ __launch_bounds__(256) void given_channel_sigma_kernel(int Nr, int Nt, int L, const float2 *Hsrc, int ldr, long long tapStride,
                                                                  long long chanStride, int want_s, int zero_is_bad, double *sig,
                                                                  unsigned long long *flag)
{
    extern __shared__ double2 gsm[];
    __shared__ double red[4];
    const int tid = threadIdx.x, l = blockIdx.x % L, ch = blockIdx.x / L;
    const float2 *X = Hsrc + (long long)ch * chanStride + (long long)l * tapStride;
    double vmax = 0.0;
    int bad = 0;
    for (int e = tid; e < Nr * Nt; e += 256) {
        const float2 v = X[(e % Nr) + (long long)ldr * (e / Nr)];
        const double ax = fabs((double)v.x), ay = fabs((double)v.y);
        if (ax <= DBL_MAX) vmax = fmax(vmax, ax); else bad = 1;            // (not NaN, not Inf)
        if (ay <= DBL_MAX) vmax = fmax(vmax, ay); else bad = 1;
    }
    bad = __syncthreads_or(bad);
    for (int o = 32; o > 0; o >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, o));
    if ((tid & 63) == 0) red[tid >> 6] = vmax;
    __syncthreads();
    vmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    if (bad || vmax == 0.0) {                                              // (the same for the whole workgroup)
        if (tid == 0) {
            if (bad || zero_is_bad) atomicMin(flag, 4ull * blockIdx.x + (bad ? 1ull : 2ull));
            sig[blockIdx.x] = bad ? nan("") : 0.0;
        }
        return;
    }
    if (!want_s) return;
    int ev = 0;
    (void)frexp(vmax, &ev);
    const double sc = ldexp(1.0, -ev);              // fp32 exponents: 2^-ev is a normal double and x * sc is exact
    const bool right = Nt <= Nr;                    // G = X^H X of order Nt; otherwise X X^H of order Nr
    const int n0 = right ? Nt : Nr, k = right ? Nr : Nt, n = (n0 + 1) & ~1, h2 = n / 2;
    double2 *H = gsm, *rs = H + (size_t)n * n;
    double *rc = reinterpret_cast<double *>(rs + h2);
    double dm = 0.0;
    for (int e = tid; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        double2 g = make_double2(0.0, 0.0);
        if (i < n0 && j < n0) {
            Dot4 d = {0.0, 0.0, 0.0, 0.0};
            for (int q = 0; q < k; ++q) {
                const float2 a = right ? X[q + (long long)ldr * i] : X[i + (long long)ldr * q];
                const float2 b = right ? X[q + (long long)ldr * j] : X[j + (long long)ldr * q];
                const double2 u = make_double2((double)a.x * sc, (double)a.y * sc), v = make_double2((double)b.x * sc, (double)b.y * sc);
                if (right) dot4_step(d, u, v);      // sum_q conj(X(q, i)) X(q, j)
                else dot4_step(d, v, u);            // sum_q X(i, q) conj(X(j, q))
            }
            g = make_double2(d.xx + d.yy, d.xy - d.yx);
        }
        if (i == j) { g.y = 0.0; dm = fmax(dm, fabs(g.x)); }
        H[e] = g;
    }
    for (int o = 32; o > 0; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o));
    __syncthreads();                                // (red has been read by every thread)
    if ((tid & 63) == 0) red[tid >> 6] = dm;
    __syncthreads();
    const double EPS = 1.1102230246251565e-16;
    const double floor_abs = EPS * EPS * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    jacobi64_lds_sweeps<false>(n, H, nullptr, rs, rc, floor_abs);
    if (tid == 0) {
        double mx = H[0].x;
        for (int i = 1; i < n0; ++i) mx = fmax(mx, H[i + n * i].x);
        sig[blockIdx.x] = ldexp(sqrt(fmax(mx, 0.0)), ev);
    }
}

// Hmat[t] = [H_1 ... H_L] (Nr x Nt*L, the layout of channel_kernel) from the supplied taps: each entry scaled in float64 by 1, 1/s^2
// (plot_errorVSsnr_nyuwireless.m:65-66 as written: rho = 1/norm(H_l)^2, which leaves a tap of norm 1/s) or 1/s and rounded once
// to fp32; JSTSP_CHAN_ASIS stores the input bits.  chanStride = 0: one channel, scaled once per entry and written to every trial slot.
__global__ __launch_bounds__(256) void given_channel_pack_kernel(int Nr, int Nt, int L, int batch, const float2 *Hsrc, int ldr,
                                                                 long long tapStride, long long chanStride, int normalize,
                                                                 const double *sig, float2 *Hmat)
{
    const long long n_el = (long long)Nr * Nt * L;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n_el; e += (long long)gridDim.x * 256) {
        const int r = (int)(e % Nr);
        const int sl = (int)(e / Nr);
        const int s = sl % Nt, l = sl / Nt;
        const long long src = (long long)l * tapStride + r + (long long)ldr * s;
        float2 v = make_float2(0.f, 0.f);
        for (int t = blockIdx.y; t < batch; t += gridDim.y) {
            if (chanStride != 0 || t == (int)blockIdx.y) {
                v = Hsrc[(long long)t * chanStride + src];
                if (normalize != JSTSP_CHAN_ASIS) {
                    const double sg = sig[(chanStride != 0 ? (long long)t * L : 0) + l];
                    const double d = normalize == JSTSP_CHAN_REFERENCE ? sg * sg : sg;
                    v = make_float2((float)((double)v.x / d), (float)((double)v.y / d));
                }
            }
            Hmat[(size_t)t * n_el + e] = v;
        }
    }
}


template <class T> T *out_or_tmp(jstsp_ctx *ctx, T *user, size_t n, int memspace)
{
    if (user && memspace == JSTSP_DEVICE) return user;
    return ctx->arena.get<T>(n);
}

// The body of the three builders.  given == NULL: the channel of wideband_mmwave_channel.m from the Philox draws
// (jstsp_build_trials_c32); otherwise the caller's taps, cut and scaled (plot_errorVSsnr_nyuwireless.m:62-68) - draw_small_kernel
// and channel_kernel are then not launched.  tracked != NULL (with given == NULL): frame tracked->frame of a sequence whose geometry
// is the drawn one and whose gains follow tracked_gain_kernel; noise, pilots and Omega take the frame into their sweep word.
// tracked->drifting: the fourth source - the angles of that sequence walk (drift_walk_kernel) and channel_drift_kernel adds the offsets.
// Everything after Hmat is the same code.
int build_trials_impl(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx, long long trial0, int batch,
                      const GivenChannel *given, const TrackedChannel *tracked, const jstsp_trials *out, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "build_trials: NULL context");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "build_trials: bad memspace");
    JSTSP_REQUIRE(mp && out, JSTSP_E_NULL, "build_trials: NULL argument");
    if (tracked) {
        JSTSP_REQUIRE(tracked->corr >= 0.0 && tracked->corr <= 1.0, JSTSP_E_ARG,                    // (a NaN fails both)
                      "build_trials_tracked: corr must lie in [0, 1] (got %g)", tracked->corr);
        JSTSP_REQUIRE(tracked->frame >= 0 && tracked->frame <= 65535, JSTSP_E_ARG,
                      "build_trials_tracked: frame must lie in [0, 65535] (got %d)", tracked->frame);
        JSTSP_REQUIRE(!tracked->drifting || (tracked->drift >= 0.0 && tracked->drift <= DBL_MAX), JSTSP_E_ARG,  // (a NaN fails both)
                      "build_trials_tracked_drift: drift must be finite and >= 0 (got %g)", tracked->drift);
    }
    JSTSP_ENTER(ctx);
    Model m;
    m.Nt = mp->Nt; m.Nr = mp->Nr; m.L = mp->L; m.Tp = mp->T_prop; m.Mr = mp->Mr; m.Mr_e = mp->Mr_e;
    m.Gr = mp->Gr; m.Gt = mp->Gt; m.clusters = mp->clusters; m.rays = mp->rays;
    if (given) m.clusters = m.rays = 1;             // (ignored: nothing is drawn for the channel)
    JSTSP_REQUIRE(m.Nt > 0 && m.Nr > 0 && m.L > 0 && m.Tp > 0 && m.Gr > 0 && m.Gt > 0 && m.clusters > 0 && m.rays > 0 &&
                      batch > 0 && trial0 >= 0 && sweep_idx >= 0,
                  JSTSP_E_SHAPE, "build_trials: bad model dimensions");
    JSTSP_REQUIRE(m.Mr_e >= 1 && m.Mr_e <= m.Nr && m.Mr >= 1 && m.Mr <= m.Mr_e, JSTSP_E_SHAPE,
                  "build_trials: need 1 <= Mr <= Mr_e <= Nr");
    JSTSP_REQUIRE(m.L <= m.Tp, JSTSP_E_SHAPE, "build_trials: L > T_prop");
    JSTSP_REQUIRE((mp->beamformer == JSTSP_BF_ZC || mp->beamformer == JSTSP_BF_DFT) &&
                      (mp->rho_rule == JSTSP_RHO_MIN6 || mp->rho_rule == JSTSP_RHO_MAX) && mp->rho_scale >= 0.0,
                  JSTSP_E_ARG, "build_trials: bad beamformer / rho_rule / rho_scale");
    JSTSP_REQUIRE(mp->noise_var >= 0.0, JSTSP_E_ARG, "build_trials: negative noise variance");
    JSTSP_REQUIRE(mp->pilots == JSTSP_PILOTS_QAM4 || mp->pilots == JSTSP_PILOTS_GAUSS, JSTSP_E_ARG, "build_trials: bad pilots kind");
    const int gauss = mp->pilots == JSTSP_PILOTS_GAUSS;
    JSTSP_REQUIRE(mp->T_hbf >= 0 && mp->T_hbf <= m.Tp, JSTSP_E_SHAPE, "build_trials: T_hbf outside [0, T_prop]");
    m.Np = m.clusters * m.rays; m.NtL = m.Nt * m.L; m.G2 = m.L * m.Gt;
    const int N = m.Mr_e, M = m.Tp, nG = std::min(N, M), Th = mp->T_hbf;
    const bool want_hyp = out->tau_Y || out->tau_Z || out->rho;
    JSTSP_REQUIRE(!want_hyp || nG <= 128, JSTSP_E_UNSUPPORTED, "build_trials: rho needs min(Mr_e, T_prop) <= 128");
    const size_t lds_ch = given ? 0 : ((size_t)(m.Nr + m.Nt) * m.Np + (size_t)m.L * m.Np) * sizeof(float2);
    JSTSP_REQUIRE(lds_ch <= 150 * 1024 && (size_t)m.Mr_e * 4 <= 64 * 1024, JSTSP_E_UNSUPPORTED,
                  "build_trials: steering tables exceed the LDS");
    const bool want_hbf = Th > 0 && (out->Y_hbf || out->A_hbf || out->B_hbf);
    if (given)
        JSTSP_REQUIRE(!out->gains && !out->u_r && !out->u_t, JSTSP_E_ARG,
                      "build_trials_from_channel: gains, u_r and u_t must be NULL - nothing is drawn for a supplied channel");

    const size_t b = (size_t)batch;
    const size_t nH = (size_t)m.Nr * m.NtL, nPsi = (size_t)m.NtL * m.Tp, nR = (size_t)m.Nr * m.Tp, nY = (size_t)N * M,
                 nB = (size_t)m.G2 * M, nZ = (size_t)m.Gr * m.G2, nA = (size_t)N * m.Gr, nQ = (size_t)m.Nt * m.Tp;
    // ---- workspace -------------------------------------------------------------------------
    JSTSP_REQUIRE(b * nZ < (1ull << 31), JSTSP_E_UNSUPPORTED, "build_trials: batch * Gr * G2 exceeds 2^31");
    size_t sort_tmp = 0;
    if (out->indx_S)
        JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                   (int)(b * nZ), batch, (const int *)nullptr,
                                                   (const int *)nullptr, 0, 64, ctx->stream));
    size_t need = 0;
    auto acc = [&](size_t bytes) { need += rnd256(bytes); };
    acc(b * m.L * m.Np * 8); acc(b * m.Np * 4); acc(b * m.Np * 4); acc(b * nR * 8); acc(b * nQ); acc(b * nQ * 8);       // draws
    acc((size_t)m.Nr * m.Gr * 8); acc((size_t)m.Nt * m.Gt * 8); acc((size_t)m.Nr * m.Nr * 8);         // Dr, Dt, W
    acc(b * nH * 8); acc(b * nPsi * 8); acc(b * nR * 8); acc(b * nY * 8); acc(b * nY * 8); acc(b * nY * 4);
    acc(nA * 8); acc(b * nB * 8); acc(b * nZ * 8); acc(b * (size_t)m.Gr * m.NtL * 8);
    acc(b * 3 * sizeof(double)); acc(b * nG * 4);
    need += GramWS::bytes(N, M, batch, true);
    if (out->indx_S) { acc(b * nZ * 8); acc(b * nZ * 8); acc(sort_tmp); acc((b + 1) * 8); acc(b * nZ * 4); }
    if (want_hbf) { acc(b * (size_t)m.Nr * Th * 8); acc((size_t)m.Nr * m.Gr * 8); acc(b * (size_t)m.G2 * Th * 8); }
    const bool drifting = tracked && tracked->drifting;
    if (drifting) { acc(b * m.Np * 8); acc(b * m.Np * 8); }
    // a supplied channel: given_channel_hmat checks its form, reserves the workspace with its own share on top, and decides the
    // refusals before any output is written
    float2 *Hgiven = nullptr;
    if (given) {
        JSTSP_TRY(given_channel_hmat(ctx, m.Nr, m.Nt, m.L, trial0, batch, *given, memspace, need + 4096,
                                     memspace == JSTSP_DEVICE ? reinterpret_cast<float2 *>(out->H) : nullptr, &Hgiven));
    } else {
        JSTSP_TRY(ctx->arena.reserve(need + 4096));
        ctx->arena.reset();
    }
    Arena &ar = ctx->arena;
    hipStream_t st = ctx->stream;
    float2 *gains = given ? nullptr : out_or_tmp(ctx, reinterpret_cast<float2 *>(out->gains), b * m.L * m.Np, memspace);
    float *u_r = given ? nullptr : out_or_tmp(ctx, out->u_r, b * m.Np, memspace),
          *u_t = given ? nullptr : out_or_tmp(ctx, out->u_t, b * m.Np, memspace);
    float2 *noise = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->noise), b * nR, memspace);
    uint8_t *qam = out_or_tmp(ctx, out->qam_idx, b * nQ, memspace);
    float2 *psym = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->pilot_sym), b * nQ, memspace);
    float2 *Dr = ar.get<float2>((size_t)m.Nr * m.Gr), *Dt = ar.get<float2>((size_t)m.Nt * m.Gt),
           *W = ar.get<float2>((size_t)m.Nr * m.Nr);
    float2 *Hmat = given ? Hgiven : out_or_tmp(ctx, reinterpret_cast<float2 *>(out->H), b * nH, memspace);
    float2 *Psi = ar.get<float2>(b * nPsi), *R = ar.get<float2>(b * nR), *WR = ar.get<float2>(b * nY);
    float2 *subY = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->subY), b * nY, memspace);
    float *Omega = out_or_tmp(ctx, out->Omega, b * nY, memspace);
    float2 *A = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->A), nA, memspace);
    float2 *B = out->B ? out_or_tmp(ctx, reinterpret_cast<float2 *>(out->B), b * nB, memspace) : nullptr;
    float2 *Zbar = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->Zbar), b * nZ, memspace);
    float2 *T1 = ar.get<float2>(b * (size_t)m.Gr * m.NtL);
    double *hyp = ar.get<double>(b * 3);
    float *lam = ar.get<float>(b * nG);
    double *dphi_r = drifting ? out_or_tmp(ctx, tracked->dphi_r, b * m.Np, memspace) : nullptr,
           *dphi_t = drifting ? out_or_tmp(ctx, tracked->dphi_t, b * m.Np, memspace) : nullptr;
    JSTSP_REQUIRE(!drifting || (dphi_r && dphi_t), JSTSP_E_NOMEM, "build_trials: workspace exhausted");
    JSTSP_REQUIRE((given || (gains && u_r && u_t)) && noise && qam && psym && Dr && Dt && W && Hmat && Psi && R && WR && subY && Omega &&
                      A && (B || !out->B) && Zbar && T1 && hyp && lam,
                  JSTSP_E_NOMEM, "build_trials: workspace exhausted");
    // the sequence (geometry, gain innovations) is keyed by the sweep index; what a frame draws anew by (sweep index, frame)
    const uint64_t sw = (uint64_t)sweep_idx, swf = sw + ((uint64_t)(tracked ? tracked->frame : 0) << 32);

    // ---- draws ------------------------------------------------------------------------------
    if (!given) draw_small_kernel<<<batch, 64, 0, st>>>(m, seed, sw, trial0, gains, u_r, u_t);
    if (tracked)                                // (w_0 of draw_small_kernel is overwritten by g_f; frame 0: by its own bits)
        tracked_gain_kernel<<<dim3((m.L * m.Np + 63) / 64, batch), 64, 0, st>>>(m, seed, sw, trial0, tracked->frame, tracked->corr,
                                                                                 gains);
    if (drifting)
        drift_walk_kernel<<<dim3((2 * m.Np + 63) / 64, batch), 64, 0, st>>>(m, seed, sw, trial0, tracked->frame, tracked->drift,
                                                                            dphi_r, dphi_t);
    draw_noise_qam_kernel<<<dim3(grid_for((long long)std::max(nR, nQ), 1024), batch), 256, 0, st>>>(m, seed, swf, trial0,
                                                                                                      noise, qam, mp->shared_pilots, gauss, psym);
    omega_kernel<<<dim3(m.Tp, batch), 256, (size_t)m.Mr_e * 4, st>>>(m, seed, swf, trial0, Omega);
    // ---- dictionaries -------------------------------------------------------------------------
    dict_kernel<<<grid_for((long long)m.Nr * m.Gr), 256, 0, st>>>(m.Nr, m.Gr, 0, Dr);
    dict_kernel<<<grid_for((long long)m.Nt * m.Gt), 256, 0, st>>>(m.Nt, m.Gt, 0, Dt);
    // createBeamformer.m: 'ZC' (:15-16, plot_errorVSsnr.m:124) or 'fft' / 'ps' (:5,:12-13 - the same unitary DFT matrix)
    dict_kernel<<<grid_for((long long)m.Nr * m.Nr), 256, 0, st>>>(m.Nr, m.Nr, mp->beamformer == JSTSP_BF_ZC ? 1 : 0, W);
    // ---- channel, pilots ------------------------------------------------------------------------
    if (drifting)
        channel_drift_kernel<<<dim3(grid_for((long long)nH, 64), batch), 256, lds_ch, st>>>(m, gains, u_r, u_t, dphi_r, dphi_t, Hmat);
    else if (!given)                            // (a supplied channel is in Hmat already)
        channel_kernel<<<dim3(grid_for((long long)nH, 64), batch), 256, lds_ch, st>>>(m, gains, u_r, u_t, Hmat);
    pilots_kernel<<<dim3(grid_for((long long)nPsi, 1024), batch), 256, 0, st>>>(m, psym, gauss ? 0.70710678f : 1.f, Psi);
    JSTSP_HIP(hipGetLastError());
    // R = [H_1..H_L] Psi + sqrt(var/2) noise                                     proposed_hbf.m:19-22
    JSTSP_TRY(gemm(ctx, 'N', 'N', m.Nr, m.Tp, m.NtL, batch, Mat{Hmat, (long long)nH, m.Nr}, Mat{Psi, (long long)nPsi, m.NtL},
                   R, (long long)nR, m.Nr, 1.f, noise, (long long)nR, m.Nr, (float)std::sqrt(mp->noise_var / 2.0)));
    // subY = Omega .* (W_e' R)                                                   proposed_hbf.m:42
    JSTSP_TRY(gemm(ctx, 'C', 'N', N, M, m.Nr, batch, Mat{W, 0, m.Nr}, Mat{R, (long long)nR, m.Nr}, WR, (long long)nY, N));
    mask_kernel<<<dim3(grid_for((long long)nY, 1024), batch), 256, 0, st>>>((long long)nY, Omega, WR, subY);
    // Zbar = [Dr' H_1 Dt ... Dr' H_L Dt]                                         wideband_mmwave_channel.m:35,38
    JSTSP_TRY(gemm(ctx, 'C', 'N', m.Gr, m.NtL, m.Nr, batch, Mat{Dr, 0, m.Nr}, Mat{Hmat, (long long)nH, m.Nr}, T1,
                   (long long)m.Gr * m.NtL, m.Gr));
    JSTSP_TRY(gemm(ctx, 'N', 'N', m.Gr, m.Gt, m.Nt, batch * m.L, Mat{T1, (long long)m.Gr * m.Nt, m.Gr}, Mat{Dt, 0, m.Nt},
                   Zbar, (long long)m.Gr * m.Gt, m.Gr));
    // A = W_e' Dr ; B_l = Dt' Psi_l                                              plot_errorVSsnr.m:132-136
    JSTSP_TRY(gemm(ctx, 'C', 'N', N, m.Gr, m.Nr, 1, Mat{W, 0, m.Nr}, Mat{Dr, 0, m.Nr}, A, 0, N));
    if (B)
        for (int l = 0; l < m.L; ++l)
            JSTSP_TRY(gemm(ctx, 'C', 'N', m.Gt, M, m.Nt, batch, Mat{Dt, 0, m.Nt},
                           Mat{Psi + (size_t)l * m.Nt, (long long)nPsi, m.NtL}, B + (size_t)l * m.Gt, (long long)nB, m.G2));
    // ---- hyper-parameters ---------------------------------------------------------------------------
    if (want_hyp) {
        GramWS w;
        JSTSP_TRY(w.alloc(ar, N, M, batch, true));
        JSTSP_TRY(gram_partials(ctx, w, subY, (long long)nY));
        JSTSP_TRY(launch_eig(ctx, EIG_VECS, w.n, batch, w.Gpart, (long long)w.n * w.n * w.nsplit, w.nsplit,
                             (long long)w.n * w.n, nullptr, nullptr, w.Q, lam, w.Vg));
        hyper_kernel<<<batch, 256, 0, st>>>((long long)nY, (long long)nZ, w.n, M, subY, Zbar, lam, hyp,
                                            mp->rho_rule == JSTSP_RHO_MAX, mp->rho_scale > 0.0 ? mp->rho_scale : 1.0);
        JSTSP_HIP(hipGetLastError());
    }
    // ---- support ordering -------------------------------------------------------------------------------
    int32_t *indx = nullptr;
    if (out->indx_S) {
        uint64_t *k0 = ar.get<uint64_t>(b * nZ), *k1 = ar.get<uint64_t>(b * nZ);
        void *tmp = ar.get<char>(sort_tmp ? sort_tmp : 1);
        int *off = ar.get<int>(b + 1);
        indx = out_or_tmp(ctx, out->indx_S, b * nZ, memspace);
        JSTSP_REQUIRE(k0 && k1 && tmp && off && indx, JSTSP_E_NOMEM, "build_trials: workspace exhausted (sort)");
        offsets_kernel<<<1, 256, 0, st>>>(batch, (long long)nZ, off);
        sortkey_kernel<<<grid_for((long long)(b * nZ)), 256, 0, st>>>((long long)(b * nZ), (long long)nZ, Zbar, k0);
        JSTSP_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, sort_tmp, k0, k1, (int)(b * nZ), batch, off, off + 1, 0,
                                                             64, st));
        sortidx_kernel<<<grid_for((long long)(b * nZ)), 256, 0, st>>>((long long)(b * nZ), k1, indx);
        JSTSP_HIP(hipGetLastError());
    }
    // ---- conventional HBF measurement for the LS / VAMP baselines (plot_errorVSsnr.m:73-80, hbf.m:17-24) ----
    float2 *Yh = nullptr, *Ah = nullptr, *Bh = nullptr;
    if (want_hbf) {
        if (out->Y_hbf) {
            Yh = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->Y_hbf), b * (size_t)m.Nr * Th, memspace);
            JSTSP_REQUIRE(Yh, JSTSP_E_NOMEM, "build_trials: workspace exhausted (Y_hbf)");
            JSTSP_TRY(gemm(ctx, 'C', 'N', m.Nr, Th, m.Nr, batch, Mat{W, 0, m.Nr}, Mat{R, (long long)nR, m.Nr}, Yh,
                           (long long)m.Nr * Th, m.Nr));
        }
        if (out->A_hbf) {
            Ah = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->A_hbf), (size_t)m.Nr * m.Gr, memspace);
            JSTSP_REQUIRE(Ah, JSTSP_E_NOMEM, "build_trials: workspace exhausted (A_hbf)");
            JSTSP_TRY(gemm(ctx, 'C', 'N', m.Nr, m.Gr, m.Nr, 1, Mat{W, 0, m.Nr}, Mat{Dr, 0, m.Nr}, Ah, 0, m.Nr));
        }
        if (out->B_hbf) {
            JSTSP_REQUIRE(B, JSTSP_E_ARG, "build_trials: B_hbf requires B");
            Bh = out_or_tmp(ctx, reinterpret_cast<float2 *>(out->B_hbf), b * (size_t)m.G2 * Th, memspace);
            JSTSP_REQUIRE(Bh, JSTSP_E_NOMEM, "build_trials: workspace exhausted (B_hbf)");
            JSTSP_HIP(hipMemcpy2DAsync(Bh, (size_t)m.G2 * Th * 8, B, nB * 8, (size_t)m.G2 * Th * 8, batch,
                                       hipMemcpyDeviceToDevice, st));
        }
    }
    // ---- hand the arrays over ------------------------------------------------------------------------------
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->gains), gains, b * m.L * m.Np, memspace));
        JSTSP_TRY(stage_out(ctx, out->u_r, u_r, b * m.Np, memspace));
        JSTSP_TRY(stage_out(ctx, out->u_t, u_t, b * m.Np, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->noise), noise, b * nR, memspace));
        JSTSP_TRY(stage_out(ctx, out->qam_idx, qam, b * nQ, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->pilot_sym), psym, b * nQ, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->H), Hmat, b * nH, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->subY), subY, b * nY, memspace));
        JSTSP_TRY(stage_out(ctx, out->Omega, Omega, b * nY, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->A), A, nA, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->B), B, b * nB, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->Zbar), Zbar, b * nZ, memspace));
        JSTSP_TRY(stage_out(ctx, out->indx_S, indx, b * nZ, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->Y_hbf), Yh, b * (size_t)m.Nr * Th, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->A_hbf), Ah, (size_t)m.Nr * m.Gr, memspace));
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out->B_hbf), Bh, b * (size_t)m.G2 * Th, memspace));
        if (drifting) {
            JSTSP_TRY(stage_out(ctx, tracked->dphi_r, dphi_r, b * m.Np, memspace));
            JSTSP_TRY(stage_out(ctx, tracked->dphi_t, dphi_t, b * m.Np, memspace));
        }
    }
    // tau_Y, tau_Z, rho are host arrays in either memspace: the solver entry points take them from the host
    if (want_hyp) {
        std::vector<double> h(3 * b);
        JSTSP_HIP(hipMemcpyAsync(h.data(), hyp, 3 * b * sizeof(double), hipMemcpyDeviceToHost, st));
        JSTSP_HIP(hipStreamSynchronize(st));
        for (size_t t = 0; t < b; ++t) {
            if (out->tau_Y) out->tau_Y[t] = h[3 * t];
            if (out->tau_Z) out->tau_Z[t] = h[3 * t + 1];
            if (out->rho) out->rho[t] = h[3 * t + 2];
        }
    } else if (memspace == JSTSP_HOST) {
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

}  // namespace

// The cut and scale of a supplied channel (plot_errorVSsnr_nyuwireless.m:62-68) for every entry point that takes one
// (inputgen.h): the form of the arguments, norm(H_l) per tap, the refusals, then Hmat.
int jstsp::given_channel_hmat(jstsp_ctx *ctx, int Nr, int Nt, int L, long long trial0, int batch, const GivenChannel &g, int memspace,
                              size_t caller_bytes, float2 *Hmat_user, float2 **Hmat_out)
{
    JSTSP_REQUIRE(g.normalize == JSTSP_CHAN_ASIS || g.normalize == JSTSP_CHAN_REFERENCE || g.normalize == JSTSP_CHAN_UNIT, JSTSP_E_ARG,
                  "build_trials_from_channel: normalize must be JSTSP_CHAN_ASIS, _REFERENCE or _UNIT (got %d)", g.normalize);
    JSTSP_REQUIRE(g.H, JSTSP_E_NULL, "build_trials_from_channel: Hsrc is NULL");
    JSTSP_REQUIRE(g.ld_rows >= Nr && g.ld_cols >= Nt, JSTSP_E_SHAPE,
                  "build_trials_from_channel: the source taps are %d x %d, smaller than Nr x Nt = %d x %d", g.ld_rows, g.ld_cols, Nr, Nt);
    const bool shared_ch = g.stride == 0;
    const long long tap_stride = (long long)g.ld_rows * g.ld_cols;
    JSTSP_REQUIRE(g.stride == 0 || g.stride >= (long long)L * tap_stride, JSTSP_E_SHAPE,
                  "build_trials_from_channel: strideH = %lld is shorter than one channel, L * ld_rows * ld_cols = %lld", g.stride,
                  (long long)L * tap_stride);
    const bool need_s = g.normalize != JSTSP_CHAN_ASIS || g.sigma_max;
    JSTSP_REQUIRE(!need_s || std::min(Nr, Nt) <= P64_LDS_ORDER, JSTSP_E_UNSUPPORTED,
                  "build_trials_from_channel: the spectral norm of a tap needs min(Nr, Nt) <= %d (got %d); JSTSP_CHAN_ASIS without "
                  "sigma_max has no such limit", P64_LDS_ORDER, std::min(Nr, Nt));
    const size_t n_sig = (size_t)L * (shared_ch ? 1 : (size_t)batch);
    const size_t nHsrc = (shared_ch ? 0 : (size_t)(batch - 1) * (size_t)g.stride) + (size_t)L * (size_t)tap_stride;
    const size_t nH = (size_t)Nr * Nt * L;
    JSTSP_TRY(ctx->arena.reserve(caller_bytes + rnd256((n_sig + 1) * 8) + (memspace == JSTSP_HOST ? rnd256(nHsrc * 8) : 0) +
                                 (Hmat_user ? 0 : rnd256((size_t)batch * nH * 8))));
    ctx->arena.reset();
    hipStream_t st = ctx->stream;
    double *sig = ctx->arena.get<double>(n_sig + 1);            // s per (channel, tap), then the flag word of the call
    JSTSP_REQUIRE(sig, JSTSP_E_NOMEM, "build_trials_from_channel: workspace exhausted");
    const float2 *Hsrc = nullptr;
    JSTSP_TRY(stage_in(ctx, g.H, nHsrc, memspace, &Hsrc));
    unsigned long long *flag = reinterpret_cast<unsigned long long *>(sig + n_sig);
    JSTSP_HIP(hipMemsetAsync(flag, 0xFF, sizeof(*flag), st));
    const size_t sh = need_s ? jacobi_lds_bytes(std::min(Nr, Nt), false) : 0;
    if (sh > 48 * 1024)
        JSTSP_HIP(hipFuncSetAttribute((const void *)given_channel_sigma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    given_channel_sigma_kernel<<<(unsigned)n_sig, 256, sh, st>>>(Nr, Nt, L, Hsrc, g.ld_rows, tap_stride, g.stride, need_s ? 1 : 0,
                                                                 g.normalize != JSTSP_CHAN_ASIS ? 1 : 0, sig, flag);
    JSTSP_HIP(hipGetLastError());
    std::vector<double> h(n_sig + 1);
    JSTSP_HIP(hipMemcpyAsync(h.data(), sig, (n_sig + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    JSTSP_HIP(hipStreamSynchronize(st));
    unsigned long long w;
    memcpy(&w, &h[n_sig], sizeof(w));
    if (w != ~0ull) {
        const long long idx = (long long)(w / 4);
        const int tap = (int)(idx % L);
        const char *what = (w & 3) == 1 ? "has a NaN or Inf in its Nr x Nt block" : "is all zero, so 1/norm(H_l) does not exist";
        if (shared_ch) set_error("build_trials_from_channel: tap %d of the shared channel %s", tap, what);
        else set_error("build_trials_from_channel: tap %d of trial %lld %s", tap, trial0 + idx / L, what);
        return JSTSP_E_ILLCOND;
    }
    if (g.sigma_max) std::copy(h.begin(), h.begin() + n_sig, g.sigma_max);
    float2 *Hmat = Hmat_user ? Hmat_user : ctx->arena.get<float2>((size_t)batch * nH);
    JSTSP_REQUIRE(Hmat, JSTSP_E_NOMEM, "build_trials_from_channel: workspace exhausted");
    given_channel_pack_kernel<<<dim3(grid_for((long long)nH, 64), shared_ch ? std::min(batch, 16) : batch), 256, 0, st>>>(
        Nr, Nt, L, batch, Hsrc, g.ld_rows, tap_stride, g.stride, g.normalize, sig, Hmat);
    JSTSP_HIP(hipGetLastError());
    *Hmat_out = Hmat;
    return 0;
}

extern "C" int jstsp_build_trials_c32(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx,
                                      long long trial0, int batch, const jstsp_trials *out, int memspace)
{
    return build_trials_impl(ctx, mp, seed, sweep_idx, trial0, batch, nullptr, nullptr, out, memspace);
}

extern "C" int jstsp_build_trials_tracked_c32(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx,
                                              long long trial0, int batch, int frame, double corr, const jstsp_trials *out,
                                              int memspace)
{
    const TrackedChannel tr{frame, corr, 0, 0.0, nullptr, nullptr};
    return build_trials_impl(ctx, mp, seed, sweep_idx, trial0, batch, nullptr, &tr, out, memspace);
}

extern "C" int jstsp_build_trials_tracked_drift_c32(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx,
                                                    long long trial0, int batch, int frame, double corr, double drift,
                                                    const jstsp_trials *out, double *dphi_r, double *dphi_t, int memspace)
{
    const TrackedChannel tr{frame, corr, 1, drift, dphi_r, dphi_t};
    return build_trials_impl(ctx, mp, seed, sweep_idx, trial0, batch, nullptr, &tr, out, memspace);
}

extern "C" int jstsp_build_trials_from_channel_c32(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx,
                                                   long long trial0, int batch, const jstsp_c32 *Hsrc, int ld_rows, int ld_cols,
                                                   long long strideH, int normalize, const jstsp_trials *out, double *sigma_max,
                                                   int memspace)
{
    const GivenChannel g{reinterpret_cast<const float2 *>(Hsrc), ld_rows, ld_cols, strideH, normalize, sigma_max};
    return build_trials_impl(ctx, mp, seed, sweep_idx, trial0, batch, &g, nullptr, out, memspace);
}
