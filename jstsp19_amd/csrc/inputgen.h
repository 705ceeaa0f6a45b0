// Philox streams, the per-trial draws and the channel of the device-side trial construction (csrc/inputgen.hip), shared
// with the capacity sweep (csrc/capacity.hip) and the rank sweep (csrc/svdvals.hip) so that all of them see the same channel
// and pilots for the same (seed, sweep, trial).
#pragma once
#include "solver_common.h"
#include "support_key.h"

namespace {

enum { ST_GAIN = 0, ST_UR = 1, ST_UT = 2, ST_NOISE = 3, ST_QAM = 4, ST_OMEGA = 5, ST_PILOT = 6 };

__host__ __device__ inline uint64_t mix_key(uint64_t seed, uint64_t sweep, uint64_t trial)
{
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + sweep * 0xBF58476D1CE4E5B9ull + trial * 0x94D049BB133111EBull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ uint4 philox(uint64_t elem, uint32_t stream, uint64_t key64)
{
    uint32_t c0 = (uint32_t)elem, c1 = (uint32_t)(elem >> 32), c2 = stream, c3 = 0u;
    uint32_t k0 = (uint32_t)key64, k1 = (uint32_t)(key64 >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ float u01(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// two independent N(0,1) from two words (Box-Muller)
__device__ __forceinline__ float2 normal2(uint32_t w0, uint32_t w1)
{
    const float r = sqrtf(-2.0f * logf(u01(w0)));
    float s, c;
    sincospif(2.0f * u01(w1), &s, &c);
    return make_float2(r * c, r * s);
}

struct Model {
    int Nt, Nr, L, Tp, Mr, Mr_e, Gr, Gt, clusters, rays, Np, NtL, G2;
};

// ---- gains / angle draws (wideband_mmwave_channel.m:19-22; only tap 1's angles are used, :24) ----
__global__ void draw_small_kernel(Model m, uint64_t seed, uint64_t sweep, long long trial0, float2 *gains,
                                  float *u_r, float *u_t)
{
    const int t = blockIdx.x;
    const uint64_t key = mix_key(seed, sweep, (uint64_t)(trial0 + t));
    for (int i = threadIdx.x; i < m.L * m.Np; i += blockDim.x) {
        const uint4 w = philox((uint64_t)i, ST_GAIN, key);
        const float2 g = normal2(w.x, w.y);
        gains[(size_t)t * m.L * m.Np + i] = make_float2(g.x * 0.70710678f, g.y * 0.70710678f);     // :19
    }
    for (int i = threadIdx.x; i < m.Np; i += blockDim.x) {
        u_r[(size_t)t * m.Np + i] = u01(philox((uint64_t)i, ST_UR, key).x);                          // :20
        u_t[(size_t)t * m.Np + i] = u01(philox((uint64_t)i, ST_UT, key).x);                          // :22
    }
}

// noise = randn + 1j*randn (plot_errorVSsnr.m:60, unscaled) and the 4-QAM symbol indices (qam4mod.m:8)
// gauss != 0: Gaussian pilot draws randn + 1j*randn into psym instead (wideband_hybBF_comm_system_training.m:20, before its 1/sqrt(2))
// noise == NULL: the pilots only (the noise-free capacity sweep, csrc/capacity.hip); the pilot draws do not depend on it
__global__ __launch_bounds__(256) void draw_noise_qam_kernel(Model m, uint64_t seed, uint64_t sweep, long long trial0,
                                                             float2 *noise, uint8_t *qam, int shared_pilots, int gauss,
                                                             float2 *psym)
{
    const int t = blockIdx.y;
    const uint64_t key = mix_key(seed, sweep, (uint64_t)(trial0 + t));
    const uint64_t qkey = shared_pilots ? mix_key(seed, sweep, ~0ull) : key;     // one pilot set per sweep point
    const long long nn = noise ? (long long)m.Nr * m.Tp : 0, nq = (long long)m.Nt * m.Tp;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nn; i += stride) {
        const uint4 w = philox((uint64_t)i, ST_NOISE, key);
        noise[(size_t)t * nn + i] = normal2(w.x, w.y);
    }
    const float a = 0.70710678f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += stride) {
        if (gauss) {
            const uint4 w = philox((uint64_t)i, ST_PILOT, qkey);
            psym[(size_t)t * nq + i] = normal2(w.x, w.y);
            qam[(size_t)t * nq + i] = 0;
        } else {
            const uint8_t q = (uint8_t)(philox((uint64_t)i, ST_QAM, qkey).x & 3u);
            qam[(size_t)t * nq + i] = q;
            // alphabet order of qam4mod.m:7: (1+j), (-1+j), (1-j), (-1-j), all / sqrt(2)
            psym[(size_t)t * nq + i] = make_float2((q & 1) ? -a : a, (q & 2) ? -a : a);
        }
    }
}

// ---- channel: Hmat[t] = [H_1 ... H_L]  (Nr x Nt*L), H_l = 1/sqrt(Np) sum_p w_p g[l,p] a_r(p) a_t(p)^H
//      with tap 1's steering vectors for every l (:24) and w_p = clusters - cluster(p) (:29)
//      DRIFT: the angle of path p is phi_0[p] + dphi[p] (jstsp_build_trials_tracked_drift_c32), one float64 addition; without it
//      the offsets are not read and phi_0 is used as it is formed - the code of the drawn and the tracked channel, unchanged.
template <bool DRIFT>
__device__ __forceinline__ void channel_body(const Model &m, const float2 *gains, const float *u_r, const float *u_t,
                                             const double *dphi_r, const double *dphi_t, float2 *Hmat)
{
    extern __shared__ float2 sh[];
    float2 *ar = sh, *at = sh + (size_t)m.Nr * m.Np, *cf = at + (size_t)m.Nt * m.Np;
    const int t = blockIdx.y;
    const double beta = 1.0 / (1.0 - exp(-sqrt(2.0) * M_PI / 50.0));
    const double e0 = exp(-sqrt(2.0) / 50.0 * M_PI);
    for (int i = threadIdx.x; i < (m.Nr + m.Nt) * m.Np; i += 256) {
        const bool rx = i < m.Nr * m.Np;
        const int ii = rx ? i : i - m.Nr * m.Np;
        const int dim = rx ? m.Nr : m.Nt;
        const int n = ii % dim, p = ii / dim;
        const double u = rx ? u_r[(size_t)t * m.Np + p] : u_t[(size_t)t * m.Np + p];
        double phi = beta * (e0 - cosh(u));                            // :56-62
        if constexpr (DRIFT) phi = __dadd_rn(phi, (rx ? dphi_r : dphi_t)[(size_t)t * m.Np + p]);
        double s, c;
        sincos(-M_PI * sin(-phi) * (double)n, &s, &c);                 // :42-52
        (rx ? ar : at)[ii] = make_float2((float)c, (float)s);
    }
    const float isq = rsqrtf((float)m.Np);
    for (int i = threadIdx.x; i < m.L * m.Np; i += 256) {
        const int p = i % m.Np;
        const float w = (float)(m.clusters - p / m.rays) * isq;
        const float2 g = gains[(size_t)t * m.L * m.Np + i];
        cf[i] = make_float2(g.x * w, g.y * w);
    }
    __syncthreads();
    const long long n_el = (long long)m.Nr * m.NtL;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n_el; e += (long long)gridDim.x * 256) {
        const int r = (int)(e % m.Nr);
        const int sl = (int)(e / m.Nr);
        const int s = sl % m.Nt, l = sl / m.Nt;
        float hx = 0.f, hy = 0.f;
        for (int p = 0; p < m.Np; ++p) {
            const float2 a = ar[p * m.Nr + r], b = at[p * m.Nt + s], c = cf[l * m.Np + p];
            const float qx = a.x * b.x + a.y * b.y, qy = a.y * b.x - a.x * b.y;     // a * conj(b)
            hx += c.x * qx - c.y * qy;
            hy += c.x * qy + c.y * qx;
        }
        Hmat[(size_t)t * n_el + e] = make_float2(hx, hy);
    }
}

__global__ __launch_bounds__(256) void channel_kernel(Model m, const float2 *gains, const float *u_r,
                                                      const float *u_t, float2 *Hmat)
{
    channel_body<false>(m, gains, u_r, u_t, nullptr, nullptr, Hmat);
}

// the same on drifted angles: dphi_r, dphi_t hold phi_f - phi_0 per (trial, path), Np x batch doubles each
__global__ __launch_bounds__(256) void channel_drift_kernel(Model m, const float2 *gains, const float *u_r, const float *u_t,
                                                            const double *dphi_r, const double *dphi_t, float2 *Hmat)
{
    channel_body<true>(m, gains, u_r, u_t, dphi_r, dphi_t, Hmat);
}

inline int grid_for(long long n, int cap = 4096) { return (int)std::min<long long>((n + 255) / 256, cap); }

// ---- the noise-free receive signal of the sweeps that have no solver on their path (hbf.m:12-18, proposed_hbf.m:15-20, N = 0)
// Entry (r, j) of Y = sum_l H_l Psi_bar_l in fp64 from one trial's H (Nr x Nt*L) and pilot symbols (Nt x Tp, unscaled draws):
// Psi_bar_l(s, j) = toeplitz(s_s)(l, j) = s_s(|j - l|), conjugated below the diagonal; pscale: pilots_kernel's fp32 scaling.
__device__ __forceinline__ double2 received_entry(const Model &m, const float2 *H, const float2 *sym, float pscale, int r, int j)
{
    double yr = 0.0, yi = 0.0;
    for (int l = 0; l < m.L; ++l) {
        const int d = j - l;
        for (int s = 0; s < m.Nt; ++s) {
            const float2 h = H[r + (size_t)m.Nr * (s + m.Nt * l)];
            const float2 v = sym[s * m.Tp + (d < 0 ? -d : d)];
            const double px = (double)(v.x * pscale), py = (double)((d < 0 ? -v.y : v.y) * pscale);   // pilots_kernel's values
            yr += (double)h.x * px - (double)h.y * py;
            yi += (double)h.x * py + (double)h.y * px;
        }
    }
    return make_double2(yr, yi);
}

// The channel and pilot symbols of jstsp_build_trials_c32's trials [trial0, trial0 + batch) of (seed, sweep) in the context's
// arena, which the caller has reserved (operands_bytes) and reset: the same three kernels on the same Philox streams, without
// the noise block.  Hmat: Nr x Nt*L per trial; psym: Nt x Tp per trial, to be scaled by *pscale.
struct Operands { float2 *Hmat, *psym; float pscale; };

inline size_t operands_bytes(const Model &m, size_t b)
{
    const size_t nQ = (size_t)m.Nt * m.Tp;
    return jstsp::rnd256(b * m.L * m.Np * 8) + 2 * jstsp::rnd256(b * m.Np * 4) + jstsp::rnd256(b * nQ) + jstsp::rnd256(b * nQ * 8) +
           jstsp::rnd256(b * m.Nr * m.NtL * 8);
}
inline size_t channel_lds_bytes(const Model &m) { return ((size_t)(m.Nr + m.Nt) * m.Np + (size_t)m.L * m.Np) * sizeof(float2); }

inline int draw_operands(jstsp_ctx *ctx, const Model &m, const jstsp_model *mp, uint64_t seed, uint64_t sweep, long long trial0,
                         int batch, Operands *out)
{
    const size_t b = (size_t)batch, nH = (size_t)m.Nr * m.NtL, nQ = (size_t)m.Nt * m.Tp;
    jstsp::Arena &ar = ctx->arena;
    float2 *gains = ar.get<float2>(b * m.L * m.Np), *psym = ar.get<float2>(b * nQ), *Hmat = ar.get<float2>(b * nH);
    float *u_r = ar.get<float>(b * m.Np), *u_t = ar.get<float>(b * m.Np);
    uint8_t *qam = ar.get<uint8_t>(b * nQ);
    JSTSP_REQUIRE(gains && psym && Hmat && u_r && u_t && qam, JSTSP_E_NOMEM, "trial operands: workspace exhausted");
    hipStream_t st = ctx->stream;
    const int gauss = mp->pilots == JSTSP_PILOTS_GAUSS;
    draw_small_kernel<<<batch, 64, 0, st>>>(m, seed, sweep, trial0, gains, u_r, u_t);
    draw_noise_qam_kernel<<<dim3(grid_for((long long)nQ, 1024), batch), 256, 0, st>>>(
        m, seed, sweep, trial0, nullptr, qam, mp->shared_pilots, gauss, psym);
    channel_kernel<<<dim3(grid_for((long long)nH, 64), batch), 256, channel_lds_bytes(m), st>>>(m, gains, u_r, u_t, Hmat);
    JSTSP_HIP(hipGetLastError());
    *out = Operands{Hmat, psym, gauss ? 0.70710678f : 1.f};
    return 0;
}

}  // namespace

namespace jstsp {

// a supplied channel: the arguments of jstsp_build_trials_from_channel_c32 that describe it
struct GivenChannel {
    const float2 *H;
    int ld_rows, ld_cols;
    long long stride;
    int normalize;
    double *sigma_max;
};

// a tracked channel: the arguments of jstsp_build_trials_tracked_c32 that place a frame in its sequence, and those of
// jstsp_build_trials_tracked_drift_c32 that make its angles walk (drifting == 0: the geometry is fixed and the rest is not read)
struct TrackedChannel {
    int frame;
    double corr;
    int drifting;
    double drift;
    double *dphi_r, *dphi_t;
};

// The cut and scale of a supplied channel for trials [trial0, trial0 + batch) (csrc/inputgen.hip), ONE implementation for the trial
// builder and the spectrum sweep: checks the form of g (the error codes of jstsp_build_trials_from_channel_c32), reserves the
// context's arena for caller_bytes plus its own arrays and resets it, computes norm(H_l) per tap, returns JSTSP_E_ILLCOND before
// anything is written when a used block holds a NaN or Inf (or is zero where 1/s is needed), copies s to g.sigma_max, and writes
// Hmat[t] = [H_1 .. H_L] (Nr x Nt*L, the layout of channel_kernel) to Hmat_user (device) or, when that is NULL, to an array of
// the arena.  *Hmat_out: where it is.  Waits for the stream once.
int given_channel_hmat(jstsp_ctx *ctx, int Nr, int Nt, int L, long long trial0, int batch, const GivenChannel &g, int memspace,
                       size_t caller_bytes, float2 *Hmat_user, float2 **Hmat_out);

}  // namespace jstsp
