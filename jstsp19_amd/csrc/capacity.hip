// Achievable spectral efficiency of the combiners (plot_capacity.m, plot_ee.m):
//
//   createBeamformer.m:5-32          -> bf_kernel: 'ZC', 'fft'/'ps', 'quantized', 'quantized_4' from integer phase indices
//   plot_capacity.m:47,52,57,64      -> ASE = real(log2(det(eye(Mr) + c W_c' (Y Y') W_c))),  c = 1/(sigma^2 Nt)
//   plot_capacity.m:36-64            -> ase_sweep_kernel: the channel and pilots of jstsp_build_trials_c32's trial t,
//                                       Y = sum_l H_l Psi_bar_l (hbf.m:12-18, noise-free), every requested design on that Y
//
// The ASE of one trial: P = W_c^H Y (Mr x T) is accumulated in fp64 from the operands; by Sylvester
// det(I_Mr + c P P^H) = det(I_T + c P^H P), so the Gram is formed on the smaller side, n = min(Mr, T) <= 64, as a sum of
// rank-one terms q q^H over the other side (chunks of q in LDS).  G = I + c sum q q^H is Hermitian with every eigenvalue >= 1,
// so its square-root-free Cholesky factorisation G = L D L^H in fp64 needs no pivoting and every pivot is >= 1 in exact
// arithmetic; ASE = sum_k log2 d_k (= 2 sum_k log2 of the Cholesky diagonal).  Non-finite input gives NaN for that trial.
#include "inputgen.h"

using namespace jstsp;

namespace {

constexpr int ASE_NMAX = 64;        // order of the Gram: min(Mr, T)
constexpr int ASE_PC = 2048;        // complex doubles of LDS for one chunk of q vectors
constexpr int ASE_MAX_DESIGNS = 8;
enum { ST_COLS = 7 };               // Philox stream of the column subsets (streams 0..6: csrc/inputgen.h)

// W(n, k) = N^-1/2 exp(-j 2 pi r / D): the phase index r of entry (n, k) of createBeamformer(N, kind), reduced in integers
struct Codebook {
    int kind, N, D, K;
    __host__ __device__ static Codebook make(int kind, int N)
    {
        Codebook b{kind, N, N, 1};
        if (kind == JSTSP_BF_ZC) b.D = 2 * N;                             // exp(-j 11 pi n (k+1) / N)            :15-16
        if (kind == JSTSP_BF_QUANTIZED || kind == JSTSP_BF_QUANTIZED4) {  // A = vec(kron(ones(K,1), 0:2^Nq-1)).' :18-31
            b.D = kind == JSTSP_BF_QUANTIZED ? 64 : 16;
            b.K = (N + b.D - 1) / b.D;                                    // each phase index repeats K times in a row
        }
        return b;
    }
    __device__ int phase(int n, int k) const
    {
        long long r;
        if (kind == JSTSP_BF_ZC) r = 11ll * n * (k + 1);
        else if (kind == JSTSP_BF_DFT) r = (long long)n * k;                // fft(eye(N)) :5 = 'ps' :12-13
        else r = (long long)n * (k / K);
        return (int)(r % D);
    }
};

__device__ __forceinline__ float2 bf_value_f32(int r, int D, int N)
{
    float s, c;
    sincospif(-2.0f * (float)r / (float)D, &s, &c);
    const float sc = rsqrtf((float)N);
    return make_float2(c * sc, s * sc);
}
__device__ __forceinline__ double2 bf_value_f64(int r, int D, int N)
{
    double s, c;
    sincospi(-2.0 * (double)r / (double)D, &s, &c);
    const double sc = 1.0 / sqrt((double)N);
    return make_double2(c * sc, s * sc);
}

template <class T> __global__ void bf_kernel(Codebook b, T *W)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)b.N * b.N) return;
    const int n = (int)(i % b.N), k = (int)(i / b.N);
    const int r = b.phase(n, k);
    if constexpr (sizeof(T) == 8) W[i] = bf_value_f32(r, b.D, b.N);
    else W[i] = bf_value_f64(r, b.D, b.N);
}

__device__ __forceinline__ double2 ld2(const float2 &v) { return make_double2(v.x, v.y); }
__device__ __forceinline__ double2 ld2(const double2 &v) { return v; }

// ASE of one trial on the whole workgroup (every thread calls it; the result is valid in thread 0).
//   Y: Nr x T (column-major, LDS or global); w.column(c): the entries of codebook column c (0-based) in row order (next());
//   col(i): column of slot i < Mr.
//   G: n*n complex doubles of LDS, Pc: n*min(K, ASE_PC/n) complex doubles of LDS (ase_lds_bytes).
template <class TY, class WF, class CF>
__device__ double ase_block(const TY *Y, int Nr, int T, int Mr, const WF &w, const CF &col, double scale, double2 *G,
                            double2 *Pc)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = min(Mr, T);
    const bool wide = Mr >= T;                   // n = T: q_i = conj(P(i, :))^T over the Mr slots; else q_j = P(:, j) over T
    const int K = wide ? Mr : T;
    const int kc = max(1, ASE_PC / n);
    for (int e = tid; e < n * n; e += nt) G[e] = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = min(kc, K - k0);
        __syncthreads();
        for (int e = tid; e < n * kn; e += nt) {
            const int a = e % n, kk = e / n;
            const int i = wide ? k0 + kk : a, j = wide ? a : k0 + kk;
            const int c = col(i);
            double sr = 0.0, si = 0.0;                                 // P(i, j) = sum_r conj(W(r, c)) Y(r, j)
            auto wc = w.column(c);
            for (int r = 0; r < Nr; ++r) {
                const double2 wv = wc.next(), y = ld2(Y[r + (size_t)Nr * j]);
                sr += wv.x * y.x + wv.y * y.y;
                si += wv.x * y.y - wv.y * y.x;
            }
            Pc[a + n * kk] = make_double2(sr, wide ? -si : si);
        }
        __syncthreads();
        for (int e = tid; e < n * n; e += nt) {                          // lower triangle: G(a, b) += sum_k q_k(a) conj(q_k(b))
            const int a = e % n, b = e / n;
            if (a < b) continue;
            double gr = 0.0, gi = 0.0;
            for (int kk = 0; kk < kn; ++kk) {
                const double2 x = Pc[a + n * kk], z = Pc[b + n * kk];
                gr += x.x * z.x + x.y * z.y;
                gi += x.y * z.x - x.x * z.y;
            }
            G[e].x += gr;
            G[e].y += gi;
        }
    }
    int bad = 0;
    for (int e = tid; e < n * n; e += nt) {                              // same owner thread per entry as above
        const int a = e % n, b = e / n;
        if (a >= b) {
            G[e] = make_double2((a == b ? 1.0 : 0.0) + scale * G[e].x, scale * G[e].y);
            bad |= !isfinite(G[e].x) || !isfinite(G[e].y);
        }
    }
    if (__syncthreads_or(bad)) return __builtin_nan("");                // non-finite input (an Inf alone could give log2 = Inf)
    // G = L D L^H, right-looking on the lower triangle; d_k = G(k, k) after step k-1
    double acc = 0.0;
    for (int k = 0; k < n; ++k) {
        const double d = G[k + n * k].x, id = 1.0 / d;
        if (tid == 0) acc += log2(d);
        const int m = n - k - 1;
        for (int e = tid; e < m * m; e += nt) {
            const int i = k + 1 + e % m, j = k + 1 + e / m;
            if (i < j) continue;
            const double2 x = G[i + n * k], z = G[j + n * k];
            G[i + n * j].x -= (x.x * z.x + x.y * z.y) * id;
            G[i + n * j].y -= (x.y * z.x - x.x * z.y) * id;
        }
        __syncthreads();
    }
    return acc;
}

template <class TW> struct WGlobal {
    const TW *W;
    int Nr;
    struct Col {
        const TW *p;
        __device__ double2 next() { return ld2(*p++); }
    };
    __device__ Col column(int c) const { return Col{W + (size_t)Nr * c}; }
};
// Codebook entries from their phase index: the D distinct values are a table in LDS.  Along a column the phase index is
// n * s_k mod D (s_k = phase(1, k) < D), so it is stepped by s_k with one conditional subtraction: the same index as
// Codebook::phase(n, k), without a modulo per entry.
struct WTable {
    const float2 *tab;
    Codebook b;
    struct Col {
        const float2 *tab;
        int r, step, D;
        __device__ double2 next()
        {
            const double2 v = ld2(tab[r]);
            r += step;
            if (r >= D) r -= D;
            return v;
        }
    };
    __device__ Col column(int c) const { return Col{tab, 0, b.phase(1, c), b.D}; }
};
struct ColsGlobal {              // 1-based caller indices (validated before), or NULL = 1..Mr
    const int32_t *c;
    __device__ int operator()(int i) const { return c ? c[i] - 1 : i; }
};
struct ColsLds {
    const int *c;
    __device__ int operator()(int i) const { return c ? c[i] : i; }
};

inline size_t ase_lds_bytes(int Mr, int T)
{
    const int n = std::min(Mr, T), K = std::max(Mr, T);
    const int kc = std::max(1, ASE_PC / n);
    return ((size_t)n * n + (size_t)n * std::min(K, kc)) * sizeof(double2);
}

template <class T>
__global__ __launch_bounds__(256) void ase_kernel(int Nr, int T_, int Ncols, int Mr, const T *Y, const T *W, const int32_t *cols,
                                                  double scale, double *ase)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x;
    const int32_t *ct = cols ? cols + (size_t)Mr * t : nullptr;
    int bad = 0;
    if (ct)
        for (int i = threadIdx.x; i < Mr; i += blockDim.x) bad |= ct[i] < 1 || ct[i] > Ncols;
    if (__syncthreads_or(bad)) {                                                  // a bad column index: NaN, nothing read
        if (threadIdx.x == 0) ase[t] = __builtin_nan("");
        return;
    }
    const int n = min(Mr, T_);
    const double r = ase_block(Y + (size_t)Nr * T_ * t, Nr, T_, Mr, WGlobal<T>{W, Nr}, ColsGlobal{ct}, scale, lds,
                               lds + (size_t)n * n);
    if (threadIdx.x == 0) ase[t] = r;
}

struct Design { int kind, n_cols, pool, col_off; };
struct Designs { Design d[ASE_MAX_DESIGNS]; int n; };

// One workgroup per trial: Y = [H_1 .. H_L] Psi (hbf.m:12-18 with N = 0) in LDS, then each design's ASE on it.
// LDS: Y (Nr x T complex double), the codebook table (max(2 Nr, 64) float2), subset keys and indices (2 x r4 ints), G and Pc.
__global__ __launch_bounds__(256) void ase_sweep_kernel(Model m, Designs ds, uint64_t seed, uint64_t sweep, long long trial0,
                                                        const float2 *Hmat, const float2 *psym, float pscale, double scale,
                                                        int n_sel, double *ase, int32_t *cols)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int r4 = (m.Nr + 3) & ~3;
    double2 *Y = lds;
    float2 *tab = reinterpret_cast<float2 *>(Y + (size_t)m.Nr * m.Tp);
    uint32_t *keys = reinterpret_cast<uint32_t *>(tab + max(2 * m.Nr, 64));
    int *sel = reinterpret_cast<int *>(keys + r4);
    double2 *G = reinterpret_cast<double2 *>(sel + r4);
    const float2 *H = Hmat + (size_t)t * m.Nr * m.NtL;
    const float2 *sym = psym + (size_t)t * m.Nt * m.Tp;
    for (int e = tid; e < m.Nr * m.Tp; e += blockDim.x) Y[e] = received_entry(m, H, sym, pscale, e % m.Nr, e / m.Nr);
    const uint64_t key = mix_key(seed, sweep, (uint64_t)(trial0 + t));
    for (int di = 0; di < ds.n; ++di) {
        const Design dz = ds.d[di];
        const Codebook b = Codebook::make(dz.kind, m.Nr);
        __syncthreads();                                                           // the previous design is done with tab / sel
        for (int r = tid; r < b.D; r += blockDim.x) tab[r] = bf_value_f32(r, b.D, b.N);
        if (dz.pool > 0) {          // ind = randperm(pool); ind(1:n_cols) (plot_capacity.m:63-64): the n_cols smallest of pool keys
            for (int i = tid; i < dz.pool; i += blockDim.x)
                keys[i] = philox(((uint64_t)di << 32) | (uint64_t)i, ST_COLS, key).x;
            __syncthreads();
            for (int i = tid; i < dz.pool; i += blockDim.x) {
                const uint32_t ki = keys[i];
                int rank = 0;
                for (int k = 0; k < dz.pool; ++k) rank += (keys[k] < ki) || (keys[k] == ki && k < i);
                if (rank < dz.n_cols) {
                    sel[rank] = i;
                    if (cols) cols[(size_t)n_sel * t + dz.col_off + rank] = i + 1;
                }
            }
        }
        const int n = min(dz.n_cols, m.Tp);
        const double r = ase_block(Y, m.Nr, m.Tp, dz.n_cols, WTable{tab, b}, ColsLds{dz.pool > 0 ? sel : nullptr}, scale, G,
                                   G + (size_t)n * n);
        if (tid == 0) ase[(size_t)ds.n * t + di] = r;
    }
}

bool bf_kind_ok(int k)
{
    return k == JSTSP_BF_ZC || k == JSTSP_BF_DFT || k == JSTSP_BF_QUANTIZED || k == JSTSP_BF_QUANTIZED4;
}

template <class T> int beamformer_impl(jstsp_ctx *ctx, int N, int kind, T *W, int memspace, const char *what)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: NULL context", what);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace", what);
    JSTSP_REQUIRE(W, JSTSP_E_NULL, "%s: NULL argument", what);
    JSTSP_REQUIRE(N > 0 && N <= 46340, JSTSP_E_SHAPE, "%s: need 1 <= N <= 46340", what);
    JSTSP_REQUIRE(bf_kind_ok(kind), JSTSP_E_ARG, "%s: bad beamformer kind %d", what, kind);
    JSTSP_ENTER(ctx);
    const size_t n = (size_t)N * N;
    T *d = W;
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(ctx->arena.reserve(rnd256(n * sizeof(T)) + 4096));
        ctx->arena.reset();
        d = ctx->arena.get<T>(n);
        JSTSP_REQUIRE(d, JSTSP_E_NOMEM, "%s: workspace exhausted", what);
    }
    bf_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(Codebook::make(kind, N), d);
    JSTSP_HIP(hipGetLastError());
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, W, d, n, memspace));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

template <class T>
int ase_impl(jstsp_ctx *ctx, int Nr, int T_, int Ncols, int Mr, int batch, const T *Y, const T *W, const int32_t *cols,
             double scale, double *ase, int memspace, const char *what)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: NULL context", what);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace", what);
    JSTSP_REQUIRE(Y && W && ase, JSTSP_E_NULL, "%s: NULL argument", what);
    JSTSP_REQUIRE(Nr > 0 && T_ > 0 && Ncols > 0 && Mr > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", what);
    JSTSP_REQUIRE(cols || Mr <= Ncols, JSTSP_E_SHAPE, "%s: Mr > Ncols without a column list", what);
    JSTSP_REQUIRE(std::min(Mr, T_) <= ASE_NMAX, JSTSP_E_UNSUPPORTED, "%s: min(Mr, T) = %d > %d", what, std::min(Mr, T_),
                  ASE_NMAX);
    JSTSP_ENTER(ctx);
    const size_t nY = (size_t)Nr * T_ * batch, nW = (size_t)Nr * Ncols, nC = cols ? (size_t)Mr * batch : 0;
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(ctx->arena.reserve(rnd256(nY * sizeof(T)) + rnd256(nW * sizeof(T)) + rnd256(nC * 4 + 4) +
                                     rnd256((size_t)batch * 8) + 4096));
        ctx->arena.reset();
    }
    const T *y, *w;
    const int32_t *c = nullptr;
    JSTSP_TRY(stage_in(ctx, Y, nY, memspace, &y));
    JSTSP_TRY(stage_in(ctx, W, nW, memspace, &w));
    if (cols) JSTSP_TRY(stage_in(ctx, cols, nC, memspace, &c));
    double *o = memspace == JSTSP_DEVICE ? ase : ctx->arena.get<double>(batch);
    JSTSP_REQUIRE(o, JSTSP_E_NOMEM, "%s: workspace exhausted", what);
    const size_t sh = ase_lds_bytes(Mr, T_);
    JSTSP_HIP(hipFuncSetAttribute((const void *)ase_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    ase_kernel<T><<<batch, 256, sh, ctx->stream>>>(Nr, T_, Ncols, Mr, y, w, c, scale, o);
    JSTSP_HIP(hipGetLastError());
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, ase, o, (size_t)batch, memspace));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

}  // namespace

extern "C" {

int jstsp_beamformer_c32(jstsp_ctx *ctx, int N, int kind, jstsp_c32 *W, int memspace)
{
    return beamformer_impl(ctx, N, kind, reinterpret_cast<float2 *>(W), memspace, "beamformer_c32");
}

int jstsp_beamformer_c64(jstsp_ctx *ctx, int N, int kind, jstsp_c64 *W, int memspace)
{
    return beamformer_impl(ctx, N, kind, reinterpret_cast<double2 *>(W), memspace, "beamformer_c64");
}

int jstsp_ase_c32(jstsp_ctx *ctx, int Nr, int T, int Ncols, int Mr, int batch, const jstsp_c32 *Y, const jstsp_c32 *W,
                  const int32_t *cols, double scale, double *ase, int memspace)
{
    return ase_impl(ctx, Nr, T, Ncols, Mr, batch, reinterpret_cast<const float2 *>(Y), reinterpret_cast<const float2 *>(W),
                    cols, scale, ase, memspace, "ase_c32");
}

int jstsp_ase_c64(jstsp_ctx *ctx, int Nr, int T, int Ncols, int Mr, int batch, const jstsp_c64 *Y, const jstsp_c64 *W,
                  const int32_t *cols, double scale, double *ase, int memspace)
{
    return ase_impl(ctx, Nr, T, Ncols, Mr, batch, reinterpret_cast<const double2 *>(Y), reinterpret_cast<const double2 *>(W),
                    cols, scale, ase, memspace, "ase_c64");
}

int jstsp_ase_trials_c32(jstsp_ctx *ctx, const jstsp_model *mp, const jstsp_ase_design *designs, int n_designs, uint64_t seed,
                         int sweep_idx, long long trial0, int batch, double *ase, int32_t *cols, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ase_trials: NULL context");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "ase_trials: bad memspace");
    JSTSP_REQUIRE(mp && designs && ase, JSTSP_E_NULL, "ase_trials: NULL argument");
    JSTSP_ENTER(ctx);
    Model m;
    m.Nt = mp->Nt; m.Nr = mp->Nr; m.L = mp->L; m.Tp = mp->T_prop; m.Mr = mp->Mr; m.Mr_e = mp->Mr_e;
    m.Gr = mp->Gr; m.Gt = mp->Gt; m.clusters = mp->clusters; m.rays = mp->rays;
    JSTSP_REQUIRE(m.Nt > 0 && m.Nr > 0 && m.L > 0 && m.Tp > 0 && m.clusters > 0 && m.rays > 0 && batch > 0 && trial0 >= 0 &&
                      sweep_idx >= 0,
                  JSTSP_E_SHAPE, "ase_trials: bad model dimensions");
    JSTSP_REQUIRE(m.L <= m.Tp, JSTSP_E_SHAPE, "ase_trials: L > T_prop");
    JSTSP_REQUIRE(mp->noise_var > 0.0, JSTSP_E_ARG, "ase_trials: the noise variance must be positive");
    JSTSP_REQUIRE(mp->pilots == JSTSP_PILOTS_QAM4 || mp->pilots == JSTSP_PILOTS_GAUSS, JSTSP_E_ARG, "ase_trials: bad pilots kind");
    JSTSP_REQUIRE(n_designs >= 1 && n_designs <= ASE_MAX_DESIGNS, JSTSP_E_ARG, "ase_trials: need 1 <= n_designs <= %d",
                  ASE_MAX_DESIGNS);
    m.Np = m.clusters * m.rays; m.NtL = m.Nt * m.L; m.G2 = m.L * m.Gt;
    Designs ds{};
    ds.n = n_designs;
    int n_sel = 0;
    size_t lds_g = 0;
    for (int i = 0; i < n_designs; ++i) {
        const jstsp_ase_design &d = designs[i];
        JSTSP_REQUIRE(bf_kind_ok(d.kind), JSTSP_E_ARG, "ase_trials: design %d: bad beamformer kind %d", i, d.kind);
        JSTSP_REQUIRE(d.n_cols >= 1 && d.pool >= 0 && (d.pool == 0 ? d.n_cols <= m.Nr : d.n_cols <= d.pool && d.pool <= m.Nr),
                      JSTSP_E_SHAPE, "ase_trials: design %d: need 1 <= n_cols <= (pool ? pool : Nr) and pool <= Nr", i);
        JSTSP_REQUIRE(std::min(d.n_cols, m.Tp) <= ASE_NMAX, JSTSP_E_UNSUPPORTED, "ase_trials: design %d: min(n_cols, T) > %d", i,
                      ASE_NMAX);
        ds.d[i] = Design{d.kind, d.n_cols, d.pool, n_sel};
        if (d.pool > 0) n_sel += d.n_cols;
        lds_g = std::max(lds_g, ase_lds_bytes(d.n_cols, m.Tp));
    }
    const size_t r4 = (size_t)((m.Nr + 3) & ~3);
    const size_t lds_ch = channel_lds_bytes(m);
    const size_t lds = (size_t)m.Nr * m.Tp * sizeof(double2) + (size_t)std::max(2 * m.Nr, 64) * sizeof(float2) + 2 * r4 * 4 + lds_g;
    JSTSP_REQUIRE(lds_ch <= 150 * 1024 && lds <= 150 * 1024, JSTSP_E_UNSUPPORTED, "ase_trials: Nr x T_prop too large for the LDS");

    const size_t b = (size_t)batch;
    JSTSP_TRY(ctx->arena.reserve(operands_bytes(m, b) + rnd256(b * n_designs * 8) + rnd256(b * (n_sel + 1) * 4) + 4096));
    ctx->arena.reset();
    Arena &ar = ctx->arena;
    // the draws and the channel of jstsp_build_trials_c32 (csrc/inputgen.hip) for the same (seed, sweep_idx, trial); Y is
    // noise-free (the drivers pass N = zeros), so the noise block is not drawn
    Operands op;
    JSTSP_TRY(draw_operands(ctx, m, mp, seed, (uint64_t)sweep_idx, trial0, batch, &op));
    double *o = memspace == JSTSP_DEVICE ? ase : ar.get<double>(b * n_designs);
    int32_t *c = cols && n_sel ? (memspace == JSTSP_DEVICE ? cols : ar.get<int32_t>(b * n_sel)) : nullptr;
    JSTSP_REQUIRE(o && (c || !(cols && n_sel)), JSTSP_E_NOMEM, "ase_trials: workspace exhausted");
    hipStream_t st = ctx->stream;
    JSTSP_HIP(hipFuncSetAttribute((const void *)ase_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    ase_sweep_kernel<<<batch, 256, lds, st>>>(m, ds, seed, (uint64_t)sweep_idx, trial0, op.Hmat, op.psym, op.pscale,
                                              1.0 / (mp->noise_var * m.Nt), n_sel, o, c);
    JSTSP_HIP(hipGetLastError());
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, ase, o, b * n_designs, memspace));
        if (c) JSTSP_TRY(stage_out(ctx, cols, c, b * n_sel, memspace));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

}  // extern "C"
