// jstsp_proposed_algorithm_c32 — the batched ADMM of
//   basic_system_functions/proposed_algorithm.m:1-73          (indx_S == NULL)
//   basic_system_functions/proposed_algorithm_angles.m:1-85   (indx_S != NULL)
// in structured form: the dense Kronecker operators K1, K2, R, K3 of the
// reference (:14-25, angles :37-43) are never formed —
//   K2*s = vec(A S B),  K2'*k = vec(A^H K B^H),  R*v = vec((A^H A) V (B B^H)),
//   iK1*b = b ./ (Omega + 2 rho),  K3*s = Omega_S .* S.
// All problems of the batch advance together; every step below is one kernel launch over
// the whole batch on the context's stream.
#include "solver_common.h"
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <climits>

namespace jstsp {

// The arrays of one solve (proposed_alloc), the staged inputs and what the set-up stages leave for the loop.
struct ProposedWS {
    // state, N x M per problem
    float2 *X, *V1, *V2, *C, *Xs, *Y, *ZK, *Zb, *Zb2;
    float *invD;
    // Gr x G2 per problem
    float2 *V, *RV, *Res, *RRes, *S, *P1;
    // N x G2 per problem
    float2 *Tc, *W;
    float2 *GA, *GB;
    TrialParams *prm; int32_t *rank; double *ce;
    float *lam;            // 3 * batch
    GramWS gz, gn;         // SVT of Z; spectral norms of V1, V2, X
    // split-f16 path (hgemm.hip): B packed once per solve in both orientations, per-problem operand maxima
    HPack Bc, Bs;          // b(k = m, j = g) = conj(B) for K B^H ;  b(k = g, j = m) = B for (A S) B
    uint32_t *kmax = nullptr, *wmax = nullptr, *pmax = nullptr;
    uint32_t *nmax = nullptr, *zmax = nullptr;   // [X | V1 | V2] (3*batch, contiguous after kmax) and Znext maxima
    HPack GBp;             // b(k, j) = G_B[k + G2 j]: the two (G_A V) G_B applies of the gradient step on the same path
    HPack Wp;              // the synthesis' a operand A S, re-packed every iteration (64 j-tiles would each split it)
    HPack Kp;              // K of K B^H in fragment order (one dictionary for the batch: hgemm_pair_kernel reads it for two trials at a time)
    // the inputs on the device (stage_inputs); subY1 = subY + rho D of a resumed call's first iteration, sin its state (resume.hip)
    const float2 *subY = nullptr, *A = nullptr, *B = nullptr, *sin = nullptr, *subY1 = nullptr;
    const float *Omega = nullptr; const int32_t *indx_S = nullptr;
    bool omega_direct = false;      // the fused pass forms 1 / (Omega + 2 rho) itself, as two floats, when it can read Omega with its 16-byte loads
    Mat Am{}, Bm{}, GAm{}, GBm{}, GAl{};
    int known_gt = 0, toep_gt = 0;  // block height of a block-Toeplitz dictionary: found on the host while staging; the one in use
    float2 *GAlo = nullptr;         // low-order part of G_A ('approximate')
    float2 *PA = nullptr, *PB = nullptr;          // 'std': pinv(A), Gr x N per problem;  pinv(B), M x G2 per problem
    float2 *sout = nullptr;         // the state to return, packed
    int32_t *top = nullptr;         // the list of a support policy's last refresh
    bool toep_probed = false;
    FusedWS fw;
    UntilWS un;                     // the stopping rule of jstsp_proposed_until_c32 (until.hip); empty for every other entry
};

// k-split of the fused three-Gram pass (hgram3_kernel: G_x, G_v1 and G_z from one read of X and V1): chunks of at most
// 1024 columns; 0 = that pass is not used for this shape (then every Gram workspace picks its own split)
static int gram3_nsplit(int N, int M, int G2, bool want_ce)
{
    const int chunk = 1024;
    if (!(want_ce && N <= 64 && N <= M && use_hgemm(N, G2, M))) return 0;
    return std::max(1, std::min(32, (M + chunk - 1) / chunk));
}

// Every decision of one solve that follows from the shape, the switches and the arguments alone: filled once by make_plan, which
// makes no HIP call.  The last row depends on what the Gram workspaces chose and is filled by plan_gram_choices right after
// proposed_alloc.  What each path is and what was measured for it: DESIGN.md sections 5 and 5a.
struct AdmmPlan {
    bool approx, angles, want_ce;
    int nA, nB, Imax1, R;                 // dictionaries held, max(Imax, 1), entries of a refreshed order
    size_t ng, szA, szB;                  // N x G2; elements of the caller's A and B
    long long sGA, sGB;                   // between the Grams of two trials, 0 = one for the batch
    int ns3;                              // gram3_nsplit
    bool h2, h2g, pair;                   // split-f16 products with B, with G_B; the pair kernel on K in fragment order
    bool pinvA, pinvB;                    // 'std': the factor fits the in-LDS float64 pinv (otherwise its Gram inverse)
    int fparts;                           // column ranges per problem of the fused pass
    bool want_fused;                      // the fused pass is allowed and takes the shape
    bool host_compact; size_t compact_elems;      // a JSTSP_HOST dictionary uploaded as first block + leading columns (hostpack.hip)
    bool overlap, grad_fused;             // side streams; the fused launches of the gradient step (gradstep.hip)
    int toep_env, fused_kback;            // JSTSP_TOEPLITZ, JSTSP_FUSED_KBACK
    bool until, live;                     // the call returns iters / ce3 (jstsp_proposed_until_c32); some tol is positive: trials can stop early
    bool want_top;                        // a support policy whose call runs a refresh and whose list is wanted
    // -- after proposed_alloc --
    bool fz, explicit_c;                  // Y = Z - Q Z orientation: fused epilogues; the other one carries C as an operand
    bool hmax;                            // the epilogues also deliver max|X|, |V1|, |V2|, |Znext|: split-f16 Grams
    bool zfly;                            // Z = X - V1/rho is never stored: formed by the three-Gram pass and the (I - Q) Z product
    bool fusedp;                          // the fused pass runs, and forms Y = (I - Q) Z itself
    bool rv_fused1, rv_early_ok;          // R v's first factor as one launch; R v recomputed early on s2
};

static AdmmPlan make_plan(const AdmmProblem &p, const Tuning &tn, bool allow_fused)
{
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2;
    AdmmPlan pl{};
    pl.approx = p.type == JSTSP_TYPE_APPROXIMATE; pl.angles = p.indx_S != nullptr; pl.want_ce = p.ce_out != nullptr;
    pl.nA = p.strideA ? p.batch : 1; pl.nB = p.strideB ? p.batch : 1;
    pl.Imax1 = std::max(p.Imax, 1); pl.R = (int)p.R();
    pl.ng = (size_t)N * G2;
    pl.szA = (size_t)p.strideA * (pl.nA - 1) + (size_t)N * Gr; pl.szB = (size_t)p.strideB * (pl.nB - 1) + (size_t)G2 * M;
    pl.sGA = p.strideA ? (long long)Gr * Gr : 0; pl.sGB = p.strideB ? (long long)G2 * G2 : 0;
    pl.ns3 = gram3_nsplit(N, M, G2, pl.want_ce);
    pl.h2 = use_hgemm(N, G2, M); pl.h2g = use_hgemm(Gr, G2, G2);
    pl.pair = pl.h2 && pl.nB == 1 && hgemm_pair_shape(N, G2, p.batch);
    pl.pinvA = !pl.approx && pinv_fits(N, Gr); pl.pinvB = !pl.approx && pinv_fits(G2, M);
    // JSTSP_FUSED_PARTS, or 4 ranges; when M / 32 is not a multiple of 4: 2 ranges, or 1
    const int ftiles = (M % 32 == 0) ? M / 32 : 0;
    pl.fparts = tn.fused_parts > 0 ? tn.fused_parts : (ftiles % 4 == 0 ? 4 : (ftiles % 2 == 0 ? 2 : 1));
    pl.want_fused = allow_fused && tn.fused != 0 && pl.approx && p.Imax > 1 && fused_shape_ok(N, M, G2, pl.fparts);
    // a JSTSP_HOST dictionary of some size, one per trial, contiguous: tested for the block-Toeplitz structure on the host while
    // it is staged (JSTSP_HOST_COMPACT=2: at any size - the tests)
    pl.host_compact = p.memspace == JSTSP_HOST && tn.host_compact != 0 && tn.toeplitz != 0 && pl.nB > 1 && G2 >= 32 &&
                      p.strideB == (long long)G2 * M && (pl.szB * sizeof(float2) >= ((size_t)64 << 20) || tn.host_compact >= 2) &&
                      (long long)G2 * M < (1ll << 31);
    pl.compact_elems = pl.host_compact ? host_toeplitz_compact_elems(G2, M, pl.nB) : 0;
    // JSTSP_OVERLAP; by default the side streams are on where the work between two passes is three short independent chains
    pl.overlap = tn.overlap >= 0 ? tn.overlap != 0 : pl.want_fused;
    pl.grad_fused = tn.grad_fused != 0; pl.toep_env = tn.toeplitz; pl.fused_kback = tn.fused_kback;
    pl.until = p.until(); pl.live = p.live();
    pl.want_top = p.policy && p.indx_out && p.runs_refresh();
    return pl;
}

static void plan_gram_choices(AdmmPlan &pl, const AdmmProblem &p, const ProposedWS &w)
{
    pl.fz = w.gz.left; pl.explicit_c = !w.gz.left;
    pl.hmax = pl.h2 && pl.fz && p.N <= 64;
    // (only with convergence_error, where the Gram pass over X and V1 exists anyway and delivers G_z with it)
    pl.zfly = pl.hmax && pl.want_ce && pl.ns3 > 0 && w.gz.nsplit == w.gn.nsplit;
    // with convergence_error G_z comes from the three-Gram pass over X, V1 (zfly); without: from the Z the pass stores
    pl.fusedp = pl.want_fused && pl.hmax && (pl.want_ce ? pl.zfly : true);
    pl.rv_fused1 = pl.fusedp && pl.grad_fused && grad_fused_shape(p.N, p.Gr, p.G2);
    // (the two-output call - no split window, no work on s2 - recomputes inline: not measured there)
    pl.rv_early_ok = pl.rv_fused1 && pl.zfly && pl.h2g && pl.overlap;
}

// The arrays every solve takes whatever its data: the state, the Gram workspaces, the operand maxima and the per-iteration packs.
static int proposed_alloc(Arena &a, ProposedWS &w, const AdmmProblem &p, const AdmmPlan &pl)
{
    const size_t nm = p.nm(), g = p.g(), batch = p.batch;
    // X, V1, V2 in one block: the spectral norms of the three are one batched Gram over 3*batch matrices
    w.X = a.get<float2>(3 * batch * nm);
    w.V1 = w.X ? w.X + batch * nm : nullptr;
    w.V2 = w.X ? w.X + 2 * batch * nm : nullptr;
    w.C = a.get<float2>(batch * nm); w.Xs = a.get<float2>(batch * nm); w.Y = a.get<float2>(batch * nm);
    w.ZK = a.get<float2>(batch * nm);
    w.Zb = a.get<float2>(batch * nm);
    w.Zb2 = a.get<float2>(batch * nm);
    w.invD = a.get<float>(batch * nm);
    w.V = a.get<float2>(batch * g); w.RV = a.get<float2>(batch * g); w.Res = a.get<float2>(batch * g);
    w.RRes = a.get<float2>(batch * g); w.S = a.get<float2>(batch * g); w.P1 = a.get<float2>(batch * g);
    w.Tc = a.get<float2>(batch * pl.ng); w.W = a.get<float2>(batch * pl.ng);
    w.GA = a.get<float2>((size_t)pl.nA * p.Gr * p.Gr); w.GB = a.get<float2>((size_t)pl.nB * p.G2 * p.G2);
    w.prm = a.get<TrialParams>(batch);
    w.rank = (pl.angles || p.policy) ? a.get<int32_t>(batch * g) : nullptr;      // of indx_S, then of a policy's refreshes
    w.ce = a.get<double>(batch * 3 * pl.Imax1);
    w.lam = a.get<float>(3 * batch);
    JSTSP_REQUIRE(!a.overrun, JSTSP_E_NOMEM, "proposed_algorithm: workspace exhausted");
    w.GAm = Mat{w.GA, pl.sGA, p.Gr}; w.GBm = Mat{w.GB, pl.sGB, p.G2};
    JSTSP_TRY(w.gz.alloc(a, p.N, p.M, p.batch, true, pl.ns3));
    if (pl.want_ce) JSTSP_TRY(w.gn.alloc(a, p.N, p.M, 3 * p.batch, false, pl.ns3));
    if (pl.h2) {
        // operand maxima of one iteration, one block zeroed once per iteration: kmax | X | V1 | V2 | Znext | wmax | pmax x2.
        // TWO blocks, used by even / odd iterations: with JSTSP_OVERLAP=1 the side-stream Grams of iteration i still
        // read their maxima while the main stream starts iteration i+1, whose memset must not touch those words.
        w.kmax = a.get<uint32_t>(16 * batch);
        w.Wp.KS = 4 * ((p.G2 + 63) / 64); w.Wp.JT = 2 * ((p.N + 63) / 64); w.Wp.count = p.batch;     // (an a pack needs whole 64-row
                                                                                                  //  tiles only, not 128-wide ones)
        w.Wp.st = (long long)w.Wp.JT * w.Wp.KS * 256;
        w.Wp.data = a.get<uint4>(batch * w.Wp.st);
        w.Wp.bmax = w.kmax ? w.kmax + 5 * batch : nullptr;
        if (pl.pair) {
            w.Kp.KS = 4 * ((p.M + 63) / 64); w.Kp.JT = 2; w.Kp.count = p.batch;
            w.Kp.st = (long long)w.Kp.JT * w.Kp.KS * 256;
            w.Kp.data = a.get<uint4>(batch * w.Kp.st);
        }
    } else if (pl.h2g)
        w.pmax = a.get<uint32_t>(2 * batch);
    if (pl.until) {
        // the rule's per-trial words; under a live rule also where a stopped trial is captured: the caller's arrays, or - a host
        // call - what finish_solve stages out in place of w.S / w.Y (the state and the order: setup_resumed, setup_scalars), and
        // the list the loop's own refreshes go on writing
        UntilWS &u = w.un;
        u.flag = a.get<int32_t>(batch); u.iters = a.get<int32_t>(batch); u.left = a.get<int32_t>(1);
        u.ce3 = a.get<double>(batch); u.tol = a.get<double>(batch); u.ovf = a.get<uint32_t>(batch);
        if (pl.live) {
            const bool host = p.memspace == JSTSP_HOST;
            u.S = host ? a.get<float2>(batch * g) : as_f2(p.S_out);
            u.Y = !p.Y_out ? nullptr : host ? a.get<float2>(batch * nm) : as_f2(p.Y_out);
            if (pl.want_top) u.top_loop = a.get<int32_t>(batch * pl.R);
        }
    }
    JSTSP_REQUIRE(!a.overrun, JSTSP_E_NOMEM, "proposed_algorithm: workspace exhausted");
    return 0;
}

// The workspace of one call.  proposed_alloc is measured; the takes of the set-up stages depend on a device probe in their middle
// or happen lazily and stay an upper bound, each term under the condition of the take it covers, in the order of the stages.
static size_t proposed_bytes(const AdmmProblem &p, const AdmmPlan &pl)
{
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2, nA = pl.nA, nB = pl.nB;
    const size_t batch = p.batch, nm = p.nm(), ne = p.state_elems();
    const bool host = p.memspace == JSTSP_HOST;
    Arena m = Arena::measuring();
    ProposedWS w;
    (void)proposed_alloc(m, w, p, pl);
    size_t b = m.peak;
    if (host) {         // stage_inputs: the arrays, the compacted dictionary, the list
        b += rnd256(batch * nm * sizeof(float2)) + rnd256(batch * nm * sizeof(float)) + rnd256(pl.szA * sizeof(float2)) +
             rnd256(pl.szB * sizeof(float2)) + rnd256(pl.compact_elems * sizeof(float2));
        if (pl.angles) b += rnd256(batch * p.listed() * sizeof(int32_t));
    }
    if (host && p.policy && p.indx_out) b += rnd256(batch * pl.R * sizeof(int32_t));       // setup_scalars: the staged list of the last refresh
    if (host) b += (p.state_in ? rnd256(batch * ne * sizeof(float2)) : 0) + (p.state_out ? rnd256(batch * ne * sizeof(float2)) : 0);   // setup_resumed
    if (p.state_in) b += rnd256(batch * nm * sizeof(float2));                              //   subY + rho D
    if (pl.approx) b += rnd256((size_t)nA * Gr * Gr * sizeof(float2));                     // setup_grams: low-order part of G_A
    b += 1024;                                                                             //   probe flags of the block-Toeplitz test
    if (pl.h2) b += hgemm_pack_bytes(M, G2, nB);                                           //   Bc
    if (pl.approx) b += 2 * rnd256((size_t)nB * (G2 / 2 + 1) * G2 * sizeof(float2));       //   G_B's first block row (hi, lo)
    if (pl.h2g) b += hgemm_pack_bytes(G2, G2, nB);                                         //   GBp
    if (!pl.approx)     // setup_std_factors: the pinv, or the Gram inverse with its temporaries
        b += (pl.pinvA ? rnd256((size_t)nA * Gr * N * sizeof(float2)) : rnd256((size_t)nA * Gr * Gr * sizeof(float2)) + hinv_bytes(Gr, nA)) +
             (pl.pinvB ? rnd256((size_t)nB * M * G2 * sizeof(float2)) : rnd256((size_t)nB * G2 * G2 * sizeof(float2)) + hinv_bytes(G2, nB));
    if (pl.want_fused) b += fused_bytes(M, G2, nB, p.batch, pl.fparts);                    // setup_fused
    if (pl.h2) b += hgemm_pack_bytes(G2, M, nB);                                           // the loop's first unfused synthesis: Bs
    return b;
}

}  // namespace jstsp

using namespace jstsp;

static bool tune_host_pipeline()
{
    load_tuning();
    return tune().host_pipeline != 0;
}

// ---- the set-up of a solve, stage by stage -------------------------------------------------------------
static int check_arguments(jstsp_ctx *ctx, const AdmmProblem &p)
{
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2;
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(p.subY && p.Omega && p.A && p.B && p.tau_Y && p.tau_S && p.rho && p.S_out, JSTSP_E_NULL,
                  "proposed_algorithm: NULL array argument");
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && p.batch > 0 && p.Imax >= 0, JSTSP_E_SHAPE,
                  "proposed_algorithm: bad shape N=%d M=%d Gr=%d G2=%d batch=%d Imax=%d", N, M, Gr, G2, p.batch, p.Imax);
    JSTSP_REQUIRE(p.memspace == JSTSP_HOST || p.memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", p.memspace);
    JSTSP_REQUIRE(p.type == JSTSP_TYPE_APPROXIMATE || p.type == JSTSP_TYPE_STD, JSTSP_E_ARG, "bad type %d", p.type);
    JSTSP_REQUIRE(std::min(N, M) <= 2048, JSTSP_E_UNSUPPORTED,
                  "proposed_algorithm: min(N, M) = %d > 2048 (order of the SVT's Gram eigenproblem)", std::min(N, M));
    JSTSP_REQUIRE(p.strideA == 0 || p.strideA >= (long long)N * Gr, JSTSP_E_SHAPE, "strideA too small");
    JSTSP_REQUIRE(p.strideB == 0 || p.strideB >= (long long)G2 * M, JSTSP_E_SHAPE, "strideB too small");
    JSTSP_REQUIRE(p.type == JSTSP_TYPE_APPROXIMATE || (N >= Gr && M >= G2), JSTSP_E_UNSUPPORTED,
                  "proposed_algorithm 'std': K2 = kron(B.', A) must have full column rank (N >= Gr, M >= G2); the "
                  "under-determined U\\(L\\k) of the reference returns a basic, not least-squares, solution");
    return 0;
}

// The inputs on the device.  A JSTSP_HOST dictionary that the plan wants compacted is tested for the block-Toeplitz structure on
// the host while it is staged and uploaded as its first block + leading columns (hostpack.hip).
static int stage_inputs(jstsp_ctx *ctx, const AdmmProblem &p, const AdmmPlan &pl, ProposedWS &w)
{
    const size_t bnm = p.batch * p.nm();
    JSTSP_TRY(stage_in(ctx, as_f2(p.subY), bnm, p.memspace, &w.subY));
    JSTSP_TRY(stage_in(ctx, p.Omega, bnm, p.memspace, &w.Omega));
    JSTSP_TRY(stage_in(ctx, as_f2(p.A), pl.szA, p.memspace, &w.A));
    w.known_gt = ctx->dict_block_hint;        // (a caller that expanded a block-Toeplitz dictionary itself: c64.hip)
    ctx->dict_block_hint = 0;
    if (pl.host_compact) {
        float2 *Bd = ctx->arena.get<float2>(pl.szB), *Cd = ctx->arena.get<float2>(pl.compact_elems);
        JSTSP_REQUIRE(Bd && Cd, JSTSP_E_NOMEM, "workspace exhausted while staging an input");
        JSTSP_TRY(host_toeplitz_stage(ctx, as_f2(p.B), p.G2, p.M, pl.nB, Bd, Cd, pl.compact_elems, &w.known_gt));
        if (!w.known_gt) JSTSP_HIP(hipMemcpyAsync(Bd, p.B, pl.szB * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
        w.B = Bd;
    } else
        JSTSP_TRY(stage_in(ctx, as_f2(p.B), pl.szB, p.memspace, &w.B));
    if (pl.angles) JSTSP_TRY(stage_in(ctx, p.indx_S, p.batch * p.listed(), p.memspace, &w.indx_S));
    if (p.memspace == JSTSP_DEVICE)
        JSTSP_REQUIRE(((uintptr_t)w.subY % 16 == 0) && ((uintptr_t)w.Omega % 8 == 0), JSTSP_E_ARG,
                      "device arrays must be 16-byte aligned");
    w.subY1 = w.subY;
    w.omega_direct = ((uintptr_t)w.Omega % 16 == 0) && (p.nm() % 4 == 0);
    w.Am = Mat{w.A, p.strideA, p.N}; w.Bm = Mat{w.B, p.strideB, p.G2};
    return 0;
}

// Per-problem scalars; zero state (:8-12); iK1 (:14-20); the rank of indx_S; `top`, the list of a support policy's last refresh
// (jstsp_proposed_refresh_c32; every other entry passes none - the policy itself: gradient_step).
static int setup_scalars(jstsp_ctx *ctx, const AdmmProblem &p, const AdmmPlan &pl, ProposedWS &w)
{
    const int batch = p.batch;
    const size_t bnm = batch * p.nm() * sizeof(float2), bg = batch * p.g() * sizeof(float2);
    {
        std::vector<TrialParams> hp(batch);
        for (int t = 0; t < batch; ++t) hp[t] = make_trial_params(p.rho[t], p.tau_Y[t], p.tau_S[t]);
        JSTSP_TRY(upload(ctx, w.prm, hp.data(), batch * sizeof(TrialParams)));
    }
    hipStream_t st = ctx->stream;
    for (float2 *z : {w.X, w.V1, w.V2, w.C, w.Xs, w.Y}) JSTSP_HIP(hipMemsetAsync(z, 0, bnm, st));
    JSTSP_HIP(hipMemsetAsync(w.V, 0, bg, st));
    JSTSP_HIP(hipMemsetAsync(w.S, 0, bg, st));
    JSTSP_HIP(hipMemsetAsync(w.ce, 0, (size_t)batch * 3 * pl.Imax1 * sizeof(double), st));   // ce(:,3) stays 0 for 'std' (:6)
    JSTSP_TRY(launch_inv_d(ctx, (long long)p.nm(), batch, w.Omega, 2.f, w.prm, w.invD));
    if (pl.angles) JSTSP_TRY(launch_rank_from_index(ctx, (int)p.g(), batch, w.indx_S, (int)p.listed(), w.rank));
    if (pl.want_top) {
        w.top = p.memspace == JSTSP_DEVICE ? p.indx_out : ctx->arena.get<int32_t>((size_t)batch * pl.R);
        JSTSP_REQUIRE(w.top, JSTSP_E_NOMEM, "proposed_algorithm: workspace exhausted (refreshed order)");
        if (pl.live) { w.un.top = w.top; w.top = w.un.top_loop; }      // a stopped trial's list is captured; the loop writes its own
    }
    if (pl.until) {
        JSTSP_TRY(upload(ctx, w.un.tol, p.tol, batch * sizeof(double)));
        JSTSP_TRY(launch_until_init(ctx, batch, w.un));
    }
    return 0;
}

// A resumed call: the iterate from the caller's state instead of zeros, Xs = A S B from the loaded S.  The loop does not carry
// C (C == -V2): where its first X / K update is an epilogue, w.C holds D = C + V2 and subY1 = subY + rho D (resume.hip)
static int setup_resumed(jstsp_ctx *ctx, const AdmmProblem &p, const AdmmPlan &pl, ProposedWS &w)
{
    const int N = p.N, batch = p.batch;
    const size_t nm = p.nm(), g = p.g(), ne = p.state_elems();
    if (p.state_in) {
        JSTSP_TRY(stage_in(ctx, as_f2(p.state_in), batch * ne, p.memspace, &w.sin));
        float2 *sy1 = pl.explicit_c ? nullptr : ctx->arena.get<float2>(batch * nm);
        JSTSP_REQUIRE(pl.explicit_c || sy1, JSTSP_E_NOMEM, "proposed_algorithm: workspace exhausted (resumed state)");
        JSTSP_TRY(launch_resume_unpack(ctx, (long long)nm, (long long)g, batch, w.sin, w.X, w.V1, w.V2, w.C, w.V, w.S, w.subY, sy1, w.prm, pl.explicit_c));
        if (!pl.explicit_c) w.subY1 = sy1;
        JSTSP_TRY(gemm(ctx, 'N', 'N', N, p.G2, p.Gr, batch, w.Am, Mat{w.S, (long long)g, p.Gr}, w.W, (long long)pl.ng, N));
        JSTSP_TRY(gemm(ctx, 'N', 'N', N, p.M, p.G2, batch, Mat{w.W, (long long)pl.ng, N}, w.Bm, w.Xs, (long long)nm, N, 1.f, nullptr, 0, 0, 0.f, GEMM_SYNTH));
    }
    if (p.state_out) {
        w.sout = p.memspace == JSTSP_DEVICE ? as_f2(p.state_out) : ctx->arena.get<float2>(batch * ne);
        JSTSP_REQUIRE(w.sout, JSTSP_E_NOMEM, "proposed_algorithm: workspace exhausted (resumed state)");
    }
    return 0;
}

// G_A = A^H A (Gr x Gr), G_B = B B^H (G2 x G2):  R = K2'*K2 = G_B^T (x) G_A  (:25), with the block-Toeplitz probe (fused.hip), which
// serves the Gram as well as the pass, and the packs of B and G_B.  The two Grams are OPERATORS of the iteration - an error of a
// Gram is a constant bias of the gradient, not rounding noise - so 'approximate' forms both in float64 from the fp32 inputs: G_A
// kept as TWO floats hi + lo (gram64.hip), G_B rounded once to fp32 (the measurements: DESIGN.md section 5a).
static int setup_grams(jstsp_ctx *ctx, const AdmmProblem &p, const AdmmPlan &pl, ProposedWS &w)
{
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2, nA = pl.nA, nB = pl.nB;
    const long long strideB = p.strideB, sGB = (long long)G2 * G2;
    if (pl.approx) {
        w.GAlo = ctx->arena.get<float2>((size_t)nA * Gr * Gr);
        JSTSP_REQUIRE(w.GAlo, JSTSP_E_NOMEM, "proposed_algorithm: workspace exhausted (Gram refinement)");
        JSTSP_TRY(gram_f64(ctx, 'L', w.A, p.strideA, N, Gr, nA, w.GA, (long long)Gr * Gr, w.GAlo));
        w.GAl = Mat{w.GAlo, pl.sGA, Gr};
    } else
        JSTSP_TRY(gemm(ctx, 'C', 'N', Gr, Gr, N, nA, w.Am, w.Am, w.GA, (long long)Gr * Gr, Gr));
    if (pl.toep_env != 0 && w.known_gt && strideB) {        // found on the host while staging (exact by construction): no device probe
        w.toep_gt = w.known_gt;
        w.toep_probed = true;
    } else if (pl.toep_env != 0 && (long long)G2 * M < (1ll << 31) && pl.approx) {
        JSTSP_TRY(fused_probe_toeplitz(ctx, ctx->arena, w.B, strideB, G2, M, nB, &w.toep_gt));
        w.toep_probed = true;
    }
    // pack the dictionary first: G_B = B B^H is itself "a = B, b = conj(B)^T" on the split-f16 path (the synthesis orientation
    // w.Bs is packed at its first use: with the fused pass the last iteration of a three-output call, never in a two-output call)
    if (pl.h2) JSTSP_TRY(hgemm_pack(ctx, w.Bc, ctx->arena, w.B, strideB, G2, 1, 1, M, G2, nB, (long long)G2 * M));
    if (pl.approx) {
        // JSTSP_TOEPLITZ=1 stays bit-identical to the unstructured path: full product there.  The assembly reads B columns below
        // L = G2 / Gt and above M - L: a constant dictionary with fewer columns than delay blocks passes the probe and takes the full product.
        if (w.toep_gt && pl.toep_env >= 2 && M >= G2 / w.toep_gt) {
            // block (ld, ld') of G_B from block (0, ld' - ld) of the first block row (fused.hip: toeplitz_gram_kernel), all in float64
            const int gt = w.toep_gt;
            float2 *G0 = ctx->arena.get<float2>((size_t)nB * gt * G2), *G0lo = ctx->arena.get<float2>((size_t)nB * gt * G2);
            JSTSP_REQUIRE(G0 && G0lo, JSTSP_E_NOMEM, "workspace exhausted (G_B block row)");
            GemmDesc dg = make_gemm('N', 'C', gt, G2, M, nB, w.Bm, w.Bm, G0, (long long)gt * G2, gt);
            dg.force_m64 = 1; dg.C_lo = G0lo;
            JSTSP_TRY(launch_cgemm(ctx, dg, GEMM_MISC));
            JSTSP_TRY(toeplitz_gram_assemble(ctx, w.B, strideB, G2, M, gt, nB, G0, G0lo, w.GB, nullptr));
            ctx->last_dict_block = gt;        // (the structure has been used, whether or not the fused pass takes this shape)
        } else {
            GemmDesc dg = make_gemm('N', 'C', G2, G2, M, nB, w.Bm, w.Bm, w.GB, sGB, G2);
            dg.force_m64 = 1; dg.herm_upper = 1;
            JSTSP_TRY(launch_cgemm(ctx, dg, GEMM_MISC));
            JSTSP_TRY(hermitian_fill_lower(ctx, w.GB, sGB, G2, nB));
        }
    } else if (pl.h2) {
        // (G_B is Hermitian: the tiles below its diagonal - 12 of 32 at G2 = 512 - are not computed but mirrored)
        HGemmDesc hb{w.B, strideB, G2, w.Bc.bmax, w.Bc.data, w.Bc.st, w.Bc.bmax, 1, w.Bc.KS, w.Bc.JT, w.GB,
                     sGB, G2, G2, G2, M, nB, EPI_NONE, nullptr, nullptr, nullptr};
        hb.herm_upper = 1;
        JSTSP_TRY(launch_hgemm(ctx, hb, nullptr));
        JSTSP_TRY(hermitian_fill_lower(ctx, w.GB, sGB, G2, nB));
    } else
        JSTSP_TRY(gemm(ctx, 'N', 'C', G2, G2, M, nB, w.Bm, w.Bm, w.GB, sGB, G2));
    if (pl.h2g && pl.approx) JSTSP_TRY(hgemm_pack(ctx, w.GBp, ctx->arena, w.GB, pl.sGB, 1, G2, 0, G2, G2, nB, sGB));
    return 0;
}

// 'std': v = U\(L\k) (:29,:53) is the least-squares solution K2^+ k = vec(pinv(A) K pinv(B)) for K2 = kron(B.', A)
// of full column rank.  Factors that fit the in-LDS float64 kernel get a true SVD-based pinv (pinv.hip: every shape
// of the reference's drivers); larger ones the fp32 Gram inverse G^-1 (hinv.hip), kept in GA / GB, with its
// conditioning recorded (JSTSP_E_ILLCOND / jstsp_last_conditioning).
static int setup_std_factors(jstsp_ctx *ctx, const AdmmProblem &p, const AdmmPlan &pl, ProposedWS &w)
{
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2, nA = pl.nA, nB = pl.nB;
    JSTSP_TRY(diag_reset(ctx));
    if (pl.pinvA) {
        w.PA = ctx->arena.get<float2>((size_t)nA * Gr * N);
        JSTSP_REQUIRE(w.PA, JSTSP_E_NOMEM, "proposed_algorithm 'std': workspace exhausted");
        JSTSP_TRY(launch_pinv(ctx, N, Gr, nA, w.A, p.strideA, N, w.PA, (long long)Gr * N, Gr));
    }
    if (pl.pinvB) {
        w.PB = ctx->arena.get<float2>((size_t)nB * M * G2);
        JSTSP_REQUIRE(w.PB, JSTSP_E_NOMEM, "proposed_algorithm 'std': workspace exhausted");
        JSTSP_TRY(launch_pinv(ctx, G2, M, nB, w.B, p.strideB, G2, w.PB, (long long)M * G2, M));
    }
    float2 *GAi = w.PA ? nullptr : ctx->arena.get<float2>((size_t)nA * Gr * Gr);
    float2 *GBi = w.PB ? nullptr : ctx->arena.get<float2>((size_t)nB * G2 * G2);
    JSTSP_REQUIRE((w.PA || GAi) && (w.PB || GBi), JSTSP_E_NOMEM, "proposed_algorithm 'std': workspace exhausted");
    const size_t mark = ctx->arena.off;         // (the temporaries of an inverse are free again once it has been enqueued)
    if (!w.PA) {
        JSTSP_TRY(hermitian_inverse(ctx, Gr, nA, w.GA, GAi));
        ctx->arena.off = mark;
        JSTSP_HIP(hipMemcpyAsync(w.GA, GAi, (size_t)nA * Gr * Gr * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (!w.PB) {
        JSTSP_TRY(hermitian_inverse(ctx, G2, nB, w.GB, GBi));
        ctx->arena.off = mark;
        JSTSP_HIP(hipMemcpyAsync(w.GB, GBi, (size_t)nB * G2 * G2 * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
    }
    return 0;
}

// Iteration 0's SVT preparation on the main stream (X = V1 = 0, or the resumed iterate), then the fused pass's workspace (fused.hip):
// after the gradient step of iteration it, ONE kernel forms Xs = A S B, the V2 / X / V1 / k updates of :61-65 and of the next
// iteration's :38-43, Y = (I - Q) Z, and the first factor K B^H of the next :47 - the dictionary is read once per iteration, and
// the next iteration starts at the gradient step.  A block-Toeplitz dictionary is kept as its first block only: probed exactly.
// JSTSP_TOEPLITZ: 0 - always the full tile image; 1 - the compact HBM image (bit-identical to 0); 2 (default) - block height 64
// also takes the window kernel (fused_pass64_kernel: fp32-equivalent, not bit-identical).
static int setup_fused(jstsp_ctx *ctx, const AdmmProblem &p, const AdmmPlan &pl, ProposedWS &w)
{
    if (p.Imax > 0) {
        JSTSP_TRY(launch_form_z(ctx, (long long)p.nm(), p.batch, w.X, w.V1, w.prm, w.Zb));
        JSTSP_TRY(svt_prepare(ctx, w.gz, w.Zb, w.prm, nullptr, true));
    }
    if (!pl.fusedp) return 0;
    if (pl.toep_env != 0 && !w.toep_probed) JSTSP_TRY(fused_probe_toeplitz(ctx, ctx->arena, w.B, p.strideB, p.G2, p.M, pl.nB, &w.toep_gt));
    ctx->last_dict_block = w.toep_gt;
    JSTSP_TRY(fused_alloc(ctx->arena, w.fw, p.M, p.G2, pl.nB, p.batch, pl.fparts, w.toep_gt, pl.toep_env >= 2 && pl.fusedp));
    JSTSP_TRY(fused_pack_b(ctx, w.fw, w.B, p.strideB, p.G2, p.M, pl.nB, w.Bc.bmax));
    JSTSP_HIP(hipMemsetAsync(w.fw.ovf, 0, (size_t)p.batch * sizeof(uint32_t), ctx->stream));
    return 0;
}

// ---- the iteration: its pieces, its three streams and the events between them --------------------------
// The MFMA-bound critical path [Y = Z - QZ, X/K/V1 update] -> K B^H -> Gram applies -> step -> A S B -> [C/V2 update] stays on the
// context's stream `sm`.  With the plan's `overlap` two chains run beside it (without it s1 = s2 = sm: same kernels, same results):
//   s1: once X, V1 of iteration i exist (ev_x) the NEXT iteration's SVT input Z = X - V1/rho, its Gram and eigen-decomposition;
//   s2: the norms of convergence_error(i,1:2): Gram of [X | V1] (ev_x), Gram of V2 after update_c (ev_c), lambda_max of all three;
//       behind a fused pass also the recomputation of R v (ev_v, ev_rv: gradient_step).
// Buffer hazards are closed by events: update_x(i+1) waits for s1 (ev_svt: needs Q) and for s2's Gram of [X | V1] (ev_gxv: reads
// what update_x overwrites); update_c(i+1) waits for s2's Gram of V2 (ev_gv2).  The operand maxima are double-buffered by
// iteration parity for the same reason.
struct AdmmLoop {
    jstsp_ctx *const ctx; const AdmmProblem &p; const AdmmPlan &pl; ProposedWS &w;      // (the side streams exist: ensure_side_streams)
    const int N = p.N, M = p.M, Gr = p.Gr, G2 = p.G2, batch = p.batch, Imax = p.Imax;
    const long long snm = (long long)p.nm(), sg = (long long)p.g(), sng = (long long)pl.ng;
    hipStream_t sm = ctx->stream, s1 = pl.overlap ? ctx->side[0] : sm, s2 = pl.overlap ? ctx->side[1] : sm;
    hipEvent_t ev_x = ctx->ev[0], ev_svt = ctx->ev[1], ev_gxv = ctx->ev[2], ev_c = ctx->ev[3], ev_gv2 = ctx->ev[4], ev_ce = ctx->ev[5],
               ev_lxv = ctx->ev[6], ev_q1 = ctx->ev[7], ev_v = ctx->ev[8], ev_rv = ctx->ev[9];
    float2 *Zbuf[2] = {w.Zb, w.Zb2};        // svt argument of iteration it lives in Zbuf[it & 1]
    uint32_t *const kmax0 = w.kmax;         // the two blocks of operand maxima
    // carried from one iteration to the next
    bool passed = false;                    // X, V1, k-partials of this iteration came from the previous pass
    bool rv_early = false;                  // R v of this iteration is being recomputed on s2 (issued by the previous iteration)
    bool in_force = pl.angles;              // a rank masks S
    bool listed = false;                    // the call has run a refresh: w.top holds a list
    // of the iteration in progress
    int it = 0, apply_no = 0, cnt = 0;      // cnt: entries of the mask (angles)
    float2 *Zc = nullptr, *Zn = nullptr;
    bool svt_split = false;                 // behind a pass: the side chain in two halves around the gradient step's head
    bool next_zeroed = false;               // step_v has zeroed the next iteration's operand maxima

    bool xs_unused() const { return pl.fusedp && !pl.want_ce && it + 1 == Imax && !w.sout; }
    uint32_t *maxima(int i) const { return kmax0 + (size_t)(i & 1) * 8 * (size_t)batch; }
    uint32_t *pmax_slot() { return w.pmax ? w.pmax + (size_t)(apply_no++ & 1) * batch : nullptr; }     // two applies per iteration, one slot each

    // The iteration's block of operand maxima, zeroed (one memset instead of four; block it & 1: every consumer of the same block from
    // iteration it-2 has been waited for by the main stream during iteration it-1: ev_svt, ev_gxv, ev_gv2), and the waits of sub 1.
    int begin(int it_)
    {
        it = it_;
        if (pl.want_ce) w.gn.lz.call = it;
        Zc = pl.fz ? Zbuf[it & 1] : w.Zb; Zn = pl.fz ? Zbuf[(it + 1) & 1] : w.Zb;
        if (pl.h2) {
            w.kmax = maxima(it); w.nmax = w.kmax + batch; w.zmax = w.kmax + 4 * (size_t)batch;
            w.wmax = w.kmax + 5 * (size_t)batch; w.pmax = w.kmax + 6 * (size_t)batch;
            if (!passed) JSTSP_HIP(hipMemsetAsync(w.kmax, 0, 8 * (size_t)batch * sizeof(uint32_t), sm));
        } else if (pl.h2g) JSTSP_HIP(hipMemsetAsync(w.pmax, 0, 2 * (size_t)batch * sizeof(uint32_t), sm));
        apply_no = 0;
        next_zeroed = false;
        if (it > 0) JSTSP_HIP(hipStreamWaitEvent(sm, ev_svt, 0));
        if (it > 0 && pl.want_ce) JSTSP_HIP(hipStreamWaitEvent(sm, ev_gxv, 0));
        // behind a pass (with convergence_error): the Gram pass starts with the window, the eigen-decomposition behind the
        // gradient step's bandwidth-heavy head (profiles/r03_fused_iteration_timeline.txt); otherwise the whole side chain at once
        svt_split = passed && pl.fusedp && pl.zfly && it + 1 < Imax;
        cnt = (int)std::min<long long>(10 + 5ll * ((long long)p.it0 + it + 1), sg);
        return 0;
    }

    // -- sub 1: Y = svt(X - V1/rho, tau_Y/rho) = Z - Q Z (:35), sub 2 + k of sub 3 + V1 dual update (:38-43,:64); records ev_x
    int update_x()
    {
        const bool first_resumed = w.sin && it == 0;
        if (passed) {
            // all of it was applied by the previous iteration's pass
        } else if (pl.fz) {
            // Y = Z - Q Z as (I - Q) Z (the beta-term form reads the Z tile a second time from HBM: +0.5 GB), with the X / K / V1
            // updates (and the next Z) applied to the tile in registers
            JSTSP_TRY(launch_eye_minus(ctx, N, batch, w.gz.Q, w.gz.Q));
            GemmDesc dq = make_gemm('N', 'N', N, M, N, batch, Mat{w.gz.Q, (long long)N * N, N}, Mat{Zc, snm, N}, w.Y, snm, N);
            dq.epi = EPI_UPDATE_X; dq.prm = w.prm;
            dq.e_rw0 = w.V1; dq.e_w1 = w.X; dq.e_w2 = w.ZK;
            dq.e_r0 = w.V2; dq.e_r2 = w.Xs; dq.e_r3 = first_resumed ? w.subY1 : w.subY; dq.e_f0 = w.invD;
            dq.e_w3 = (it + 1 < Imax && (!pl.zfly || pl.fusedp)) ? Zn : nullptr;      // (the fused pass reads the stored Z)
            if (pl.zfly && it > 0) { dq.B = w.X; dq.B2 = w.V1; }      // Z = X - V1/rho in the panel loader (it == 0: Z = 0 in Zc)
            dq.epi_store_c = (it + 1 == Imax) || pl.live;    // Y itself is only an output of a trial's last iteration
            if (pl.h2) {                                // max|K| for the split-f16 correlation, from the same epilogue
                dq.amax_out = w.kmax;
                if (N <= 64) { dq.amax_x = w.nmax; dq.amax_v1 = w.nmax + batch; dq.amax_z = w.zmax; }
            }
            JSTSP_TRY(launch_cgemm(ctx, dq, GEMM_MISC));
            if (first_resumed) {                        // k = [k with C = -V2] - D, and its maximum again (resume.hip)
                JSTSP_TRY(launch_resume_fix_k(ctx, (long long)batch * snm, w.ZK, w.C));
                if (pl.h2) JSTSP_TRY(hgemm_absmax(ctx, w.ZK, snm, snm, batch, w.kmax));
            }
        } else {
            JSTSP_TRY(svt_apply(ctx, w.gz, Zc, w.Y));
            JSTSP_TRY(launch_update_x(ctx, snm, batch, w.X, w.V1, w.V2, w.C, w.Xs, w.Y, w.subY, w.invD, w.prm, w.ZK));
        }
        JSTSP_HIP(hipEventRecord(ev_x, sm));
        return 0;
    }

    // s1: next iteration's Z, Gram, eigen-decomposition; records ev_svt (and ev_gxv, ev_lxv with the three-Gram pass).
    // stage 0: all of it; 1: up to the Gram pass; 2: from the eigen-decomposition on
    int side_chain(int stage)
    {
        if (stage != 2) JSTSP_HIP(hipStreamWaitEvent(s1, ev_x, 0));
        StreamScope sc(ctx, s1);
        if (stage != 2 && !pl.fz) JSTSP_TRY(launch_form_z(ctx, snm, batch, w.X, w.V1, w.prm, Zn));   // fused: written by the epilogue
        if (pl.zfly) {
            if (stage != 2) {
                // (the spectral norms of X, V1 of the previous iteration read the G_x, G_v1 partials this pass overwrites)
                if (pl.fusedp && it > 0) JSTSP_HIP(hipStreamWaitEvent(s1, ev_lxv, 0));
                // one pass over X and V1: G_x, G_v1 (convergence_error) and G_z of Z = X - V1/rho (next svt)
                JSTSP_TRY(launch_hgram3(ctx, w.X, w.V1, snm, N, M, batch, w.gz.nsplit, w.nmax, w.nmax + batch, w.zmax,
                                        w.prm, w.gz.Gpart, w.gn.Gpart, w.gn.Gpart + (size_t)batch * N * N * w.gn.nsplit));
                JSTSP_HIP(hipEventRecord(ev_gxv, s1));
                if (pl.fusedp) {    // lambda_max of G_x, G_v1 now (beside the pass), not after it with G_v2: the next Gram
                                    // pass then never waits for them
                    JSTSP_HIP(hipStreamWaitEvent(s2, ev_gxv, 0));
                    StreamScope sc2(ctx, s2);
                    JSTSP_TRY(lmax_from_partials_range(ctx, w.gn, 0, 2 * batch, w.lam, true));
                    JSTSP_HIP(hipEventRecord(ev_lxv, s2));
                }
            }
            if (stage == 1) return 0;
            JSTSP_TRY(svt_prepare(ctx, w.gz, w.X, w.prm, nullptr, true, w.zmax, nullptr, true));
        } else
            JSTSP_TRY(svt_prepare(ctx, w.gz, Zn, w.prm, nullptr, true, pl.hmax ? w.zmax : nullptr));
        // the pass at the end of this iteration forms Y = (I - Q) Z itself: fragments of I - Q
        if (pl.fusedp) JSTSP_TRY(fused_pack_wq(ctx, w.fw, w.gz.Q, batch));
        JSTSP_HIP(hipEventRecord(ev_svt, s1));
        return 0;
    }

    // s2: Gram of [X | V1] for the norms, where the three-Gram pass of the side chain does not deliver it; records ev_gxv
    int gram_xv()
    {
        if (!pl.want_ce || (pl.zfly && it + 1 < Imax)) return 0;
        JSTSP_HIP(hipStreamWaitEvent(s2, ev_x, 0));
        StreamScope sc(ctx, s2);
        JSTSP_TRY(gram_partials_range(ctx, w.gn, w.X, snm, 0, 2 * batch, pl.hmax ? w.nmax : nullptr, nullptr, nullptr, true));      // (norms only: high f16 plane)
        JSTSP_HIP(hipEventRecord(ev_gxv, s2));
        return 0;
    }

    // -- first factor of sub 3, res = K2'*k - R*v (:47): Tc = K B^H (N x G2), or K pinv(B) for 'std' with a float64 pinv of B
    int correlate()
    {
        const long long strideB = p.strideB;
        if (passed) return fused_reduce(ctx, w.fw, G2, M, batch, w.Tc);
        if (w.PB)
            return gemm(ctx, 'N', 'N', N, G2, M, batch, Mat{w.ZK, snm, N}, Mat{w.PB, strideB ? (long long)M * G2 : 0, M},
                        w.Tc, sng, N, 1.f, nullptr, 0, 0, 0.f, GEMM_CORRELATE);
        if (!pl.h2)
            return gemm(ctx, 'N', 'C', N, G2, M, batch, Mat{w.ZK, snm, N}, w.Bm, w.Tc, sng, N, 1.f, nullptr, 0, 0, 0.f, GEMM_CORRELATE);
        if (!pl.fz) JSTSP_TRY(hgemm_absmax(ctx, w.ZK, snm, snm, batch, w.kmax));
        HGemmDesc hc{w.ZK, snm, N, w.kmax, w.Bc.data, strideB ? w.Bc.st : 0, w.Bc.bmax, strideB ? 1 : 0, w.Bc.KS,
                     w.Bc.JT, w.Tc, sng, N, N, G2, M, batch, EPI_NONE, nullptr, nullptr, nullptr};
        if (w.Kp.data && !strideB && w.Kp.KS == w.Bc.KS) {
            // one dictionary for the batch: k(n, m) in fragment order once, then two trials per workgroup
            w.Kp.bmax = w.kmax;
            JSTSP_TRY(hgemm_repack(ctx, w.Kp, w.ZK, snm, N, 1, 0, M, N, w.kmax));
            hc.Ap = w.Kp.data; hc.sApt = w.Kp.st; hc.aKS = w.Kp.KS;
        }
        return launch_hgemm(ctx, hc, "correlate");
    }

    // (G_A X) G_B: the G2 x G2 factor is packed once per solve; max|G_A X| comes from the first product's epilogue.
    // exact (R v itself is being formed from v): with the low-order part of G_A, the second factor as the fp32-MFMA product with fp64
    // master accumulators
    int second_factor(float2 *out, uint32_t *pm, bool exact)
    {
        if (exact || !pl.h2g) {
            GemmDesc dr = make_gemm('N', 'N', Gr, G2, G2, batch, Mat{w.P1, sg, Gr}, w.GBm, out, sg, Gr);
            dr.force_m64 = exact ? 1 : 0;
            return launch_cgemm(ctx, dr, GEMM_MISC);
        }
        const long long strideB = p.strideB;
        HGemmDesc hg{w.P1, sg, Gr, pm, w.GBp.data, strideB ? w.GBp.st : 0, w.GBp.bmax, strideB ? 1 : 0,
                     w.GBp.KS, w.GBp.JT, out, sg, Gr, Gr, G2, G2, batch, EPI_NONE, nullptr, nullptr, nullptr};
        return launch_hgemm(ctx, hg, nullptr);
    }
    int apply_R(const float2 *Xin, float2 *out, bool exact)
    {
        uint32_t *pm = pmax_slot();
        if (exact && pl.rv_fused1) {       // P1 = G_A,hi X + (G_A,lo X) in one launch; no maximum (unused by the exact second factor)
            JSTSP_TRY(launch_grad_refresh_p1(ctx, Xin, w.GA, w.GAlo, pl.sGA, w.P1, G2, batch));
            return second_factor(out, pm, exact);
        }
        if (exact) JSTSP_TRY(gemm(ctx, 'N', 'N', Gr, G2, Gr, batch, w.GAl, Mat{Xin, sg, Gr}, w.P1, sg, Gr));      // P1 = G_A,lo X
        GemmDesc dp = make_gemm('N', 'N', Gr, G2, Gr, batch, w.GAm, Mat{Xin, sg, Gr}, w.P1, sg, Gr, 1.f, exact ? w.P1 : nullptr, sg,
                                Gr, exact ? 1.f : 0.f);
        dp.amax_out = pl.h2g ? pm : nullptr;
        JSTSP_TRY(launch_cgemm(ctx, dp, GEMM_MISC));
        return second_factor(out, pm, exact);
    }

    // -- the gradient step of Alg. 2: res = A^H Tc - R v (:47), alpha from R res (:48), v += alpha res, ce(i,3), s = soft(v) (.* Omega_S)
    //    (:49-56, angles :36,:68), and the refresh of a support policy.
    // R v is recomputed from v every 4th iteration and carried by R v += alpha R res in between (the period: DESIGN.md section 5a).
    // Behind a pass with side streams (rv_early_ok) the recomputation for iteration it is issued EARLY on s2, after step_v of
    // iteration it - 1, which then does not carry R v forward.  Hazards, all closed by ev_v / ev_rv: R v is written after
    // step_v(it - 1), the last main-stream kernel of that iteration that touches it, and before its first reader of iteration it (the
    // Res product); V is not written again before step_v(it), behind ev_rv; the product's scratch is w.P1, which the main stream does
    // not touch between the G_B apply of it - 1 and the Res / P1 launch of it (behind ev_rv).
    int gradient_step()
    {
        const bool refreshed = it % 4 == 0;
        if (refreshed && rv_early) {
            JSTSP_HIP(hipStreamWaitEvent(sm, ev_rv, 0));       // recomputed on s2 since step_v of the previous iteration
            rv_early = false;
        } else if (refreshed) JSTSP_TRY(apply_R(w.V, w.RV, true));
        if (svt_split && pl.rv_fused1 && pl.h2g) {
            // behind a pass (gradstep.hip): Res and P1 = G_A Res from ONE launch - the 64 x 64 tile of Res is the whole k range of
            // the second product for its columns and stays in LDS; same MFMA chains, same bits
            uint32_t *pm = pmax_slot();
            JSTSP_TRY(launch_grad_res_p1(ctx, w.A, p.strideA, w.Tc, w.RV, w.Res, w.GA, pl.sGA, w.P1, pm, G2, batch));
            JSTSP_TRY(second_factor(w.RRes, pm, false));
        } else {
            GemmDesc dres = make_gemm('C', 'N', Gr, G2, N, batch, w.Am, Mat{w.Tc, sng, N}, w.Res, sg, Gr, 1.f, w.RV, sg, Gr, -1.f);
            JSTSP_TRY(launch_cgemm(ctx, dres, GEMM_MISC));
            JSTSP_TRY(apply_R(w.Res, w.RRes, false));
        }
        if (svt_split) {        // the eigen-decomposition behind the G_B apply (a resident Jacobi workgroup leaves that apply no room on its CU)
            JSTSP_HIP(hipEventRecord(ev_q1, sm));
            JSTSP_HIP(hipStreamWaitEvent(s1, ev_q1, 0));
            JSTSP_TRY(side_chain(2));
        }
        // (when the next iteration recomputes R v early, R v += alpha R res would be overwritten: not formed)
        const bool early_next = pl.rv_early_ok && it + 1 < Imax && (it + 1) % 4 == 0;
        // The pass at the end of this iteration accumulates the operand maxima of iteration it + 1 (k, X, V1, next Z) in block
        // (it + 1) & 1: step_v zeroes it (JSTSP_FUSED=2: a memset in front of the pass).  Every reader of that block from
        // iteration it - 1 is behind an event the main stream has waited for by now: the three-Gram pass and svt_prepare
        // (ev_gxv, ev_svt at the top of this iteration), the Gram of V2 (ev_gv2, here).
        uint32_t *const nx_zero = (pl.fusedp && pl.grad_fused && it + 1 < Imax) ? maxima(it + 1) : nullptr;
        if (nx_zero && it > 0 && pl.want_ce) JSTSP_HIP(hipStreamWaitEvent(sm, ev_gv2, 0));
        next_zeroed = nx_zero != nullptr;
        const bool fresh = p.refresh_at((long long)p.it0 + it + 1);
        JSTSP_TRY(launch_step_v(ctx, (int)sg, batch, w.Res, w.RRes, w.V, w.S, in_force && !fresh ? w.rank : nullptr, cnt, w.prm, w.ce,
                                Imax, it, early_next ? nullptr : w.RV, svt_split, nx_zero));
        if (early_next) {
            JSTSP_HIP(hipEventRecord(ev_v, sm));
            JSTSP_HIP(hipStreamWaitEvent(s2, ev_v, 0));
            StreamScope sc(ctx, s2);
            JSTSP_TRY(launch_grad_refresh_p1(ctx, w.V, w.GA, w.GAlo, pl.sGA, w.P1, G2, batch));
            JSTSP_TRY(second_factor(w.RV, nullptr, true));
            JSTSP_HIP(hipEventRecord(ev_rv, s2));
            rv_early = true;
        }
        if (fresh) {
            // the order of the new v and S again under it, on the main stream in front of the A S product.  The early R v
            // on s2 (ev_v) only reads V, as these two do; nothing else touches w.rank or w.S before the product.
            JSTSP_TRY(launch_support_top(ctx, (int)sg, batch, pl.R, w.V, w.top, w.rank, svt_split));
            JSTSP_TRY(launch_soft(ctx, (int)sg, batch, w.V, w.S, w.rank, cnt, w.prm));
            in_force = listed = true;
        }
        return 0;
    }

    // -- the stopping rule of jstsp_proposed_until_c32 (until.hip; every other entry: not one launch).  All of it
    //    on the main stream.  stop_test sits behind the gradient step - and behind a refresh's rewrite of S and the rank - and in
    //    front of the synthesis: one thread per trial reads row it of ce(:, 3), and the trials it has just stopped (every running
    //    one in the call's last iteration) are captured in two halves.  Here: S, v, the order, Y of this iteration - which a live
    //    rule makes update_x and every pass store - and X, V1, which the pass at the end of this iteration overwrites with those
    //    of it + 1; also the pass's overflow flag as it stands: a flag the trial raises later, running on, concerns only
    //    iterations that are not returned (the pass of iteration it raises it for the k of it + 1; its V2 does not depend on the
    //    k scale: fused.hip).  capture_tail, behind the synthesis: V2 (and C), which exist only there.
    int stop_test(bool last)
    {
        JSTSP_TRY(launch_until_test(ctx, batch, it + 1, p.min_iters, last, w.ce, Imax, it, pl.fusedp ? w.fw.ovf : nullptr, w.un));
        if (!pl.live) return 0;
        return launch_until_capture_head(ctx, snm, sg, pl.R, batch, w.X, w.V1, w.Y, w.V, w.S, listed, w.un, w.sout);
    }
    int capture_tail()
    {
        if (!w.sout) return 0;
        return launch_until_capture_tail(ctx, snm, sg, batch, w.V2, pl.explicit_c ? w.C : nullptr, w.un, w.sout);
    }
    // every `check` iterations: the one int the host reads, with one synchronisation of the main stream
    int running(int *left)
    {
        JSTSP_TRY(launch_until_count(ctx, batch, w.un));
        JSTSP_HIP(hipMemcpyAsync(left, w.un.left, sizeof(int), hipMemcpyDeviceToHost, sm));
        JSTSP_HIP(hipStreamSynchronize(sm));
        return 0;
    }
    // A loop that leaves before Imax leaves work on the side streams that reads the workspace (the norms and the early R v on s2,
    // whatever s1 still holds): the main stream waits for both before anything is copied out or the next call reuses the arena.
    int join_side_streams()
    {
        if (s1 != sm) { JSTSP_HIP(hipEventRecord(ev_x, s1)); JSTSP_HIP(hipStreamWaitEvent(sm, ev_x, 0)); }
        if (s2 != sm) { JSTSP_HIP(hipEventRecord(ev_c, s2)); JSTSP_HIP(hipStreamWaitEvent(sm, ev_c, 0)); }
        return 0;
    }

    // -- 'std': v = U\(L\k) = pinv(A) K pinv(B)   [ = G_A^-1 (A^H Tc) G_B^-1 on the Gram route: GA / GB hold the inverses ]  (:53,:56)
    int least_squares_step()
    {
        float2 *left = w.PB ? w.V : w.P1;        // result of the A side; the B side (if any) finishes into V
        if (w.PA)
            JSTSP_TRY(gemm(ctx, 'N', 'N', Gr, G2, N, batch, Mat{w.PA, p.strideA ? (long long)Gr * N : 0, Gr}, Mat{w.Tc, sng, N}, left, sg, Gr));
        else {
            JSTSP_TRY(gemm(ctx, 'C', 'N', Gr, G2, N, batch, w.Am, Mat{w.Tc, sng, N}, w.Res, sg, Gr));
            JSTSP_TRY(gemm(ctx, 'N', 'N', Gr, G2, Gr, batch, w.GAm, Mat{w.Res, sg, Gr}, left, sg, Gr));
        }
        if (!w.PB) JSTSP_TRY(gemm(ctx, 'N', 'N', Gr, G2, G2, batch, Mat{w.P1, sg, Gr}, w.GBm, w.V, sg, Gr));
        return launch_soft(ctx, (int)sg, batch, w.V, w.S, w.rank, cnt, w.prm);
    }

    // -- W = A S, then Xs = W B (:58) with sub 4 and the V2 dual update (:61,:65): in the fused pass, which also applies the next
    //    iteration's sub 1 / sub 2 (waits for ev_svt: its I - Q), in the product's epilogue, or as update_c.  Waits for ev_gv2 (the
    //    norms' Gram of the V2 it overwrites).
    int synthesize()
    {
        const long long strideB = p.strideB;
        GemmDesc dw = make_gemm('N', 'N', N, G2, Gr, batch, w.Am, Mat{w.S, sg, Gr}, w.W, sng, N);
        if (pl.h2) dw.amax_out = w.wmax;            // max|A S| for the split-f16 synthesis
        JSTSP_TRY(launch_cgemm(ctx, dw, GEMM_MISC));
        if (it > 0 && pl.want_ce) JSTSP_HIP(hipStreamWaitEvent(sm, ev_gv2, 0));
        passed = false;
        if (pl.fusedp && it + 1 < Imax) {
            // the pass writes the operand maxima of iteration it + 1 (k, X, V1, next Z): zero that block now
            uint32_t *nx = maxima(it + 1);
            if (!next_zeroed) JSTSP_HIP(hipMemsetAsync(nx, 0, 8 * (size_t)batch * sizeof(uint32_t), sm));
            const FusedWS &fw = w.fw;
            JSTSP_TRY(fused_pack_as(ctx, fw, w.W, sng, G2, M, batch, w.wmax));
            JSTSP_HIP(hipStreamWaitEvent(sm, ev_svt, 0));          // Y of the next iteration (side stream s1)
            FusedDesc fd{fw.Bf, strideB ? fw.sBf : 0, w.Bc.bmax, strideB ? 1 : 0, fw.ASp, fw.sAS, w.wmax, w.kmax,
                         w.X, w.V1, w.V2, w.subY, w.Y, w.omega_direct ? w.Omega : w.invD, snm, w.prm, fw.Ppart,
                         nx, nx + batch, nx + 2 * (size_t)batch, nx + 4 * (size_t)batch, w.nmax + 2 * (size_t)batch, fw.ovf,
                         M, G2, batch, pl.fparts,
                         fw.Wqp, Zbuf[(it + 1) & 1], w.zmax,
                         (fw.v2 && pl.zfly) ? nullptr : Zbuf[it & 1],      // (window kernel: Z comes from the staged X, V1)
                         (it + 2 == Imax || pl.live) ? w.Y : nullptr, pl.fused_kback,
                         fw.Ec, strideB ? fw.sEc : 0, fw.gt ? 31 - __builtin_clz((unsigned)fw.gt) : 0, fw.ecols, fw.ehalo,
                         fw.v2, fw.XsD, fw.Kf, w.omega_direct ? 1 : 0};
            JSTSP_TRY(launch_fused_pass(ctx, fd));
            passed = true;
        } else if (pl.h2) {
            // a(i, k = g) = W[i + N g] in fragment order, once per iteration instead of once per j-tile
            JSTSP_TRY(hgemm_repack(ctx, w.Wp, w.W, sng, N, 1, 0, G2, N, w.wmax));
            if (!w.Bs.data)
                JSTSP_TRY(hgemm_pack(ctx, w.Bs, ctx->arena, w.B, strideB, 1, G2, 0, G2, M, pl.nB, (long long)G2 * M, w.Bc.bmax));
            HGemmDesc hs{w.W, sng, N, w.wmax, w.Bs.data, strideB ? w.Bs.st : 0, w.Bs.bmax, strideB ? 1 : 0, w.Bs.KS,
                         w.Bs.JT, w.Xs, snm, N, N, M, G2, batch, pl.fz ? EPI_UPDATE_C : EPI_NONE, w.prm, w.X, w.V2,
                         pl.hmax ? w.nmax + 2 * (size_t)batch : nullptr, w.Wp.data, w.Wp.st, w.Wp.KS};
            JSTSP_TRY(launch_hgemm(ctx, hs, "synthesize"));
            if (!pl.fz) JSTSP_TRY(launch_update_c(ctx, snm, batch, w.X, w.Xs, w.V2, w.C, w.prm));
        } else if (pl.fz) {
            GemmDesc ds = make_gemm('N', 'N', N, M, G2, batch, Mat{w.W, sng, N}, w.Bm, w.Xs, snm, N);
            ds.epi = EPI_UPDATE_C; ds.prm = w.prm;
            ds.e_r0 = w.X; ds.e_rw0 = w.V2;
            JSTSP_TRY(launch_cgemm(ctx, ds, GEMM_SYNTH));
        } else {
            JSTSP_TRY(gemm(ctx, 'N', 'N', N, M, G2, batch, Mat{w.W, sng, N}, w.Bm, w.Xs, snm, N, 1.f, nullptr, 0, 0, 0.f, GEMM_SYNTH));
            JSTSP_TRY(launch_update_c(ctx, snm, batch, w.X, w.Xs, w.V2, w.C, w.prm));
        }
        return 0;
    }

    // -- convergence_error(i,1:2) = norm(V1)^2/norm(X)^2, norm(V2)^2/norm(X)^2 (:67,:69) on s2: Gram of V2 (ev_c -> ev_gv2), lambda_max,
    //    the ratios (ev_ce: the copy-out waits for the last one)
    int norms()
    {
        JSTSP_HIP(hipEventRecord(ev_c, sm));
        JSTSP_HIP(hipStreamWaitEvent(s2, ev_c, 0));
        if (pl.zfly) JSTSP_HIP(hipStreamWaitEvent(s2, ev_gxv, 0));      // G_x, G_v1 came from the side stream s1
        StreamScope sc(ctx, s2);
        JSTSP_TRY(gram_partials_range(ctx, w.gn, w.X, snm, 2 * batch, batch, pl.hmax ? w.nmax : nullptr, nullptr, nullptr, true));
        JSTSP_HIP(hipEventRecord(ev_gv2, s2));
        if (pl.fusedp && pl.zfly && it + 1 < Imax) JSTSP_TRY(lmax_from_partials_range(ctx, w.gn, 2 * batch, batch, w.lam, true));
        else JSTSP_TRY(lmax_from_partials(ctx, w.gn, w.lam, true));
        JSTSP_TRY(launch_ce_ratio(ctx, batch, w.lam + batch, w.lam + 2 * batch, w.lam, w.ce, Imax, it));
        JSTSP_HIP(hipEventRecord(ev_ce, s2));
        return 0;
    }
};

// The copies of a solve's results into the outputs of its problem (on ctx->stream): the second phase of a deferred solve ...
static int deferred_copy_out(jstsp_ctx *ctx, const PendingSolve &d, const AdmmProblem &p)
{
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(p.S_out), d.dS, p.batch * p.g(), p.memspace));
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(p.Y_out), d.dY, p.batch * p.nm(), p.memspace));
    if (d.want_ce) JSTSP_TRY(stage_out(ctx, p.ce_out, d.dce, (size_t)p.batch * 3 * p.Imax, p.memspace));
    return 0;
}

// The end of a solve.  defer: the results stay in the workspace; copies, flags and recovery happen in proposed_finish or the caller.
// Otherwise the copy-out, the state, and (ONE stream synchronisation at the end of a solve that used the fused pass) the trials in
// which an entry of k left the f16 range of the scale predicted for it: wrong from that pass on, the caller re-solves exactly those.
static int finish_solve(jstsp_ctx *ctx, const AdmmProblem &p, const AdmmPlan &pl, ProposedWS &w, std::vector<int> *overflowed, PendingSolve *defer)
{
    const int batch = p.batch, memspace = p.memspace;
    // (under a live stopping rule every trial was captured at its own last iteration: S, Y, the order and the flags are the
    //  captured ones - in a device call already in the caller's arrays - and the state is packed)
    const bool live = pl.live;
    const PendingSolve d{pl.want_ce && p.Imax > 0, live ? w.un.S : w.S, live ? w.un.Y : w.Y, w.ce,
                         pl.fusedp ? (live ? w.un.ovf : w.fw.ovf) : nullptr};
    if (defer) { *defer = d; return 0; }
    if (live && d.want_ce) JSTSP_TRY(launch_until_mask_ce(ctx, batch, p.Imax, w.un, w.ce));
    if (live && memspace == JSTSP_DEVICE) {
        if (d.want_ce) JSTSP_TRY(stage_out(ctx, p.ce_out, d.dce, (size_t)batch * 3 * p.Imax, memspace));
    } else
        JSTSP_TRY(deferred_copy_out(ctx, d, p));
    const int32_t *top = live ? w.un.top : w.top;
    if (top && memspace == JSTSP_HOST) JSTSP_TRY(stage_out(ctx, p.indx_out, top, (size_t)batch * pl.R, memspace));
    if (w.sout) {
        if (!live)
            JSTSP_TRY(launch_resume_pack(ctx, (long long)p.nm(), (long long)p.g(), batch, w.X, w.V1, w.V2, pl.explicit_c ? w.C : nullptr, w.V, w.S, w.sout));
        if (memspace == JSTSP_HOST) JSTSP_TRY(stage_out(ctx, as_f2(p.state_out), w.sout, batch * p.state_elems(), memspace));
    }
    if (pl.until) {
        JSTSP_TRY(stage_out(ctx, p.iters_out, (const int32_t *)w.un.iters, (size_t)batch, memspace));
        JSTSP_TRY(stage_out(ctx, p.ce3_out, (const double *)w.un.ce3, (size_t)batch, memspace));
    }
    if (d.ovf && overflowed) JSTSP_TRY(read_flagged_trials(ctx, d.ovf, batch, overflowed));
    if (memspace == JSTSP_HOST) {
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
        if (!pl.approx) JSTSP_TRY(diag_check_host(ctx, "proposed_algorithm 'std'"));
    }
    return 0;
}

// One batched solve.  allow_fused = false: never the fused pass (the re-solve of trials whose predicted k scale
// overflowed in it).  overflowed != NULL: receives the indices of such trials (their outputs are not to be used).
// defer != NULL: the results stay in the context's workspace (the halves of a pipelined host call, the two-phase form).
static int proposed_impl(jstsp_ctx *ctx, const AdmmProblem &p, bool allow_fused, std::vector<int> *overflowed, PendingSolve *defer = nullptr)
{
    JSTSP_TRY(check_arguments(ctx, p));
    JSTSP_ENTER(ctx);
    AdmmPlan pl = make_plan(p, tune(), allow_fused);          // (the switches of this call: common.h, parsed at JSTSP_ENTER)
    JSTSP_TRY(ctx->arena.reserve(proposed_bytes(p, pl)));
    ctx->arena.reset();

    ProposedWS w;
    JSTSP_TRY(stage_inputs(ctx, p, pl, w));
    JSTSP_TRY(proposed_alloc(ctx->arena, w, p, pl));
    plan_gram_choices(pl, p, w);
    JSTSP_TRY(setup_scalars(ctx, p, pl, w));
    JSTSP_TRY(setup_resumed(ctx, p, pl, w));
    JSTSP_TRY(setup_grams(ctx, p, pl, w));
    if (!pl.approx) JSTSP_TRY(setup_std_factors(ctx, p, pl, w));

    JSTSP_TRY(ensure_side_streams(ctx));
    AdmmLoop L{ctx, p, pl, w};
    JSTSP_TRY(setup_fused(ctx, p, pl, w));
    // convergence_error(:,1:2): lambda_max of three Grams per trial and iteration, each warm-started from its own Ritz vector
    // of the previous iteration (eig2.hip); the record starts empty
    if (pl.want_ce) JSTSP_TRY(lanczos_warm_reset(ctx, w.gn));
    bool left_early = false;            // a live stopping rule: every trial had stopped before Imax
    for (int it = 0; it < p.Imax; ++it) {
        const bool last = it + 1 == p.Imax;
        JSTSP_TRY(L.begin(it));
        JSTSP_TRY(L.update_x());
        if (it + 1 < p.Imax) JSTSP_TRY(L.side_chain(L.svt_split ? 1 : 0));
        JSTSP_TRY(L.gram_xv());
        JSTSP_TRY(L.correlate());
        JSTSP_TRY(pl.approx ? L.gradient_step() : L.least_squares_step());
        if (pl.until && (pl.live || last)) JSTSP_TRY(L.stop_test(last));
        // (the last iteration of a two-output call on the fused path: Xs only feeds X, V2 and convergence_error, none of which
        //  is returned - S is final, Y was stored by the last pass; a call that returns its state needs the last V2)
        if (L.xs_unused()) break;
        JSTSP_TRY(L.synthesize());
        if (pl.want_ce) JSTSP_TRY(L.norms());
        if (!pl.live) continue;
        JSTSP_TRY(L.capture_tail());
        if (last || (it + 1) % p.check) continue;
        int left = 0;
        JSTSP_TRY(L.running(&left));
        if (left == 0) { left_early = true; break; }
    }
    if (left_early) JSTSP_TRY(L.join_side_streams());
    else if (pl.want_ce && p.Imax > 0) JSTSP_HIP(hipStreamWaitEvent(L.sm, L.ev_ce, 0));
    return finish_solve(ctx, p, pl, w, overflowed, defer);
}

// Recovery: runs of consecutive flagged trials are solved again by the three-kernel iteration (every operand scale
// there is the exact maximum of data that already exists: it cannot overflow), straight into the caller's arrays - a
// sub-batch of a problem is a problem in either memspace (AdmmProblem::sub); a resumed call's run starts from ITS state_in
// at it0.  *count grows by the trials solved again.
static int resolve_overflowed(jstsp_ctx *ctx, const AdmmProblem &p, const std::vector<int> &flagged, int *count)
{
    return for_each_run(flagged, [&](int t0, int cnt) -> int {
        JSTSP_TRY(proposed_impl(ctx, p.sub(t0, cnt), false, nullptr));
        *count += cnt;
        return 0;
    });
}

int jstsp::read_flagged_trials(jstsp_ctx *ctx, const uint32_t *dev_flags, int batch, std::vector<int> *out)
{
    std::vector<uint32_t> flags(dev_flags ? batch : 0);
    if (dev_flags) JSTSP_HIP(hipMemcpyAsync(flags.data(), dev_flags, (size_t)batch * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    flagged_trials(flags.data(), flags.size(), out);
    return 0;
}

// ... and, for a JSTSP_HOST solve, the overflow flags with one synchronisation.
static int proposed_finish(jstsp_ctx *ctx, const PendingSolve &d, const AdmmProblem &p, std::vector<int> *ovf)
{
    JSTSP_ENTER(ctx);
    JSTSP_TRY(deferred_copy_out(ctx, d, p));
    return read_flagged_trials(ctx, d.ovf, p.batch, ovf);
}

// One solve in the caller's memspace with its recovery: the flagged trials again, and how many they were for
// jstsp_last_fused_fallbacks.  (The entries zero that counter; proposed_impl never touches it.)
static int solve_and_recover(jstsp_ctx *ctx, const AdmmProblem &p)
{
    std::vector<int> ovf;
    JSTSP_TRY(proposed_impl(ctx, p, true, &ovf));
    int fallbacks = 0;
    JSTSP_TRY(resolve_overflowed(ctx, p, ovf, &fallbacks));
    ctx->fused_fallbacks = fallbacks;
    return 0;
}

extern "C" int jstsp_proposed_algorithm_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                                            const jstsp_c32 *subY, const float *Omega,
                                            const jstsp_c32 *A, long long strideA, const jstsp_c32 *B,
                                            long long strideB, int Imax, const double *tau_Y,
                                            const double *tau_S, const double *rho, int type,
                                            const int32_t *indx_S, jstsp_c32 *S_out, jstsp_c32 *Y_out,
                                            double *ce_out, int memspace)
{
    if (ctx) { ctx->fused_fallbacks = 0; ctx->last_dict_block = 0; }
    const AdmmProblem p{N, M, Gr, G2, batch, subY, Omega, A, B, tau_Y, tau_S, rho, strideA, strideB, Imax, type, indx_S, S_out, Y_out, ce_out,
                        0, nullptr, nullptr, memspace};
    // JSTSP_HOST with a large batch: the two halves of the batch on two contexts of the device, so that the upload of the second
    // half (4.75 GiB per 256 trials at BASELINE configs[1], 57 GB/s) runs while the first half is being solved, and the download
    // of the first half while the second is.  A trial's result does not depend on what else is in its batch (tests), so the
    // outputs are those of the one-call form.  Measured at configs[1] (tools/host_path_rate.py): 256 trials 544 -> 594
    // channel-estimates/s, 128 trials 514 -> 540, 64 trials 466 -> 391 (a 32-trial solve no longer fills the chip): from 128 on.
    const size_t in_bytes = (size_t)batch * (p.nm() * 12 + (strideB ? (size_t)G2 * M * 8 : 0));
    const bool pipeline = ctx && memspace == JSTSP_HOST && type == JSTSP_TYPE_APPROXIMATE && batch >= 128 && Imax > 1 && Y_out &&
                          in_bytes >= ((size_t)256 << 20) && subY && Omega && A && B && tau_Y && tau_S && rho && S_out &&
                          tune_host_pipeline();
    if (pipeline) {
        HostPipeline pipe;
        JSTSP_TRY(pipe.open(ctx, batch));
        const AdmmProblem half[2] = {p.sub(pipe.t0[0], pipe.cnt[0]), p.sub(pipe.t0[1], pipe.cnt[1])};
        PendingSolve pend[2];
        for (int k = 0; k < 2; ++k) {
            pipe.cx[k]->fused_fallbacks = 0; pipe.cx[k]->last_dict_block = 0;
            JSTSP_TRY_PIPE(pipe, proposed_impl(pipe.cx[k], half[k], true, nullptr, &pend[k]));
        }
        for (int k = 0; k < 2; ++k) {
            std::vector<int> o;
            JSTSP_TRY_PIPE(pipe, proposed_finish(pipe.cx[k], pend[k], half[k], &o));
            JSTSP_TRY_PIPE(pipe, resolve_overflowed(pipe.cx[k], half[k], o, &pipe.fallbacks));
        }
        pipe.close();
        return 0;
    }
    return solve_and_recover(ctx, p);       // (the resumed entry below from zero, without a state)
}

// The body of the resumed entries: one staged solve with its recovery.  state_out == state_in: the re-solve needs the state the
// call started from, so a copy is taken first.
static int resumed_solve(jstsp_ctx *ctx, const char *nmf, AdmmProblem &p)
{
    const int batch = p.batch, memspace = p.memspace;
    const jstsp_c32 *state_in = p.state_in;
    ctx->fused_fallbacks = 0; ctx->last_dict_block = 0;
    const size_t ne = p.state_elems();
    jstsp_c32 *keep_dev = nullptr;
    std::vector<jstsp_c32> keep_host;
    if (state_in && state_in == p.state_out) {
        if (memspace == JSTSP_HOST) { keep_host.assign(state_in, state_in + (size_t)batch * ne); p.state_in = keep_host.data(); }
        else {
            JSTSP_ENTER(ctx);
            JSTSP_HIP(hipMallocAsync((void **)&keep_dev, (size_t)batch * ne * sizeof(jstsp_c32), ctx->stream));
            const hipError_t e = hipMemcpyAsync(keep_dev, state_in, (size_t)batch * ne * sizeof(jstsp_c32), hipMemcpyDeviceToDevice, ctx->stream);
            if (e != hipSuccess) {
                (void)hipFreeAsync(keep_dev, ctx->stream);
                set_error("%s: copying the state failed: %s", nmf, hipGetErrorString(e));
                return (int)e;
            }
            p.state_in = keep_dev;
        }
    }
    const int rc = solve_and_recover(ctx, p);
    if (keep_dev) {
        JSTSP_ENTER(ctx);
        (void)hipFreeAsync(keep_dev, ctx->stream);
    }
    return rc;
}

// ---- resumed from a saved state, with a support policy, with a stopping rule (include/jstsp.h) -----------------------------------
// jstsp_proposed_resume_c32: iterations it0 + 1 ... it0 + Imax from state_in.  One staged solve in either memspace (no two-halves
// host pipeline).  A trial whose k scale overflowed in a pass is solved again from ITS state_in at it0 by the three-kernel iteration;
// state_in is read again for that, so when the caller lets state_out be state_in a copy is taken first.
// jstsp_proposed_refresh_c32: the same with a support policy in the record (solver_common.h): the schedule, the limit R and indx_out
// are those of jstsp_proposed_refresh_f64.  'approximate' only.  A flagged trial is solved again from its state_in at it0 under the
// same policy, and its indx_out comes from that re-solve (AdmmProblem::sub moves both lists).
// jstsp_proposed_until_c32: either of the two with the stopping rule in the record (AdmmLoop::stop_test says
// what runs where).  A flagged trial is solved again under the same rule.
// The record says which entry it came through: a rule - until; else a policy - refresh; else resume.  Each keeps the order of its
// checks; the solver's own (check_arguments) follow inside the solve.
int jstsp::proposed_resumed_entry(jstsp_ctx *ctx, AdmmProblem &p)
{
    const bool plain = !p.rule && !p.policy;
    const char *nmf = p.rule ? "proposed_algorithm until" : p.policy ? "proposed_algorithm refresh" : "proposed_algorithm resume";
    const bool shape_ok = p.N > 0 && p.M > 0 && p.Gr > 0 && p.G2 > 0 && p.batch > 0 && p.Imax > 0;
    if (plain) {
        JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
        JSTSP_REQUIRE(p.memspace == JSTSP_HOST || p.memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", p.memspace);
        JSTSP_REQUIRE(shape_ok, JSTSP_E_SHAPE, "%s: bad shape", nmf);
        JSTSP_TRY(check_resumed(nmf, p));
        return resumed_solve(ctx, nmf, p);
    }
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: ctx is NULL", nmf);
    JSTSP_REQUIRE(p.memspace == JSTSP_HOST || p.memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace %d", nmf, p.memspace);
    JSTSP_REQUIRE(shape_ok && p.strideA >= 0 && p.strideB >= 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE((long long)p.Gr * p.G2 < (1ll << 31), JSTSP_E_SHAPE, "%s: Gr * G2 = %lld exceeds 2^31 - 1", nmf, (long long)p.Gr * p.G2);
    JSTSP_REQUIRE(p.subY && p.Omega && p.A && p.B && p.tau_Y && p.tau_S && p.rho && p.S_out, JSTSP_E_NULL, "%s: NULL argument", nmf);
    if (p.rule) JSTSP_TRY(check_rule_arrays(nmf, p));
    JSTSP_REQUIRE(p.type == JSTSP_TYPE_APPROXIMATE || p.type == JSTSP_TYPE_STD, JSTSP_E_ARG, "%s: bad type %d", nmf, p.type);
    JSTSP_REQUIRE(p.type == JSTSP_TYPE_APPROXIMATE, JSTSP_E_UNSUPPORTED,
                  p.rule ? "%s: the rule reads the gradient step of Alg. 2; 'std' recomputes v by least squares and has none: use jstsp_proposed_resume_c32"
                         : "%s: 'std' recomputes v by least squares in every iteration and has no refreshed form: use jstsp_proposed_resume_c32",
                  nmf);
    if (p.rule) JSTSP_TRY(check_rule_counts(nmf, p));
    JSTSP_TRY(check_resumed(nmf, p));
    if (!p.rule) JSTSP_TRY(check_policy(nmf, p));
    else if (p.policy) {
        JSTSP_REQUIRE(p.start >= 0, JSTSP_E_ARG, "%s: refresh_start = %d: may not be negative (refresh_period < 0: no policy)", nmf, p.start);
        JSTSP_TRY(check_policy(nmf, p, false));
    } else JSTSP_TRY(check_rule_list(nmf, p));
    return resumed_solve(ctx, nmf, p);
}

#define RESUMED_RECORD                                                                                                                      \
    AdmmProblem p{N, M, Gr, G2, batch, subY, Omega, A, B, tau_Y, tau_S, rho, strideA, strideB, Imax, type, indx_S, S_out, Y_out, ce_out, it0, \
                  state_in, state_out, memspace}

extern "C" int jstsp_proposed_resume_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *subY, const float *Omega,
                                         const jstsp_c32 *A, long long strideA, const jstsp_c32 *B, long long strideB, int Imax,
                                         const double *tau_Y, const double *tau_S, const double *rho, int type, const int32_t *indx_S,
                                         jstsp_c32 *S_out, jstsp_c32 *Y_out, double *ce_out, int it0, const jstsp_c32 *state_in,
                                         jstsp_c32 *state_out, int memspace)
{
    RESUMED_RECORD;
    return proposed_resumed_entry(ctx, p);
}

extern "C" int jstsp_proposed_refresh_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *subY, const float *Omega,
                                          const jstsp_c32 *A, long long strideA, const jstsp_c32 *B, long long strideB, int Imax,
                                          const double *tau_Y, const double *tau_S, const double *rho, int type, const int32_t *indx_S, int n_indx,
                                          int refresh_start, int refresh_period, jstsp_c32 *S_out, jstsp_c32 *Y_out, double *ce_out, int it0,
                                          const jstsp_c32 *state_in, jstsp_c32 *state_out, int32_t *indx_out, int memspace)
{
    RESUMED_RECORD;
    p.set_policy(n_indx, refresh_start, refresh_period, indx_out);
    return proposed_resumed_entry(ctx, p);
}

// (refresh_period < 0: no policy - n_indx then counts the entries per trial of indx_S, 0 meaning all)
extern "C" int jstsp_proposed_until_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *subY, const float *Omega,
                                        const jstsp_c32 *A, long long strideA, const jstsp_c32 *B, long long strideB, int Imax,
                                        const double *tau_Y, const double *tau_S, const double *rho, int type, const int32_t *indx_S, int n_indx,
                                        int refresh_start, int refresh_period, const double *tol, int min_iters, int check, jstsp_c32 *S_out,
                                        jstsp_c32 *Y_out, double *ce_out, int it0, const jstsp_c32 *state_in, jstsp_c32 *state_out,
                                        int32_t *indx_out, int32_t *iters_out, double *ce3_out, int memspace)
{
    RESUMED_RECORD;
    p.n_indx = n_indx;
    if (refresh_period >= 0) p.set_policy(n_indx, refresh_start, refresh_period, indx_out);
    p.set_rule(tol, min_iters, check, iters_out, ce3_out);
    return proposed_resumed_entry(ctx, p);
}
#undef RESUMED_RECORD

// ---- the two-phase form for device arrays (include/jstsp.h) ---------------------------------------------------------------------
struct jstsp_pending {
    AdmmProblem prob;                   // the call's problem; its tau_Y, tau_S, rho point into the copies below
    std::vector<double> tau_Y, tau_S, rho;
    uint32_t *flags = nullptr;          // pinned host copy of the per-trial overflow flags (NULL: the solve did not use the fused pass)
    hipEvent_t done = nullptr;
};

extern "C" int jstsp_proposed_algorithm_begin_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *subY,
                                                  const float *Omega, const jstsp_c32 *A, long long strideA, const jstsp_c32 *B,
                                                  long long strideB, int Imax, const double *tau_Y, const double *tau_S,
                                                  const double *rho, int type, const int32_t *indx_S, jstsp_c32 *S_out,
                                                  jstsp_c32 *Y_out, double *ce_out, jstsp_pending **pending)
{
    JSTSP_REQUIRE(ctx && pending, JSTSP_E_NULL, "proposed_algorithm_begin: NULL context or handle pointer");
    *pending = nullptr;
    ctx->fused_fallbacks = 0; ctx->last_dict_block = 0;
    PendingSolve ps;
    const AdmmProblem prob{N, M, Gr, G2, batch, subY, Omega, A, B, tau_Y, tau_S, rho, strideA, strideB, Imax, type, indx_S, S_out, Y_out, ce_out,
                           0, nullptr, nullptr, JSTSP_DEVICE};
    JSTSP_TRY(proposed_impl(ctx, prob, true, nullptr, &ps));
    JSTSP_ENTER(ctx);
    JSTSP_TRY(deferred_copy_out(ctx, ps, prob));
    jstsp_pending *p = new (std::nothrow) jstsp_pending();
    JSTSP_REQUIRE(p, JSTSP_E_NOMEM, "proposed_algorithm_begin: out of host memory");
    p->prob = prob;
    p->tau_Y.assign(tau_Y, tau_Y + batch); p->tau_S.assign(tau_S, tau_S + batch); p->rho.assign(rho, rho + batch);
    p->prob.tau_Y = p->tau_Y.data(); p->prob.tau_S = p->tau_S.data(); p->prob.rho = p->rho.data();
    hipError_t e = hipSuccess;          // (positive status = the HIP error code, as everywhere in this ABI)
    if (ps.ovf) {
        e = hipHostMalloc((void **)&p->flags, (size_t)batch * sizeof(uint32_t), hipHostMallocDefault);
        if (e == hipSuccess) e = hipMemcpyAsync(p->flags, ps.ovf, (size_t)batch * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(p->done, ctx->stream);
    const int rc = (int)e;
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        if (p->flags) (void)hipHostFree(p->flags);
        if (p->done) (void)hipEventDestroy(p->done);
        delete p;
        set_error("proposed_algorithm_begin: could not set up the completion record: %s", hipGetErrorString(e));
        return rc;
    }
    *pending = p;
    return 0;
}

extern "C" int jstsp_proposed_algorithm_end(jstsp_ctx *ctx, jstsp_pending *p, int *fallbacks)
{
    JSTSP_REQUIRE(ctx && p, JSTSP_E_NULL, "proposed_algorithm_end: NULL context or handle");
    JSTSP_ENTER(ctx);
    int rc = 0, count = 0;
    const hipError_t e = hipEventSynchronize(p->done);
    if (e != hipSuccess) { set_error("proposed_algorithm_end: waiting for the solve failed: %s", hipGetErrorString(e)); rc = (int)e; }
    std::vector<int> ovf;
    if (!rc && p->flags) flagged_trials(p->flags, (size_t)p->prob.batch, &ovf);      // (the pinned copy: no further copy or wait)
    if (!rc) rc = resolve_overflowed(ctx, p->prob, ovf, &count);
    ctx->fused_fallbacks = count;
    if (fallbacks) *fallbacks = count;
    if (p->flags) (void)hipHostFree(p->flags);
    (void)hipEventDestroy(p->done);
    delete p;
    return rc;
}

namespace jstsp {
// (solver_common.h: the phases of a pipelined host call for c64.hip, which stages - and narrows - its inputs itself)
int proposed_enqueue_device(jstsp_ctx *ctx, const AdmmProblem &p, bool want_ce, PendingSolve *out)
{
    static jstsp_c32 sink_c;            // (a deferred solve never writes its output arguments; they only say what is wanted)
    static double sink_d;
    if (ctx) { ctx->fused_fallbacks = 0; ctx->last_dict_block = 0; }
    AdmmProblem q = p;
    q.S_out = q.Y_out = &sink_c; q.ce_out = want_ce ? &sink_d : nullptr;
    return proposed_impl(ctx, q, true, nullptr, out);
}
int proposed_resolve_device(jstsp_ctx *ctx, const AdmmProblem &run)
{
    return proposed_impl(ctx, run, false, nullptr);
}
}  // namespace jstsp

/* Trials of the last jstsp_proposed_algorithm_* call on this context that were solved a second time by the three-kernel
 * iteration because the fused pass's predicted operand scale overflowed for them (0 in all but pathological inputs). */
extern "C" int jstsp_last_fused_fallbacks(jstsp_ctx *ctx, int *count)
{
    JSTSP_REQUIRE(ctx && count, JSTSP_E_NULL, "last_fused_fallbacks: NULL argument");
    *count = ctx->fused_fallbacks;
    return 0;
}
/* Block height Gt of the block-Toeplitz structure the last jstsp_proposed_algorithm_* call found in its dictionary
 * (B(ld Gt + g, m) == B(g, m - ld) bit for bit; the pass then streams the first block only), 0 if it found none. */
extern "C" int jstsp_last_dictionary_block(jstsp_ctx *ctx, int *gt)
{
    JSTSP_REQUIRE(ctx && gt, JSTSP_E_NULL, "last_dictionary_block: NULL argument");
    *gt = ctx->last_dict_block;
    return 0;
}
