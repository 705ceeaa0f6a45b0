#!/usr/bin/env python
"""What a warm start buys on a slowly varying channel: `--seqs` independent sequences of `--frames`
frames at BASELINE configs[1]'s shape (or --small: the reference's own driver shape).  The channel of a sequence is the model of
wideband_mmwave_channel.m - clusters x rays paths whose Laplacian-distributed angles all delay taps share, cluster c weighted
(C - c), H_l = A_r diag(g_l w / sqrt(Np)) A_t^H - with the angles fixed over the sequence and the path gains g_l following a
first-order autoregression with coefficient `--corr` from one frame to the next (g_f = corr g_{f-1} + sqrt(1 - corr^2) w_f,
w_f ~ CN(0, 1): every frame's channel has the statistics of a drawn one).  Every frame has pilots, noise and sampling pattern of
its own.  Two sources of the channel:
  default           generated on the host by numpy and fed through build_trials(..., channel=H, channel_normalize="asis"); the
                    sweep index is the frame
  --device-channel  built by the library (jstsp_build_trials_tracked_c32 through montecarlo.run_tracking):
                    Philox draws keyed by (seed, sweep index, sequence) and the frame, the sweep index free for the SNR point;
                    states, estimates and scores stay on the device.  The two sources see different draws: their results agree
                    statistically, not number by number.

Per frame and sequence, in float64 (proposed_algorithm_resume_f64, nmse_spectral_f64; the default) or with --precision f32 by the
fp32 solver (proposed_algorithm_resume, nmse_spectral: its estimates/s are the ones the headline is about), at each Imax of --imax (and --cold-imax):
  cold     from zero
  warm     from the previous frame's whole state [X | V1 | V2 | C | v | S]; each Imax is a chain of its own
  warm_vs  from the previous frame's v and S only (X = V1 = V2 = C = 0): the part of the state that lives in the angle-delay
           domain and does not depend on the frame's pilots and sampling pattern
With --device-channel, --modes also takes the "Proposed - PAI" variants - pai: from zero with the frame's
own true support order (the genie of plot_errorVSsnr.m:143-145); pai_prev: from zero with the order of the chain's previous
estimate (support_order on the device); warm_pai_prev: the previous frame's whole state and that order - and --drift SIGMA lets the
angles of every sequence walk, SIGMA radians of standard deviation per frame, so the support moves across the dictionary grid.
pai_wide_prev and warm_pai_wide_prev are pai_prev and warm_pai_prev with the order widened over the
neighbouring angle cells (support_order_wide): --widen WR,WT cells each way on the receive and transmit grid, --widen-primary
neighbourhood (a strong entry, then its window) or ties (the plain order, its exact zeros by their strongest neighbour).
refresh, warm_refresh and pai_prev_refresh (float64 only) refresh the support from the solver's own iterate
inside the loop (proposed_algorithm_refresh_f64) - from zero, from the previous frame's state, and from zero with the order of the
chain's previous estimate in force until the first refresh: --refresh START,PERIOD, a refresh at the iterations i > START with
(i - START - 1) % PERIOD == 0, PERIOD 0 for the one refresh at START + 1 (default: 0,1, every iteration).  With --precision f32,
--refresh-f32 runs the three on the fp32 solver (proposed_algorithm_refresh).
cold_until, warm_until, refresh_until and warm_refresh_until (float64 only) are cold, warm, refresh and
warm_refresh with the stopping rule of proposed_algorithm_until_f64: --stop TOL[,MIN] stops each trial after its first iteration
i >= MIN (default 2) with |v_i - v_{i-1}|^2 / |v_{i-1}|^2 <= TOL; one solve per frame at --cold-imax, and the result also carries
the mean, median and largest number of iterations.  --stop without --modes runs these four.  With --precision f32, --until-f32
runs them on the fp32 solver (proposed_algorithm_until).
--refit K,ITERS (float64 only) also re-fits every scored estimate on its K largest entries by ITERS
conjugate-gradient steps (refit_f64) and scores it again: mean_nmse_refit, mean_nmse_refit_by_frame, refit_estimates_per_s per row.
A warm chain at Imax n has run n iterations in every earlier frame as well: by frame f it has accumulated f n iterations on a
channel that is corr^k-correlated with the one k frames back.  So the result is also given frame by frame: frame 2 (index 1) is
the warm start proper - n iterations on the previous frame plus n on this one - and the later frames show what accumulates.
Scored by nmse_spectral_f64 against the frame's Zbar; frame 1 (index 0: every mode starts from zero there) is left out.
Prints ONE JSON line: per (mode, Imax) the mean NMSE over the scored frames, its standard error over the sequences, the mean per
frame, and estimates/s.  No threshold is asserted."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import jstsp19_amd as J
from jstsp19_amd.system_model import SweepParams, build_trials

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--seqs", type=int, default=16)
ap.add_argument("--corr", type=float, default=0.95)
ap.add_argument("--snr-db", type=float, default=5.0)
ap.add_argument("--imax", type=int, nargs="+", default=[10, 20, 30, 50, 100])
ap.add_argument("--cold-imax", type=int, default=100)
ap.add_argument("--seed", type=int, default=20190913)
ap.add_argument("--precision", choices=("f64", "f32"), default="f64")
ap.add_argument("--small", action="store_true", help="Nt=4, Nr=32, L=4, T=35, Mr=4 instead of BASELINE configs[1]")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
ap.add_argument("--device-channel", action="store_true", help="frames built by the library (montecarlo.run_tracking)")
ap.add_argument("--sweep-idx", type=int, default=0, help="--device-channel: the sweep index of the sequences' Philox key")
ap.add_argument("--drift", type=float, default=None, metavar="SIGMA",
                help="--device-channel: random walk of every path angle, SIGMA rad per frame (default: fixed angles)")
ap.add_argument("--modes", nargs="+", default=None,
                choices=("cold", "warm", "warm_vs", "pai", "pai_prev", "warm_pai_prev", "pai_wide_prev", "warm_pai_wide_prev", "refresh",
                         "warm_refresh", "pai_prev_refresh", "cold_until", "warm_until", "refresh_until", "warm_refresh_until"),
                help="--device-channel: the columns to run (default: cold warm warm_vs; with --stop the four *_until modes)")
ap.add_argument("--widen", default=None, metavar="WR,WT",
                help="--device-channel: the radii of pai_wide_prev / warm_pai_wide_prev in grid cells (default: 1,1)")
ap.add_argument("--widen-primary", choices=("neighbourhood", "ties"), default=None,
                help="--device-channel: what the widened order sorts by first (default: neighbourhood)")
ap.add_argument("--refresh", default=None, metavar="START,PERIOD",
                help="--device-channel: the refresh schedule of refresh / warm_refresh / pai_prev_refresh (default: 0,1)")
ap.add_argument("--refresh-f32", action="store_true",
                help="--device-channel --precision f32: the refresh modes on the fp32 solver (proposed_algorithm_refresh)")
ap.add_argument("--until-f32", action="store_true",
                help="--device-channel --precision f32 --stop: the *_until modes on the fp32 solver (proposed_algorithm_until)")
ap.add_argument("--stop", default=None, metavar="TOL[,MIN]",
                help="--device-channel: the stopping rule of the *_until modes (tolerance and, default 2, the fewest iterations)")
ap.add_argument("--refit", default=None, metavar="K,ITERS",
                help="--device-channel: also score every estimate after a float64 re-fit on its K largest entries, ITERS steps")
a = ap.parse_args()
if a.refit is not None:
    if not a.device_channel:
        ap.error("--refit needs --device-channel")
    try:
        a.refit = tuple(int(x) for x in a.refit.split(","))
    except ValueError:
        a.refit = ()
    if len(a.refit) != 2 or min(a.refit) < 1:
        ap.error("--refit takes two integers >= 1 as K,ITERS")
if a.stop is not None:
    if not a.device_channel:
        ap.error("--stop needs --device-channel")
    try:
        parts = a.stop.split(",")
        a.stop = (float(parts[0]), int(parts[1]) if len(parts) > 1 else 2)
    except ValueError:
        a.stop = (0.0, 0)
    if len(parts) > 2 or not a.stop[0] > 0.0 or a.stop[1] < 1:
        ap.error("--stop takes TOL > 0 and optionally MIN >= 1 as TOL[,MIN]")
    if a.modes is None:
        a.modes = ["cold_until", "warm_until", "refresh_until", "warm_refresh_until"]
if (a.drift is not None or a.modes is not None or a.widen is not None or a.widen_primary is not None or a.refresh is not None
        or a.refresh_f32 or a.until_f32) and not a.device_channel:
    ap.error("--drift, --modes, --widen, --widen-primary, --refresh, --refresh-f32 and --until-f32 need --device-channel")
if a.refresh is not None:
    try:
        a.refresh = tuple(int(x) for x in a.refresh.split(","))
    except ValueError:
        a.refresh = ()
    if len(a.refresh) != 2 or min(a.refresh) < 0:
        ap.error("--refresh takes two integers >= 0 as START,PERIOD")
if a.widen is not None:
    try:
        a.widen = tuple(int(x) for x in a.widen.split(","))
    except ValueError:
        a.widen = ()
    if len(a.widen) != 2 or min(a.widen) < 0:
        ap.error("--widen takes two radii >= 0 as WR,WT")

p = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, snr_db=a.snr_db) if a.small else SweepParams(Nt=64, Nr=64, L=8, T=64, Mr=8, snr_db=a.snr_db)


def emit(res):
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if a.device_channel:
    from jstsp19_amd.montecarlo import run_tracking
    kw = {} if a.modes is None else {"modes": tuple(a.modes)}
    if a.widen is not None:
        kw["widen"] = a.widen
    if a.widen_primary is not None:
        kw["widen_primary"] = a.widen_primary
    if a.refresh is not None:
        kw["refresh"] = a.refresh
    if a.refresh_f32:
        kw["refresh_f32"] = True
    if a.stop is not None:
        kw["stop"] = a.stop
    if a.until_f32:
        kw["until_f32"] = True
    if a.refit is not None:
        kw["refit"] = a.refit
    emit(run_tracking(p, a.seqs, a.frames, a.corr, imax=a.imax, cold_imax=a.cold_imax, precision=a.precision, batch=a.seqs,
                      seed=a.seed, sweep_idx=a.sweep_idx, device=torch.device("cuda:0"), drift=a.drift, **kw))
    sys.exit(0)

N, M, Gr, G2 = p.solver_shape
nm, g = N * M, Gr * G2
dev = torch.device("cuda:0")
rng = np.random.default_rng(a.seed)
cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)

# fixed geometry per sequence (wideband_mmwave_channel.m:20-24, :42-62): half-wavelength uniform linear arrays, the angles of
# all taps those of tap 1, Laplacian around broadside
Np = p.clusters * p.rays
beta = 1.0 / (1.0 - np.exp(-np.sqrt(2.0) * np.pi / 50.0))
lap = lambda u: beta * (np.exp(-np.sqrt(2.0) / 50.0 * np.pi) - np.cosh(u))
steer = lambda n, phi: np.exp(1j * np.pi * np.arange(n)[:, None] * np.sin(phi)[:, None, :])                   # (seqs, n, Np)
Ar, At = steer(p.Nr, lap(rng.random((a.seqs, Np)))), steer(p.Nt, lap(rng.random((a.seqs, Np))))
wgt = (p.clusters - np.arange(Np) // p.rays) / np.sqrt(Np)                                                   # :29, :33
gain = cn(a.seqs, p.L, Np)


def channel(gn):
    """(seqs, Nr, Nt, L): H(:, :, l) = A_r diag(g_l w / sqrt(Np)) A_t^H"""
    return np.einsum("srp,slp,stp->srtl", Ar, gn * wgt, At.conj())


f64 = a.precision == "f64"
wide = (lambda x: J.colmajor(x.to(torch.complex128))) if f64 else (lambda x: x)
solve = J.proposed_algorithm_resume_f64 if f64 else J.proposed_algorithm_resume
score = J.nmse_spectral_f64 if f64 else J.nmse_spectral
modes = [("cold", i) for i in sorted(set(a.imax + [a.cold_imax]))] + [(m, i) for m in ("warm", "warm_vs") for i in a.imax]
err = {k: [] for k in modes}
secs = {k: 0.0 for k in modes}
state = {}
for f in range(a.frames):
    if f:
        gain = a.corr * gain + np.sqrt(1.0 - a.corr ** 2) * cn(a.seqs, p.L, Np)
    inp = build_trials(p, 0, a.seqs, seed=a.seed, sweep_idx=f, device=dev, channel=channel(gain), channel_normalize="asis")
    args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)) if f64 else inp["Omega"], wide(inp["A"]), wide(inp["B"]))
    prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
    zb = wide(inp["Zbar"])
    for k in modes:
        mode, imax = k
        st = state.get(k) if mode.startswith("warm") else None
        if st is not None and mode == "warm_vs":
            st = st.clone()
            st[:, :4 * nm] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S, _, _, out = solve(*args, imax, *prm, want_ce=False, state=st, return_state=mode.startswith("warm"))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if mode.startswith("warm"):
            state[k] = out
        if f:
            secs[k] += dt
            err[k].append(torch.as_tensor(score(S, zb)).double().cpu().numpy())

def summary(m, i):
    e = np.stack(err[(m, i)])                                   # (scored frames, seqs)
    per_seq = e.mean(axis=0)
    return {"mode": m, "Imax": i, "mean_nmse": float(e.mean()), "sem_over_seqs": float(per_seq.std(ddof=1) / np.sqrt(len(per_seq))) if len(per_seq) > 1 else None,
            "median_nmse": float(np.median(e)), "mean_nmse_by_frame": [float(x) for x in e.mean(axis=1)],
            "estimates_per_s": a.seqs * (a.frames - 1) / secs[(m, i)]}


res = {"tool": "run_tracking", "precision": a.precision, "shape": [N, M, Gr, G2], "frames": a.frames, "seqs": a.seqs, "corr": a.corr,
       "clusters": p.clusters, "rays": p.rays, "snr_db": a.snr_db, "seed": a.seed, "scored_frames": list(range(1, a.frames)),
       "cold_imax": a.cold_imax, "results": [summary(m, i) for m, i in modes if err[(m, i)]]}
emit(res)
