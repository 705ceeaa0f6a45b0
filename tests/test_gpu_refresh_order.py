"""The recomputation of R v (every 4th iteration) behind a fused pass is issued on a side stream as soon as v is final, its first
factor P1 = G_A,hi V + (G_A,lo V) is one launch (csrc/gradstep.hip: grad_refresh_p1_kernel), and the next pass's operand maxima
are zeroed by step_v instead of a memset.  None of this changes a rounding: with JSTSP_FUSED=1 (default) S, Y and
convergence_error are BIT-identical to JSTSP_FUSED=2, which runs the parent's launches in the parent's order (the recomputation
inline on the main stream as three launches, the memset).  A missing event would show as bits that differ from =2 or from run
to run.

Shapes as in test_gpu_gradstep.py, the smallest that reach the window path (Nr = Nt = 64: N = Gr = 64, G2 = 64 L in {128, 512},
M = 128; JSTSP_H2=2).  Imax = 9: early recomputations for iterations 4 and 8, the second one consumed by the last iteration (which
has no fused Res / P1 launch); Imax = 5: the only early one is the last iteration's; Imax = 4: none (iteration 0 is inline).

The first-factor kernel has no entry point of its own in the C ABI: it is checked through the solver, where at =1 it forms
every recomputation of R v (iteration 0 inline, the others early) and at =2 the two cgemm launches do."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _solve(inp, B, env, imax, angles=False, want_ce=True):
    import torch
    import jstsp19_amd as J
    env = dict(env, JSTSP_H2="2")
    for k, v in env.items():
        os.environ[k] = v
    try:
        hp = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
        if angles:
            r = J.proposed_algorithm_angles(inp["subY"], inp["Omega"], inp["indx_S"], inp["A"], B, imax, *hp, "approximate", None,
                                            want_ce=want_ce)
        else:
            r = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], B, imax, *hp, "approximate", want_ce=want_ce)
        torch.cuda.synchronize()
        ctx = J.default_context(0)
        gt, nfb = ctx.last_dictionary_block(), ctx.last_fused_fallbacks()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return [None if x is None else x.cpu().numpy() for x in r], gt, nfb


def _same(r1, r0):
    assert len(r1) == len(r0)
    for a, b in zip(r1, r0):
        if a is None or b is None:
            assert a is None and b is None
            continue
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), float(np.nanmax(np.abs(a - b)))


@functools.lru_cache(maxsize=None)
def _inputs(L, batch, shared):
    from jstsp19_amd.system_model import SweepParams, build_trials
    p = SweepParams(Nt=64, Nr=64, L=L, T=2, Mr=8, snr_db=5.0)
    assert p.solver_shape == (64, 128, 64, 64 * L)
    inp = build_trials(p, 0, batch, seed=140 + 8 * L + batch, shared_pilots=shared)
    return inp, (inp["B"][0] if shared else inp["B"])


@pytest.mark.parametrize("imax", [9, 5, 4])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("L", [2, 8])            # G2 = 128, 512
def test_early_refresh_is_bit_identical(L, batch, imax):
    """Three outputs, per-trial and shared pilots, proposed_algorithm and proposed_algorithm_angles: every output bit for bit, on
    the window path (block height 64, no re-solve)."""
    for shared in (False, True):
        inp, B = _inputs(L, batch, shared)
        for angles in (False, True):
            r0, gt0, n0 = _solve(inp, B, {"JSTSP_FUSED": "2"}, imax, angles)
            r1, gt1, n1 = _solve(inp, B, {"JSTSP_FUSED": "1"}, imax, angles)
            assert gt0 == 64 and gt1 == 64 and n0 == 0 and n1 == 0
            assert r0[2] is not None and r0[2].size == batch * 3 * imax and np.all(np.isfinite(r0[0]))
            assert np.max(np.abs(r0[0])) > 0
            _same(r1, r0)


@pytest.mark.parametrize("shared", [False, True])
def test_default_runs_repeat_their_bits(shared):
    """Three consecutive default runs (the early recomputation on its side stream) return the same bytes, those of =2."""
    inp, B = _inputs(8, 3, shared)
    r0, gt0, n0 = _solve(inp, B, {"JSTSP_FUSED": "2"}, 9)
    assert gt0 == 64 and n0 == 0
    for _ in range(3):
        rd, gtd, nd = _solve(inp, B, {}, 9)
        assert gtd == 64 and nd == 0
        _same(rd, r0)


@pytest.mark.parametrize("angles", [False, True])
@pytest.mark.parametrize("L", [2, 8])
def test_two_output_call_is_bit_identical(L, angles):
    """Without convergence_error the recomputation stays inline (with the one-launch first factor) and step_v zeroes the maxima:
    S and Y bit for bit."""
    for shared in (False, True):
        inp, B = _inputs(L, 3, shared)
        r0, gt0, n0 = _solve(inp, B, {"JSTSP_FUSED": "2"}, 9, angles, want_ce=False)
        r1, gt1, n1 = _solve(inp, B, {"JSTSP_FUSED": "1"}, 9, angles, want_ce=False)
        assert gt0 == 64 and gt1 == 64 and n0 == 0 and n1 == 0
        assert r0[2] is None and r1[2] is None
        _same(r1, r0)
