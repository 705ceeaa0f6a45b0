"""The fused launches of the gradient step between two passes (csrc/gradstep.hip) remove launches and HBM round trips and change
no rounding: with JSTSP_FUSED=1 (default) S, Y and convergence_error are BIT-identical to JSTSP_FUSED=2, which runs the pass with the
separate launches.  The fused launches are taken only in the window behind a pass of the block-64 window kernel, with
convergence_error and not in the last iteration, so the shapes are the smallest ones that reach that path (Nr = Nt = 64:
N = Gr = 64, G2 = 64 L, M = 64 T; JSTSP_H2=2 because frames this short would not take the split-f16 path otherwise).  Imax = 6:
the recomputations of R v at iterations 0 and 4, the recurrence between them, and the unfused first and last iterations."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IMAX = 6


def _solve(inp, B, env, angles=False, want_ce=True):
    import torch
    import jstsp19_amd as J
    env = dict(env, JSTSP_H2="2")
    for k, v in env.items():
        os.environ[k] = v
    try:
        hp = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
        if angles:
            r = J.proposed_algorithm_angles(inp["subY"], inp["Omega"], inp["indx_S"], inp["A"], B, IMAX, *hp, "approximate", None,
                                            want_ce=want_ce)
        else:
            r = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], B, IMAX, *hp, "approximate", want_ce=want_ce)
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


def _inputs(L, T, batch, shared):
    from jstsp19_amd.system_model import SweepParams, build_trials
    p = SweepParams(Nt=64, Nr=64, L=L, T=T, Mr=8, snr_db=5.0)
    assert p.solver_shape == (64, 64 * T, 64, 64 * L)
    inp = build_trials(p, 0, batch, seed=40 + 8 * L + T + batch, shared_pilots=shared)
    return inp, (inp["B"][0] if shared else inp["B"])


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("T", [2, 4])            # M = 128, 256
@pytest.mark.parametrize("L", [2, 4, 8])         # G2 = 128, 256, 512
def test_fused_gradient_step_is_bit_identical(L, T, batch):
    """Three outputs, per-trial and shared pilots, proposed_algorithm and proposed_algorithm_angles (the rank mask of the soft
    threshold): every output bit for bit, and the window path (block height 64, no re-solve) really was taken."""
    for shared in (False, True):
        inp, B = _inputs(L, T, batch, shared)
        for angles in (False, True):
            r0, gt0, n0 = _solve(inp, B, {"JSTSP_FUSED": "2"}, angles)
            r1, gt1, n1 = _solve(inp, B, {"JSTSP_FUSED": "1"}, angles)
            assert gt0 == 64 and gt1 == 64 and n0 == 0 and n1 == 0
            assert r0[2] is not None and r0[2].size == batch * 3 * IMAX and np.all(np.isfinite(r0[0]))
            assert np.max(np.abs(r0[0])) > 0
            _same(r1, r0)


def test_default_is_the_fused_path_and_takes_the_window_kernel():
    """Unset = 1: the default run equals JSTSP_FUSED=1 and =2, and default_context().last_dictionary_block() reports the
    block-64 window path - without it the comparisons of this file would compare one path with itself."""
    import jstsp19_amd as J
    inp, B = _inputs(4, 4, 3, False)
    rd, gtd, nd = _solve(inp, B, {})
    assert J.default_context(0).last_dictionary_block() == 64 and gtd == 64 and nd == 0
    r1, _, _ = _solve(inp, B, {"JSTSP_FUSED": "1"})
    r0, _, _ = _solve(inp, B, {"JSTSP_FUSED": "2"})
    _same(rd, r1)
    _same(rd, r0)
    # the gradient step does reach the outputs: another input gives other bits
    inp2, B2 = _inputs(4, 4, 3, True)
    r2, _, _ = _solve(inp2, B2, {})
    assert r2[0].tobytes() != rd[0].tobytes()


@pytest.mark.parametrize("angles", [False, True])
def test_two_output_call_is_unchanged(angles):
    """Without convergence_error the window has no split eigen-decomposition and the fused launches are not taken: equal by
    construction, and equal in S and Y to nothing else than itself under either setting."""
    inp, B = _inputs(8, 4, 3, False)
    r0, gt0, _ = _solve(inp, B, {"JSTSP_FUSED": "2"}, angles, want_ce=False)
    r1, gt1, _ = _solve(inp, B, {"JSTSP_FUSED": "1"}, angles, want_ce=False)
    assert gt0 == 64 and gt1 == 64
    assert r0[2] is None and r1[2] is None
    _same(r1, r0)
