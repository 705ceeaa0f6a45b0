"""The problems of tests/refresh32_problems.py against their own decision rule, without a GPU: tests/test_gpu_refresh32.py compares
the fp32 solver with the float64 restatement only on DECIDED trials (boundary gap > 4 * TOL_S at every iteration under a refreshed
order), so the share it may leave out is bounded here, at Imax = 6:

    policy (2, 0)                       every trial of every problem is decided
    policies (0, 1), (1, 2), (3, 1)     at least 2 of 3 trials per problem

"Problem" is one of the four the helper names - R1, R2 (B per trial, the form the GPU tests run), T, G.  Measured (float64 numpy):
  R1 and R2, shared and per-trial B - (2, 0): 12 of 12 decided, smallest gap 5.9e-5 (asserted below for the shared forms too); the
  four policies together 42 of 48 decided.  The six undecided: R1 per-trial (3, 1) trial 2 at 3.7e-6; R1 shared (0, 1) trial 0 at
  7.4e-6; R2 shared (0, 1) trial 2 at 3.0e-5, (1, 2) trial 0 at 2.8e-5, (3, 1) trials 1 and 2 at 2.7e-5 and 2.0e-5.  So R2 with a
  SHARED B has 2 of 3 undecided at (3, 1): the two-of-three condition holds for the per-trial forms only, and no GPU test compares
  a shared-B problem with the restatement.
  T and G at the committed seed: all 24 (policy, trial) pairs decided, smallest gap 4.14e-5 (T, (1, 2), trial 1)."""
import pytest

import refresh32_problems as Q


@pytest.mark.parametrize("name,shared_B", Q.variants())
def test_the_one_refresh_policy_is_decided_in_every_trial(name, shared_B):
    gaps = [Q.min_gap(name, shared_B, t, 2, 0) for t in range(Q.BATCH)]
    print("refresh32 gaps (2, 0)", name, shared_B, gaps)
    assert all(gp > Q.GAP_MIN for gp in gaps), gaps


@pytest.mark.parametrize("policy", [(0, 1), (1, 2), (3, 1)])
@pytest.mark.parametrize("name,shared_B", [(n, False) for n in Q.NAMES])
def test_the_periodic_policies_are_decided_in_two_of_three_trials(name, shared_B, policy):
    gaps = [Q.min_gap(name, shared_B, t, *policy) for t in range(Q.BATCH)]
    print("refresh32 gaps", policy, name, shared_B, gaps)
    assert sum(gp > Q.GAP_MIN for gp in gaps) >= 2, gaps


def test_the_rounded_block_toeplitz_dictionary_repeats_on_the_bits():
    B = Q.problem("T")["B"]
    assert B.dtype.name == "complex64" and (B[:, 64:, 1:] == B[:, :64, :-1]).all()
    assert not (Q.problem("G")["B"][:, 64:, 1:] == Q.problem("G")["B"][:, :64, :-1]).any()
