"""The float64 helpers of the drifting-channel and support-order tests (tests/drift_ref.py) against the oracle and against
literal restatements - CPU only."""
import numpy as np
import pytest

import drift_ref as D
from oracle import system_model as osm

# entries whose keys tie exactly: |3+4j|^2 == |5|^2 == 25, |1|^2 == |1j|^2 == |-1|^2, and 1e-30, whose square is 0 in fp32 only
TIE_VALUES = np.array([0, 1, 1j, -1, 3 + 4j, 5, 1e-30], dtype=complex)


def tie_trials(seed=3, shape=(5, 7), count=3):
    """``count`` trials of ``shape`` drawn from TIE_VALUES, then an all-zero trial, then one with a NaN and an Inf."""
    rng = np.random.default_rng(seed)
    t = [TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=shape)] for _ in range(count)]
    t.append(np.zeros(shape, complex))
    x = TIE_VALUES[rng.integers(0, TIE_VALUES.size, size=shape)]
    x[1, 2] = complex(np.nan, 1.0)
    x[3, 0] = complex(2.0, -np.inf)
    t.append(x)
    return np.stack(t)


def continuous_trial(seed=7, shape=(64, 512)):
    """A random trial without ties: uniform phases, and squared magnitudes 1 + (i + U_i/2)/n, U_i ~ U(0, 1), in random positions -
    continuous, but stratified so that neighbouring keys are at least 1/(2n) apart (2^-16 at n = 32768: 64 ulp of fp32).  Plain
    normal entries cannot serve in fp32: 32768 keys spread over a few binades of 2^23 values each leave about 1 gap in 200
    below 4 ulp, whatever the seed."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    m2 = 1.0 + (np.arange(n) + 0.5 * rng.random(n)) / n
    z = np.sqrt(m2) * np.exp(2j * np.pi * rng.random(n))
    return z[rng.permutation(n)].reshape(shape)


def keys_are_separated(S, dtype, ulps=4):
    """Neighbouring sorted keys are equal or more than ``ulps`` ulp apart: a last-bit difference in how x*x + y*y is rounded
    (an fma contraction) cannot reorder them."""
    k = np.sort(D.support_key(S, dtype).astype(dtype))
    d = np.diff(k)
    return bool(np.all((d == 0) | (d > ulps * np.spacing(k[1:]))))


def _literal_order(S, dtype):
    key = D.support_key(S, dtype)
    rank = lambda i: (0, 0.0) if np.isnan(key[i]) else (1, -float(key[i]))
    return np.array(sorted(range(key.size), key=lambda i: (rank(i), i)), dtype=np.int32) + 1


def test_walk_is_the_cumulative_sum_times_drift():
    z = np.random.default_rng(0).standard_normal((5, 2, 3))
    w = D.walk(z, 0.3)
    assert w.shape == (6, 2, 3) and not w[0].any()
    np.testing.assert_array_equal(w[3], 0.3 * ((z[0] + z[1]) + z[2]))
    np.testing.assert_array_equal(D.walk(z, 0.0), np.zeros((6, 2, 3)))


@pytest.mark.parametrize("clusters,rays,L,Nr,Nt", [(2, 3, 2, 8, 2), (3, 2, 3, 12, 4), (1, 1, 1, 4, 1)])
def test_channel_from_angles_is_the_oracles_channel(clusters, rays, L, Nr, Nt):
    rng = np.random.default_rng(11)
    Np = clusters * rays
    gains = (rng.standard_normal((L, Np)) + 1j * rng.standard_normal((L, Np))) / np.sqrt(2)
    u_r, u_t = rng.random((L, Np)), rng.random((L, Np))
    H = osm.wideband_mmwave_channel(L, Nr, Nt, clusters, rays, Nr, Nt, gains, u_r, u_t)[0]
    got = D.channel_from_angles(gains, osm._laplacian(u_r[0]), osm._laplacian(u_t[0]), clusters, rays, Nr, Nt)
    assert np.max(np.abs(got - H)) <= 1e-14 * max(1.0, np.max(np.abs(H)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_support_order_ref_on_engineered_ties(dtype):
    trials = tie_trials()
    assert D.support_key(np.array([[3 + 4j, 5]]), dtype).tolist() == [25.0, 25.0]
    for t, S in enumerate(trials):
        got = D.support_order_ref(S, dtype)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, _literal_order(S, dtype), err_msg="trial %d" % t)
    n = trials[0].size
    np.testing.assert_array_equal(D.support_order_ref(trials[3], dtype), np.arange(1, n + 1))       # all zero: 1..n
    last = D.support_order_ref(trials[4], dtype)
    assert last[0] == 1 + 1 + 5 * 2 and last[1] == 1 + 3 + 5 * 0                                      # the NaN, then the Inf
    # 1e-30 squares to zero in fp32 and ties with the zeros there; in float64 it stands before them
    S = np.array([[0, 1e-30], [1e-30, 0]], complex)
    assert D.support_order_ref(S, np.float32).tolist() == [1, 2, 3, 4]
    assert D.support_order_ref(S, np.float64).tolist() == [2, 3, 1, 4]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_continuous_trial_has_separated_keys(dtype):
    """The seed of continuous_trial is one for which no two of the 32768 keys are within 4 ulp without being equal: the GPU test
    relies on it."""
    S = continuous_trial()
    assert keys_are_separated(S.astype(np.complex64) if dtype is np.float32 else S, dtype)
    np.testing.assert_array_equal(D.support_order_ref(S[:8, :8], dtype), _literal_order(S[:8, :8], dtype))
