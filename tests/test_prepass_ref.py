"""The exact reference of the visibility pre-pass (tests/prepass_ref.py) and its scenes, checked on the CPU: the fused step is correctly rounded,
the candidate search loses nothing against the brute-force exact minimum, the fp64 oracle agrees to its own rounding, and -- for every scene of the
GPU matrix -- every node's result is decided by its witness: without it the node's distance changes by more than 1 cm."""
from fractions import Fraction

import numpy as np
import pytest

import prepass_ref as R


def test_fma_is_correctly_rounded():
    rng = np.random.default_rng(1)
    for _ in range(300):
        a, b = rng.normal(size=2)
        c = -a * b * (1.0 + rng.normal() * 1e-15)                  # heavy cancellation: a plain product would lose every digit
        got = R.fma(a, b, c)
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        err = abs(Fraction(got) - exact)
        assert err <= abs(Fraction(np.nextafter(got, np.inf)) - exact) and err <= abs(Fraction(np.nextafter(got, -np.inf)) - exact)
    a = 1.0 + 2.0 ** -30
    assert R.fma(a, a, -(a * a)) == 2.0 ** -60 and a * a - a * a == 0.0


def test_fused_and_plain_distances_differ_somewhere_but_by_less_than_4_ulps():
    X, Y, _, _, _ = R.scene(257, 45)
    differ = 0
    for y in Y[:8]:
        for x in X:
            f = R.d2_fused(y, x); p = float(R._plain_d2(x[None, :], y)[0])
            differ += f != p
            assert abs(f - p) < 4 * np.spacing(f)
    assert differ > 100                                             # the scenes can tell a plain product from a fused one


def test_candidate_search_equals_the_brute_force_exact_minimum():
    X, Y, _, _, _ = R.scene(257, 65, seed=3)
    X = np.array(X); X[5] = X[R.index_list(257)[0]]                 # an exact duplicate of a witness: the first index wins
    d2, arg = R.min_d2(X, Y)
    for m, y in enumerate(Y):
        allv = [R.d2_fused(y, x) for x in X]
        assert d2[m] == min(allv) and arg[m] == int(np.argmin(allv))


@pytest.mark.parametrize("N,M", R.cases(), ids=lambda v: str(v))
def test_every_witness_decides_its_nodes(N, M):
    X, Y, coord, idx, r, (d2, arg) = R.case_ref(N, M)
    K = len(idx)
    near, d1, d2nd = R.nearest_two(X, Y)
    want = np.asarray(idx)[np.arange(M) % K]
    np.testing.assert_array_equal(arg, want)                        # the exact minimum is attained at the witness ...
    np.testing.assert_array_equal(near, want)
    assert len(set(r.tolist())) == M and r.min() >= 0.001 and r.max() <= 0.02
    np.testing.assert_allclose(np.sqrt(d2), r, rtol=1e-9)           # ... at the node's own distance ...
    assert (d2nd - d1).min() > 0.01, (d2nd - d1).min()             # ... and removing it moves node_dist by more than 1 cm
    far = np.ones(N, dtype=bool); far[idx] = False
    if far.any():
        assert min(np.sqrt(R._plain_d2(X[far], y).min()) for y in Y[:: max(1, M // 16)]) >= 0.05
    assert set(R.index_list(N)) >= {i for i in (0, 63, 64, 255, 256, N - 1, N - 2) if 0 <= i < N}
    if N > R.TRIP:
        assert {R.TRIP - 1, R.TRIP} <= set(idx) and max(idx) // 64 == (N - 1) // 64


@pytest.mark.parametrize("N,M", [(257, 45), (30000, 64), (37, 300)])
def test_reference_against_the_fp64_oracle(oracle, N, M):
    X, Y, coord, idx, r, (d2, _) = R.case_ref(N, M)
    thr = float(np.median(r))
    dist, vis, ext = R.threshold_and_fill(d2, thr, 0.06, coord)
    do, viso, exto = oracle.visibility_prepass(X, Y, thr, 0.06, coord)
    np.testing.assert_allclose(dist, do, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(vis, viso); np.testing.assert_array_equal(ext, exto)
    assert 0 < len(vis) < M or M == 1


def test_threshold_tie_on_the_reference():
    X, Y, coord, d = R.tie_scene()
    assert 0.004 < d < 0.008 and R.min_d2(X, Y)[1][1] == R.index_list(len(X))[1]
    for thr, inside in ((d, True), (np.nextafter(d, 0.0), False), (np.nextafter(d, 1.0), True)):
        _, vis, _ = R.prepass(X, Y, thr, 0.0, coord)
        assert (1 in vis) == inside


def test_gap_fill_tie_and_degenerate_sets_on_the_reference():
    coord = np.array([0.0, 0.013, 0.029, 0.041, 0.0577, 0.07])
    vis = np.array([0, 1, 4, 5], dtype=np.int32)
    gap = abs(coord[4] - coord[1])
    np.testing.assert_array_equal(R.fill_gaps(vis, coord, gap), [0, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(R.fill_gaps(vis, coord, np.nextafter(gap, 0.0)), [0, 1, 4, 5])
    assert len(R.fill_gaps(np.zeros(0, dtype=np.int32), coord, 1.0)) == 0
    np.testing.assert_array_equal(R.fill_gaps(np.array([3]), coord, 1.0), [3])


def test_non_finite_points_never_win_and_an_all_non_finite_cloud_reports_the_start_value(oracle):
    X, Y, coord, idx, r, (d2, _) = R.case_ref(257, 45)
    X2, bad = R.with_non_finite(X)
    assert len(X2) == len(X) + len(bad) and not np.isfinite(X2[bad]).all(axis=1).any() and set(bad) >= set(R.index_list(len(X2))) and len(bad) == 10
    np.testing.assert_array_equal(R.min_d2(X2, Y)[0], d2)
    dist, vis, ext = R.prepass(X2[bad], Y, 0.008, 0.06, coord)
    assert (dist == R.START).all() and len(vis) == 0 and len(ext) == 0
    do, viso, _ = oracle.visibility_prepass(X2[bad], Y, 0.008, 0.06, coord)
    np.testing.assert_array_equal(do, dist); assert len(viso) == 0
