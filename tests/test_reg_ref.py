"""The longdouble reference of `reg` and its derived gate (tests/reg_ref.py), checked on the CPU for every case of the GPU matrix:
(a) an honest fp64 restatement of tdlo_reg.hip lies inside the gate, summed in the kernels' order and in numpy's own order;
(b) removing one point of the cloud moves some centroid or sigma2 by more than 10 gates -- every point of clouds of up to 257 points; of larger
    clouds the points at the indices where a kernel goes wrong (first and last lanes of waves and workgroups, the last two points, both sides of
    the second trip's border) and eight drawn at random;
(c) the reference agrees with the fp64 oracle to 1e-9."""
import numpy as np
import pytest

import reg_ref as R


def removal_indices(N):
    if N <= 257:
        return list(range(N))
    rng = np.random.default_rng(N)
    fixed = [0, 63, 64, 255, 256, N - 1, N - 2, R.TRIP - 1, R.TRIP, R.TRIP + 64, 2 * R.TRIP - 1, 2 * R.TRIP]
    return sorted({i for i in fixed if 0 <= i < N} | set(int(i) for i in rng.integers(0, N, 8)))


@pytest.mark.parametrize("c", R.cases(), ids=R.cid)
def test_gate_holds_an_fp64_restatement_and_sees_one_point(oracle, c):
    X, ref = R.case_ref(c)
    Yb, sb, gy, gs = ref
    N, M = c["N"], c["M"]
    assert np.isfinite(Yb.astype(np.float64)).all() and np.isfinite(float(sb)) and sb > 0
    # (a)
    for order in (True, False):
        Y64, s64 = R.reg_fp64(X, M, c["mu"], c["it"], kernel_order=order)
        qy, qs = R.ratio(Y64, s64, ref)
        assert qy <= 1.0 and qs <= 1.0, (R.cid(c), "kernel order" if order else "plain order", qy, qs)
        print(f"{R.cid(c)} fp64 restatement in {'the kernels' if order else 'plain'} order: Y {qy:.3g}, sigma2 {qs:.3g} of the gate")
    if c["it"] == 0:
        assert np.array_equal(Y64, R.start_nodes(M))
    # (c)
    Yo, so = oracle.reg(X, M, mu=c["mu"], max_iter=c["it"])
    np.testing.assert_allclose(Yo, Yb.astype(np.float64), rtol=0, atol=1e-9)
    assert abs(so - float(sb)) <= 1e-9 * float(sb)
    # (b)
    if N == 1:
        return                                              # (no cloud is left without its only point)
    worst = np.inf
    for n in removal_indices(N):
        Yr, sr = R.reg_fp64(np.delete(X, n, axis=0), M, c["mu"], c["it"], kernel_order=False)
        dy = np.abs(Yr - Y64)
        moved = max(float(np.max(np.where(dy == 0, 0.0, dy / np.where(dy == 0, 1.0, gy)))), abs(sr - s64) / gs)
        worst = min(worst, moved)
    print(f"{R.cid(c)}: removing one point moves the result by at least {worst:.3g} gates")
    assert worst > 10.0, (R.cid(c), "the gate cannot see one point", worst)


def test_matrix_covers_what_it_names():
    cs = R.cases()
    for N in R.NS:
        assert {c["M"] for c in cs if c["N"] == N} >= set(R.MS)
    for key, vals in (("it", R.ITERS), ("mu", R.MUS)):
        assert {c[key] for c in R.small_cases()} == set(vals)
        for M in R.MS:
            assert len({c[key] for c in R.small_cases() if c["M"] == M and c["N"] > 1}) >= 3
    assert [R.geometry(c["N"]) for c in R.trip_cases()] == [(256, 1), (256, 2), (256, 2), (256, 3)]
    lds = lambda M: 8 * (3 * M + 4 * (5 * M + 1))
    assert lds(356) <= 64 * 1024 < lds(357) and lds(890) <= 160 * 1024 < lds(891)
    assert R.LONG_CASE["it"] == 50


def test_nan_by_the_reference_own_arithmetic(oracle):
    c = R.NAN_CASE
    X = R.nan_cloud()
    r = R.reg(X, c["M"], c["mu"], c["it"], keep=True)
    assert r["iters"][2]["sigma2"] == 0 and r["iters"][1]["sigma2"] > 0          # sigma2 reaches 0, then 0 * -inf
    assert np.isnan(r["Y"].astype(np.float64)).all() and np.isnan(float(r["sigma2"]))
    Y64, s64 = R.reg_fp64(X, c["M"], c["mu"], c["it"])
    Yo, so = oracle.reg(X, c["M"], mu=c["mu"], max_iter=c["it"])
    assert np.isnan(Y64).all() and np.isnan(s64) and np.isnan(Yo).all() and np.isnan(so)
    two = R.reg(X, c["M"], c["mu"], 2)
    assert np.array_equal(two["Y"].astype(np.float64), X) and two["sigma2"] == 0


def test_moving_the_sums_moves_the_result():
    """The perturbed runs the gate is built on do perturb: a relative move of 1e-6 of every sum shows in Y and in sigma2."""
    c = dict(N=257, M=5, mu=0.05, it=2)
    X = R.cloud(c["N"], c["M"])
    base = R.reg(X, 5, 0.05, 2)
    rng = np.random.default_rng(3)
    def move(it, s):
        if it < 0:
            return dict(S0=1e-6 * float(s["S0"]))
        if "num" in s:
            return {}
        return {k: 1e-6 * rng.choice([-1.0, 1.0], np.shape(s[k])) * np.abs(s[k].astype(np.float64)) for k in ("P1", "PX", "Q")}
    r = R.reg(X, 5, 0.05, 2, move=move)
    dy = float(np.abs(r["Y"] - base["Y"]).max()); ds = float(abs(r["sigma2"] - base["sigma2"]) / base["sigma2"])
    assert 1e-9 < dy < 1e-4 and 1e-8 < ds < 1e-4, (dy, ds)
