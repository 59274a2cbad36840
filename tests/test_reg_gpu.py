"""`reg` on the device (k_reg_estep / k_reg_mstep, tdlo_reg.hip) against the longdouble reference of tests/reg_ref.py, within the gate derived there
and carried through the iterations on the reference alone; and to 1e-9 against the fp64 oracle.

The matrix (reg_ref.cases, each case held on the CPU by tests/test_reg_ref.py): clouds below one wave, of one point, around the wave and workgroup
sizes; one centroid; odd 3 M (launch_reg pads the partials' offset by one double); max_iter 0 .. 5 and the reference's 50; mu 0 .. 0.99; the E-step's
second and third trip of the grid-stride loop (beyond 65 536 points); both sides of the 64 KB border of the dynamic LDS (M = 356 | 357) and its
end (M = 890).  Every test prints its worst ratio to the gate."""
import numpy as np
import pytest

import reg_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from trackdlo_amd import binding as B
    c = B.Context(device=0, max_points=1 << 16, max_nodes=64, timing=False)
    yield c
    c.close()


def held(ctx, c, label=None, pts=True):
    """One tdlo_reg of case c on ctx: within the gate of the reference and within 1e-9 of the oracle.  Returns (Y, sigma2, worst ratios)."""
    from oracle import ref_cpu
    X, ref = R.case_ref(c)
    Yg, sg = ctx.reg(X if pts else None, c["M"], mu=c["mu"], max_iter=c["it"])
    qy, qs = R.ratio(Yg, sg, ref)
    label = label or R.cid(c)
    print(f"{label}: Y {qy:.3g}, sigma2 {qs:.3g} of the gate")
    assert qy <= 1.0 and qs <= 1.0, f"{label}: Y off by {qy:.3g} gates, sigma2 by {qs:.3g} gates"
    Yo, so = ref_cpu.reg(X, c["M"], mu=c["mu"], max_iter=c["it"])
    np.testing.assert_allclose(Yg, Yo, rtol=0, atol=1e-9)
    assert abs(sg - so) <= 1e-9 * so
    if c["it"] == 0:
        assert np.array_equal(Yg, R.start_nodes(c["M"]))
    return Yg, sg, (qy, qs)


@pytest.mark.parametrize("c", R.small_cases() + [R.LONG_CASE], ids=R.cid)
def test_small_clouds(ctx, c):
    held(ctx, c)


@pytest.mark.parametrize("c", R.trip_cases(), ids=R.cid)
def test_second_trip_of_the_grid_stride_loop(ctx, c):
    """More than 65 536 points: 256 workgroups take a second (and at 131 137 points a third, ragged) trip; the resident-cloud form gives the same bits."""
    assert R.geometry(c["N"])[1] == (1 if c["N"] == R.TRIP else -(-c["N"] // R.TRIP))
    Yg, sg, _ = held(ctx, c)
    Yr, sr = ctx.reg(None, c["M"], mu=c["mu"], max_iter=c["it"])
    assert np.array_equal(Yr, Yg) and sr == sg


@pytest.mark.parametrize("c", R.lds_cases(), ids=R.cid)
def test_lds_border_values(ctx, c):
    """M = 356: the last size below 64 KB of dynamic LDS; 357: the first that needs hipFuncSetAttribute; 890: reg_max_nodes().  Values, not shapes."""
    held(ctx, c)


def test_one_context_across_shapes():
    """M = 890 -> 5 -> 357 and N large -> small -> large on one fresh context: the workspace grows and is reused, the large-LDS attribute is set once
    and does not disturb the small case; the repeated cases give the bits of their first run."""
    from trackdlo_amd import binding as B
    c = B.Context(device=0, max_points=4096, max_nodes=64, timing=False)
    try:
        seq = [dict(N=2000, M=890, mu=0.05, it=2), dict(N=257, M=5, mu=0.05, it=2), dict(N=2000, M=357, mu=0.05, it=2),
               dict(N=R.TRIP + 321, M=5, mu=0.05, it=2), dict(N=37, M=5, mu=0.0, it=5), dict(N=2 * R.TRIP + 65, M=5, mu=0.05, it=2),
               dict(N=257, M=5, mu=0.05, it=2), dict(N=2000, M=890, mu=0.05, it=2)]
        first = {}
        for k, case in enumerate(seq):
            assert R.cid(case) in {R.cid(x) for x in R.cases()}
            Yg, sg, _ = held(c, case, f"step {k} {R.cid(case)}")
            if R.cid(case) in first:
                assert np.array_equal(first[R.cid(case)][0], Yg) and first[R.cid(case)][1] == sg
            first.setdefault(R.cid(case), (Yg, sg))
    finally:
        c.close()


def test_nan_by_the_reference_own_arithmetic(ctx):
    """N = 1, M = 1, three iterations on a point with power-of-two coordinates: sigma2 reaches 0, then 0 * -inf.  Same NaN mask as the reference; two
    iterations give the point and sigma2 = 0 exactly; the context stays usable."""
    c = R.NAN_CASE
    X = R.nan_cloud()
    r = R.reg(X, c["M"], c["mu"], c["it"])
    Yg, sg = ctx.reg(X, c["M"], mu=c["mu"], max_iter=c["it"])
    assert np.array_equal(np.isnan(Yg), np.isnan(r["Y"].astype(np.float64))) and np.isnan(Yg).all() and np.isnan(sg) and np.isnan(float(r["sigma2"]))
    Y2, s2 = ctx.reg(X, c["M"], mu=c["mu"], max_iter=2)
    assert np.array_equal(Y2, X) and s2 == 0.0
    held(ctx, R.REUSE_CASES[0], "after the NaN run")
