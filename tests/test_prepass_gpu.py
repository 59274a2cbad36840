"""The visibility pre-pass on the device against its exact reference (tests/prepass_ref.py): node_dist bit for bit, the visible sets as arrays.

Every scene's deciding points are known (tests/test_prepass_ref.py holds that on the CPU): one witness per group of nodes, written at the cloud indices
where a kernel goes wrong -- 0, 63, 64, 255, 256, the ragged last wave, and both sides of the 262 144-point border behind which the grid-stride loop
of k_node_min_dist / k_node_min_dist_direct takes its second trip.  Each case runs tdlo_visibility_prepass on the one-launch route and on the copy
route (TDLO_DIRECT_UPLOAD=0) and asserts which one ran (tdlo_debug_route_count 22 / 23); one case rides in k_cloud_team (route count 8)."""
import os

import numpy as np
import pytest

import prepass_ref as R

pytestmark = pytest.mark.gpu
NMAX = R.TRIP + 512


def make_ctx(env=None, **kw):
    from trackdlo_amd import binding as B
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = str(v)
        return B.Context(device=0, timing=False, **kw)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@pytest.fixture(scope="module")
def direct_ctx():
    ctx = make_ctx({"TDLO_DIRECT_UPLOAD": None}, max_points=NMAX, max_nodes=1024)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def copy_ctx():
    ctx = make_ctx({"TDLO_DIRECT_UPLOAD": 0}, max_points=NMAX, max_nodes=1024)
    yield ctx
    ctx.close()


def run(ctx, route, X, Y, thr, d_vis, coord, resident=False):
    """One tdlo_visibility_prepass on `ctx`; asserts that it took `route` (0: k_node_min_dist_direct, 1: copies + k_node_min_dist) and nothing else."""
    if not resident:
        ctx.set_cloud(0, X)
    before = ctx.prepass_route_counts(); rides = ctx.cloud_vis_rides()
    out = ctx.visibility_prepass(0, Y, thr, d_vis, coord)
    after = ctx.prepass_route_counts()
    assert [a - b for a, b in zip(after, before)] == [1 - route, route] and ctx.cloud_vis_rides() == rides, (route, before, after)
    return out


def check(got, want, label):
    for g, w, what in zip(got, want, ("node_dist", "visible_nodes", "visible_nodes_extended")):
        assert g.dtype == w.dtype and g.shape == w.shape, (label, what, g.shape, w.shape)
        bad = np.nonzero(g.view(np.uint64) != w.view(np.uint64))[0] if what == "node_dist" else np.nonzero(g != w)[0]
        assert len(bad) == 0, f"{label}: {what} differs at {bad[:8].tolist()}: kernel {g[bad[:4]]!r}, reference {w[bad[:4]]!r}"


@pytest.mark.parametrize("N,M", R.cases(), ids=lambda v: str(v))
def test_bit_for_bit_on_both_routes(direct_ctx, copy_ctx, N, M):
    X, Y, coord, idx, r, (d2, _) = R.case_ref(N, M)
    thr = float(np.median(r))                                   # about half of the nodes visible: the gap fill has gaps to fill
    want = R.threshold_and_fill(d2, thr, 0.06, coord)
    assert M == 1 or 0 < len(want[1]) < M
    for route, ctx in ((0, direct_ctx), (1, copy_ctx)):
        check(run(ctx, route, X, Y, thr, 0.06, coord), want, f"N{N}-M{M}-route{route}")


def test_rides_in_the_cloud_kernel(direct_ctx):
    """tdlo_depth_to_cloud_visibility with up to 64 nodes: the pre-pass rides in k_cloud_team; held to the reference on the cloud that call left resident."""
    from trackdlo_amd import synth
    depth, mask, cam, Y0 = synth.depth_scene(30, config=9, frame=2)
    coord = synth.geodesic_coord(Y0)
    d, m = direct_ctx.image_buffers(*depth.shape)
    d[:] = depth; m[:] = mask
    rides = direct_ctx.cloud_vis_rides(); before = direct_ctx.prepass_route_counts()
    dist, vis, ext, n, _ = direct_ctx.depth_to_cloud_visibility(0, d, m, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.008, Y0, 0.008, 0.06, coord)
    assert direct_ctx.cloud_vis_rides() == rides + 1 and direct_ctx.prepass_route_counts() == before
    X = direct_ctx.get_cloud(0)
    assert len(X) == n > 64
    want = R.prepass(X, Y0, 0.008, 0.06, coord)
    assert 0 < len(want[1])
    check((dist, vis, ext), want, "ride-along")
    check(run(direct_ctx, 0, None, Y0, 0.008, 0.06, coord, resident=True), want, "ride-along, then the call of its own")


@pytest.mark.parametrize("route", [0, 1], ids=["one-launch", "copies"])
def test_nothing_of_an_earlier_call_survives(direct_ctx, copy_ctx, route):
    """M = 300 with near witnesses, M = 45 whose nodes are all far (6 .. 7 cm), M = 300 again, every call twice: the minima are re-armed."""
    ctx = (direct_ctx, copy_ctx)[route]
    N = 30000
    a = R.case_ref(N, 300)
    b = R.case_ref(N, 45, seed=5, far_nodes=tuple(range(45)))
    assert np.sqrt(b[5][0]).min() > 0.05 and np.sqrt(a[5][0][:45]).max() <= 0.02
    for k, (X, Y, coord, idx, r, (d2, _)) in enumerate((a, b, a)):
        want = R.threshold_and_fill(d2, 0.0655, 0.06, coord)
        first = run(ctx, route, X, Y, 0.0655, 0.06, coord)
        check(first, want, f"call {k}")
        check(run(ctx, route, X, Y, 0.0655, 0.06, coord, resident=True), first, f"call {k} repeated")


@pytest.mark.parametrize("route", [0, 1], ids=["one-launch", "copies"])
def test_threshold_tie(direct_ctx, copy_ctx, route):
    """d^2 exact on a 2^-26 m grid: visibility_threshold = d takes the node in, one ulp below leaves it out, one ulp above takes it in (:316, <=)."""
    ctx = (direct_ctx, copy_ctx)[route]
    X, Y, coord, d = R.tie_scene()
    for thr, inside in ((d, True), (np.nextafter(d, 0.0), False), (np.nextafter(d, 1.0), True)):
        got = run(ctx, route, X, Y, thr, 0.0, coord)
        check(got, R.prepass(X, Y, thr, 0.0, coord), f"thr {thr!r}")
        assert got[0][1] == d and (1 in got[1]) == inside


def test_gap_fill_tie_and_degenerate_sets(direct_ctx):
    """d_vis equal to the coordinate difference across an occluded run fills it, one ulp below does not (:351-359, <=); n_vis = 0 gives both counts 0
    and TDLO_OK; n_vis = 1; M = 1 visible and invisible."""
    X, Y, coord, idx, r = R.scene(257, 8, seed=2, far_nodes=(2, 3))
    gap = abs(coord[4] - coord[1])
    for d_vis, ext in ((gap, list(range(8))), (np.nextafter(gap, 0.0), [0, 1, 4, 5, 6, 7])):
        got = run(direct_ctx, 0, X, Y, 0.03, d_vis, coord)
        check(got, R.prepass(X, Y, 0.03, d_vis, coord), f"d_vis {d_vis!r}")
        assert got[1].tolist() == [0, 1, 4, 5, 6, 7] and got[2].tolist() == ext
    got = run(direct_ctx, 0, X, Y, 0.0005, 0.06, coord)                       # nothing visible
    assert len(got[1]) == 0 and len(got[2]) == 0
    check(got, R.prepass(X, Y, 0.0005, 0.06, coord), "n_vis = 0")
    m = int(np.argmin(r))
    got = run(direct_ctx, 0, X, Y, float(np.sort(r)[:2].mean()), 0.06, coord)  # one node visible
    assert got[1].tolist() == [m] and got[2].tolist() == [m]
    X, Y, coord, idx, r, (d2, _) = R.case_ref(65, 1)
    for thr, n in ((float(r[0]) * 1.5, 1), (float(r[0]) * 0.5, 0)):
        got = run(direct_ctx, 0, X, Y, thr, 0.06, coord)
        check(got, R.threshold_and_fill(d2, thr, 0.06, coord), f"M = 1, n_vis = {n}")
        assert len(got[1]) == n and len(got[2]) == n


@pytest.mark.parametrize("N,M", [(257, 45), (R.TRIP + 311, 8)], ids=lambda v: str(v))
def test_non_finite_points_change_nothing(direct_ctx, copy_ctx, N, M):
    """NaN and +-inf coordinates written at the index list give the results of the cloud without those points: fmin never lets a NaN win."""
    X, Y, coord, idx, r, (d2, _) = R.case_ref(N, M, seed=8)
    X2, bad = R.with_non_finite(X)
    thr = float(np.median(r))
    want = R.threshold_and_fill(d2, thr, 0.06, coord)
    for route, ctx in ((0, direct_ctx), (1, copy_ctx)):
        check(run(ctx, route, X2, Y, thr, 0.06, coord), want, f"non-finite N{N} route{route}")


@pytest.mark.parametrize("route", [0, 1], ids=["one-launch", "copies"])
def test_a_cloud_without_a_finite_point_reports_the_reference_start_value(direct_ctx, copy_ctx, route):
    """trackdlo_node.cpp:261: shortest_dist starts at 100000 and stays there; nothing is visible; the context goes on working."""
    ctx = (direct_ctx, copy_ctx)[route]
    X, Y, coord, idx, r, (d2, _) = R.case_ref(257, 45)
    X2, bad = R.with_non_finite(X)
    got = run(ctx, route, X2[bad], Y, 0.008, 0.06, coord)
    assert (got[0] == 100000.0).all() and len(got[1]) == 0 and len(got[2]) == 0
    check(got, R.prepass(X2[bad], Y, 0.008, 0.06, coord), "no finite point")
    check(run(ctx, route, X, Y, 0.008, 0.06, coord), R.threshold_and_fill(d2, 0.008, 0.06, coord), "the next call")
