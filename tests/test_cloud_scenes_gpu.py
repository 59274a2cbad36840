"""GPU suite for the one-launch depth -> cloud kernels on CONSTRUCTED scenes (tests/cloud_scenes.py; their properties and their power to discriminate
are established on the CPU in tests/test_cloud_scenes_ref.py).  Three contexts: the team of eight workgroups (k_cloud_team, the default), the one finishing
workgroup (k_cloud_fused, TDLO_CLOUD_TEAM=0) and the multi-launch form (TDLO_CLOUD_FUSED=0).  Every scene, on every route, twice: the cloud against
tests/voxel_ref.py BIT FOR BIT (a.view(uint64) == b.view(uint64): the sign of a zero counts), n, n_raw, and the route counters -- taken, passed on or
untouched as the scene says; a team that gave its launch up after its 2 s wait would show as a passed-on count and fails the test."""
import os

import numpy as np
import pytest

import cloud_scenes as S
import prepass_ref

pytestmark = pytest.mark.gpu

ROUTES = ("team", "one", "multi")
SEEN = dict(run=0, tiles=0, kb=0, cases=0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what=None):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).any(axis=1).sum()), "rows differ; first", int(np.argmax((_bits(a) != _bits(b)).any(axis=1))))


def _make(route):
    from trackdlo_amd import binding as B
    old = {k: os.environ.get(k) for k in ("TDLO_CLOUD_TEAM", "TDLO_CLOUD_FUSED")}
    try:
        for k in old:
            os.environ.pop(k, None)
        if route == "one":
            os.environ["TDLO_CLOUD_TEAM"] = "0"
        elif route == "multi":
            os.environ["TDLO_CLOUD_FUSED"] = "0"
        return B.Context(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    c = {r: _make(r) for r in ROUTES}
    yield c
    for x in c.values():
        x.close()


def _delta(route, scene_route, calls=1):
    if route == "multi" or scene_route == "untouched":
        return [0, 0]
    return [calls, 0] if scene_route == "taken" else [0, calls]


def _run(ctx, route, s, what=None, reps=1):
    """The scene on the context: X (bits), n, n_raw, and the route counters' movement."""
    Xr, nraw_r = s.ref
    for rep in range(reps):
        before = ctx.cloud_route_counts()
        X, n, nraw = ctx.depth_to_cloud(0, s.depth, s.mask, *s.cam, s.leaf)
        after = ctx.cloud_route_counts()
        assert [a - b for a, b in zip(after, before)] == _delta(route, s.route), (what or s.name, route, rep, before, after, s.route)
        assert nraw == nraw_r and n == Xr.shape[0], (what or s.name, route, rep, n, nraw, Xr.shape, nraw_r)
        _same_bits(X, Xr, (what or s.name, route, rep))
    st = s.structure
    if s.route == "taken" and route != "multi":
        SEEN["run"] = max(SEEN["run"], int(st["runs"].max()) if st["n"] else 0); SEEN["tiles"] = max(SEEN["tiles"], s.T); SEEN["kb"] = max(SEEN["kb"], st["kb"])
    SEEN["cases"] += reps


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", S.NAMES)
def test_scene(ctxs, name, route):
    _run(ctxs[route], route, S.get(name), reps=2)          # (the second call finds the kernels' state words and sort buffers as the first one left them)


class _Empty:
    """A frame with nothing segmented: the kernel itself reports an empty cloud."""
    name, route, leaf = "empty", "taken", S.LEAF

    def __init__(self, like):
        self.depth, self.mask, self.cam, self.T = like.depth, np.zeros_like(like.mask), like.cam, like.T
        self.ref = (np.zeros((0, 3)), 0)
        self.structure = dict(n=0, kb=1, runs=np.zeros(0, dtype=np.int64))


@pytest.mark.parametrize("route", ("team", "one"))
def test_one_context_through_frames_of_different_sizes(route):
    """The team's sort words, digit counts and compacted points (and the single workgroup's state words) keep the earlier frame's contents: a frame of another
    size, another image shape or no points at all behind a full one must not see them."""
    ctx = _make(route)
    try:
        seq = [S.get("C_distinct"), S.get("C_65"), S.get("B_i"), _Empty(S.get("A")), S.get("C_1"), S.get("B_iii"), S.get("D_2_alternate")]
        for i, s in enumerate(seq):
            _run(ctx, route, s, what=("sequence", i, s.name))
        assert ctx.cloud_route_counts() == [len(seq), 0]
    finally:
        ctx.close()


def _nodes(s, M, seed):
    """M nodes 0.2 .. 3 mm from centroids of the reference cloud: the first ones from the centroids of runs that cross a slice end, the next ones from
    centroids of the member slice with the most heads, the rest anywhere; every fifth node 3 .. 5 cm off the cloud (beyond the threshold)."""
    rng = np.random.default_rng(seed)
    X = s.ref[0]
    st = s.structure
    h = S.heads_of(st["runs"]); e = h + st["runs"]
    _, per, _ = S.team_slices(st["n_raw"], s.T)
    crossing = np.nonzero((h // per) != ((e - 1) // per))[0]
    member = np.bincount(h // per)
    busy = np.nonzero(h // per == int(np.argmax(member)))[0]
    pick = list(rng.permutation(crossing)[: max(1, M // 4)]) + list(rng.choice(busy, max(1, M // 4)))
    pick = (pick + list(rng.integers(0, len(X), M)))[:M]
    d = rng.normal(size=(M, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = rng.uniform(0.0002, 0.003, (M, 1))
    r[: 2 * max(1, M // 4)] *= 0.25                                  # (under half the 2 mm between neighbouring cells: the chosen centroid IS the nearest)
    Y = X[pick] + d * r
    if S.family(s.name) == "G":
        Y[4::5, 2] -= 0.05                                           # (in front of the wall)
    else:
        Y[4::5, 0] += 0.03                                           # (the long-lens scenes' centroids lie on the optical axis)
    return np.ascontiguousarray(Y), np.arange(M) * 0.01, crossing, int(member.max())


@pytest.mark.parametrize("name", ["A", "B_iii", "B_v", "G_wall"])
def test_the_visibility_ride_on_constructed_scenes(ctxs, name):
    """tdlo_depth_to_cloud_visibility: the minima that every team member takes over its own centroids -- members without a head (B_v), the centroid of a run
    that crosses a slice end, members with hundreds of heads -- are tests/prepass_ref.py's on the reference cloud, bit for bit."""
    ctx = ctxs["team"]
    s = S.get(name)
    X = s.ref[0]
    vt, d_vis = 0.008, 0.06
    for M in (1, 63, 64, 65):
        Y, coord, crossing, busiest = _nodes(s, M, 1000 + M)
        assert len(crossing) >= 1 and (busiest >= 100 or name == "B_v")
        rides, routes = ctx.cloud_vis_rides(), ctx.cloud_route_counts()
        dist, vis, ext, n, nraw = ctx.depth_to_cloud_visibility(0, s.depth, s.mask, *s.cam, s.leaf, Y, vt, d_vis, coord)
        assert ctx.cloud_vis_rides() - rides == (1 if M <= 64 else 0), (name, M)
        assert [a - b for a, b in zip(ctx.cloud_route_counts(), routes)] == [1, 0], (name, M)
        d2, arg = prepass_ref.min_d2(X, Y)
        want_dist, want_vis, want_ext = prepass_ref.threshold_and_fill(d2, vt, d_vis, coord)
        assert arg[0] in crossing                                    # (node 0's nearest centroid was formed from a run that crosses a slice end)
        assert n == X.shape[0] and nraw == s.ref[1]
        assert np.array_equal(dist.view(np.uint64), np.asarray(want_dist).view(np.uint64)), (name, M, int(np.argmax(dist != want_dist)))
        assert np.array_equal(vis, want_vis) and np.array_equal(ext, want_ext), (name, M)
        if M >= 63:
            assert 0 < len(vis) < M                                  # nodes on both sides of the threshold
        _same_bits(ctx.get_cloud(0), X, (name, M, "the cloud left in the slot"))
        SEEN["cases"] += 1


@pytest.mark.parametrize("route", ("team", "one"))
@pytest.mark.parametrize("name", ["A", "D_7_last"])
def test_the_colour_instantiation(ctxs, name, route):
    """The scene as a colour frame (tdlo_colour_depth_to_cloud): the segmentation formed inside the one-launch kernels -- wanted pixels inside the range, the
    others one unit outside it in H, S or V, some inside it behind an occluder byte of 0 -- gives the scene's cloud, and the fused instantiation ran."""
    from trackdlo_amd import binding as B
    ctx = ctxs[route]
    s = S.get(name)
    colour, occ, lower, upper = S.paint(s, seed=900)
    before, cbefore = ctx.cloud_route_counts(), ctx.colour_route_counts()
    for rep in range(2):
        X, n, nraw = ctx.colour_depth_to_cloud(0, s.depth, colour, B.make_colour_params(lower, upper), occ, *s.cam, s.leaf)
        assert nraw == s.ref[1] and n == s.ref[0].shape[0]
        _same_bits(X, s.ref[0], (name, route, rep))
    assert [a - b for a, b in zip(ctx.cloud_route_counts(), before)] == [2, 0]
    assert [a - b for a, b in zip(ctx.colour_route_counts(), cbefore)] == [2, 0]
    SEEN["cases"] += 2


def test_zz_worst_case_note():
    print("\n[cloud scenes] %d calls checked bit for bit; the one-launch kernels took: largest run %d points, %d tiles, kb %d"
          % (SEEN["cases"], SEEN["run"], SEEN["tiles"], SEEN["kb"]))
    assert SEEN["run"] == S.kFNmax and SEEN["tiles"] == S.kFTmax and SEEN["kb"] >= 17
