"""tdlo_cloud_assign / tdlo_cloud_assign_visibility / tdlo_tracker_frames_from_shared_cloud_batch on the device, against the statement (tests/assign_ref.py):
owners, the bits of g and of every copied coordinate, counts, the slots' state, the consequences for the calls that follow, every refusal and both route
counters (53 / 54) in every case.  TDLO_ASSIGN_RIDE is read when a context is made: both settings run on contexts made under them (test_prepass_gpu.make_ctx,
the way the tree tests such variables)."""
import numpy as np
import pytest

from test_prepass_gpu import make_ctx
import assign_ref as AR

pytestmark = pytest.mark.gpu
FMAX = 6                  # max_frames of the test contexts: five destinations and the source
SRC = 5
D_MAX = 0.008


def ctx_for(ride, frames=FMAX, **kw):
    return make_ctx({"TDLO_ASSIGN_RIDE": 1 if ride else None}, max_frames=frames, max_points=2048, max_nodes=64, **kw)


@pytest.fixture(scope="module")
def ctx():
    c = ctx_for(False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ride_ctx():
    c = ctx_for(True)
    yield c
    c.close()


_REF = {}


def ref(key, X, ropes, d_max):
    """The statement of a case, computed once per process and left unchanged."""
    if key not in _REF:
        _REF[key] = AR.assign(X, ropes, d_max)
    return _REF[key]


def check_split(c, key, X, ropes, slots, d_max, src=SRC):
    c.set_cloud(src, X)
    before = c.assign_route_counts()
    n_each, un, own, d2 = c.cloud_assign(src, list(zip(slots, ropes)), d_max, owners=True)
    ro, rg, rn, ru = ref(key, X, ropes, d_max)
    assert n_each == rn and un == ru, (key, n_each, rn, un, ru)
    assert np.array_equal(own, ro) and np.array_equal(AR.bits(d2), AR.bits(rg)), key
    for f, part in enumerate(AR.split(X, ro, len(ropes))):
        got = c.get_cloud(slots[f])
        assert got.shape == part.shape and np.array_equal(AR.bits(got), AR.bits(part)), (key, f)
    assert np.array_equal(AR.bits(c.get_cloud(src)), AR.bits(X))                    # the source stays
    assert c.assign_route_counts() == [before[0] + 1, before[1]], key
    return ro, rn


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_sizes_around_waves_and_workgroups(ctx, n):
    X, ropes, _ = AR.cloud_scene(n, (2, 45), seed=1)
    check_split(ctx, ("sz", n), X, ropes, [0, 1], D_MAX)
    check_split(ctx, ("sz1", n), X, ropes[:1], [3], np.inf)                          # F = 1, no gate: every finite point


def test_three_ropes_interleaved_point_by_point_cross_every_block_border(ctx):
    X, ropes, _ = AR.cloud_scene(1025, (45, 45, 45), seed=1)
    ro, rn = check_split(ctx, "inter", X, ropes, [0, 1, 2], D_MAX)
    for b in range(0, 1024, 256):                                                      # (the fifth block holds the last point alone)
        assert set(ro[b:b + 256].tolist()) >= {0, 1, 2}
    assert min(rn) > 250


def test_mixed_node_counts_destinations_reversed_and_shrinking(ctx):
    """M_f = 1, 2, 45, 300 in one call (348 nodes: one tile); destinations in descending slot order that held larger clouds before."""
    big, _, _ = AR.cloud_scene(1500, (5,), seed=9)
    for s in (0, 1, 2, 3):
        ctx.set_cloud(s, big)
    X, ropes, _ = AR.cloud_scene(257, (1, 2, 45, 300), seed=1)
    _, rn = check_split(ctx, "mixed", X, ropes, [3, 2, 1, 0], D_MAX)
    assert max(rn) < 1500 and sum(len(r) for r in ropes) < AR.TILE


def test_node_list_beyond_one_tile_and_the_exact_tie(ctx):
    """645 nodes: two LDS tiles; point 0 is exactly equidistant from rope 0 (tile 0) and rope 2 (tile 1) and goes to rope 0."""
    X, ropes, d_max, i = AR.tie_scene()
    assert sum(len(r) for r in ropes) > AR.TILE
    ro, _ = check_split(ctx, "tie", X, ropes, [0, 1, 2], d_max)
    assert ro[i] == 0 and AR.rope_min(X[i:i + 1], ropes[0])[0] == AR.rope_min(X[i:i + 1], ropes[2])[0]


def test_gate_exactly_at_and_one_ulp_above(ctx):
    X, ropes, d_max = AR.gate_scene()
    ro, _ = check_split(ctx, "gate", X, ropes, [0, 1], d_max)
    assert ro.tolist() == [0, -1, 1, -1]


def test_non_finite_points_and_signed_zeros(ctx):
    X, ropes, _ = AR.cloud_scene(300, (45, 7), seed=3)
    Xs, bad = AR.with_specials(X)
    ro, _ = check_split(ctx, "nan", Xs, ropes, [0, 1], D_MAX)
    assert (ro[bad] == -1).all()
    Z, zr = AR.zero_scene()
    check_split(ctx, "zero", Z, zr, [0, 1], 0.05)
    assert np.signbit(ctx.get_cloud(0)).sum() == 8


def test_max_frames_ropes(ctx):
    """F = max_frames - 1 destinations beside the source fill the context; F = max_frames itself is accepted as a count (and then refused for its slots)."""
    X, ropes, _ = AR.cloud_scene(257, (3, 4, 5, 6, 7), seed=2)
    check_split(ctx, "fmax", X, ropes, [0, 1, 2, 3, 4], D_MAX)
    c1 = ctx_for(False, frames=2)
    try:
        c1.set_cloud(1, X)
        rc = c1.cloud_assign(1, [(0, ropes[0]), (1, ropes[1])], D_MAX, check=False)[0]     # F = max_frames = 2: the source is then among the destinations
        assert rc == -2 and c1.assign_route_counts() == [0, 0]
    finally:
        c1.close()


def test_every_point_to_one_rope_none_inside_the_gate_and_an_empty_source(ctx):
    X, ropes, _ = AR.cloud_scene(257, (45, 45), seed=6, far=0.0)
    far_rope = np.asfortranarray(ropes[1] + np.array([0.0, 3.0, 0.0]))
    _, rn = check_split(ctx, "one", X, [ropes[0], far_rope], [0, 1], np.inf)
    assert rn == [257, 0] and ctx.get_cloud(1).shape == (0, 3)
    # no point inside the gate: every destination empty, TDLO_OK
    away = [np.asfortranarray(r + np.array([0.0, 3.0, 0.0])) for r in ropes]
    _, rn = check_split(ctx, "none", X, away, [0, 1], D_MAX)
    assert rn == [0, 0]
    # the cloud of 0 points that this left in slot 0 as a source: TDLO_OK, every count 0, nothing launched
    ctx.set_cloud(2, X)
    before = ctx.assign_route_counts()
    assert ctx.cloud_assign(0, [(2, ropes[0]), (3, ropes[1])], D_MAX) == ([0, 0], 0)
    assert ctx.get_cloud(2).shape == (0, 3) and ctx.assign_route_counts() == before


def test_one_case_beyond_the_first_span_of_workgroups():
    """n = 70 001: 274 chunks of 256 points."""
    c = make_ctx(max_frames=4, max_points=70001, max_nodes=64)
    try:
        X, ropes, _ = AR.cloud_scene(70001, (45, 2, 1), seed=1)
        check_split(c, "large", X, ropes, [0, 1, 2], D_MAX, src=3)
    finally:
        c.close()


def test_refusals_leave_clouds_and_counters_alone(ctx):
    X, ropes, _ = AR.cloud_scene(65, (2, 45), seed=1)
    keep, _, _ = AR.cloud_scene(64, (3,), seed=8)
    ctx.set_cloud(SRC, X); ctx.set_cloud(0, keep); ctx.set_cloud(1, keep)
    before = ctx.assign_route_counts()
    nan_rope = np.array(ropes[1]); nan_rope[3, 1] = np.inf
    bad = [dict(r=[(SRC, ropes[0]), (1, ropes[1])]), dict(r=[(1, ropes[0]), (1, ropes[1])]), dict(src=FMAX), dict(src=-1), dict(r=[(0, ropes[0]), (FMAX, ropes[1])]),
           dict(r=[(s, ropes[0]) for s in (0, 1, 2, 3, 4, 0, 1)]), dict(r=[(0, ropes[0]), (1, nan_rope)]), dict(r=[(0, ropes[0]), (1, np.zeros((0, 3)))]),
           dict(d=0.0), dict(d=-0.01), dict(d=np.nan)]
    for b in bad:
        rc = ctx.cloud_assign(b.get("src", SRC), b.get("r", [(0, ropes[0]), (1, ropes[1])]), b.get("d", D_MAX), check=False)[0]
        assert rc == -2, b
    assert ctx.lib.tdlo_cloud_assign(ctx.h, SRC, None, 0, D_MAX, None, None, None, None) == -2      # F < 1
    assert ctx.assign_route_counts() == before
    for s in (0, 1):
        assert np.array_equal(AR.bits(ctx.get_cloud(s)), AR.bits(keep))
    assert np.array_equal(AR.bits(ctx.get_cloud(SRC)), AR.bits(X))


def test_a_registration_on_a_split_slot_is_the_one_on_a_cloud_set_by_hand(ctx):
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    X, ropes, _ = AR.cloud_scene(1025, (45, 45), seed=7)
    par = B.make_params(beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], max_iter=10, tol=0.0, include_lle=False, alpha=0.0,
                        k_vis=0.0, visibility_threshold=P["visibility_threshold"])
    twin = ctx_for(False)
    try:
        ro, _ = check_split(ctx, "reg", X, ropes, [0, 1], D_MAX)
        for f in (0, 1):
            twin.set_cloud(f, AR.split(X, ro, 2)[f])
            a = ctx.cpd_lle_resident(f, ropes[f], 1e-4, par); b = twin.cpd_lle_resident(f, ropes[f], 1e-4, par)
            assert np.array_equal(AR.bits(a["Y"]), AR.bits(b["Y"])) and a["sigma2"] == b["sigma2"] and a["iters"] == b["iters"] == 10
            assert a["n_kept"] == b["n_kept"] > 0 and a["sort_reused"] == b["sort_reused"] == 0
    finally:
        twin.close()


@pytest.mark.parametrize("ride", [False, True])
def test_assign_visibility_is_assign_then_the_prepass_per_slot(ctx, ride_ctx, ride):
    """Mixed node counts, a rope that owns nothing among them; on both settings of TDLO_ASSIGN_RIDE, against the two calls made by hand AND against the statement."""
    c = ride_ctx if ride else ctx
    X, ropes, coords = AR.cloud_scene(1025, (45, 2, 45, 30), seed=5)
    ropes[3] = np.asfortranarray(ropes[3] + np.array([0.0, 3.0, 0.0]))               # owns nothing
    slots = [0, 1, 2, 3]
    c.set_cloud(SRC, X)
    before = c.assign_route_counts()
    n_each, un, dist, vis, ext = c.cloud_assign_visibility(SRC, list(zip(slots, ropes)), D_MAX, 0.004, 0.06, coords)
    assert c.assign_route_counts() == [before[0] + 1, before[1] + (1 if ride else 0)]
    ro, _, rn, ru = ref("vis", X, ropes, D_MAX)
    assert n_each == rn and un == ru and rn[3] == 0 and min(rn[:3]) > 0
    parts = AR.split(X, ro, 4)
    for f in range(4):
        got = c.get_cloud(slots[f])
        assert np.array_equal(AR.bits(got), AR.bits(parts[f]))
        rd, rv, re_ = AR.visibility(parts[f], ropes[f], 0.004, 0.06, coords[f])
        assert np.array_equal(AR.bits(dist[f]), AR.bits(rd)) and np.array_equal(vis[f], rv) and np.array_equal(ext[f], re_), (ride, f)
        if rn[f]:
            hd, hv, he = c.visibility_prepass(slots[f], ropes[f], 0.004, 0.06, coords[f])                 # by hand on the slot
            assert np.array_equal(AR.bits(dist[f]), AR.bits(hd)) and np.array_equal(vis[f], hv) and np.array_equal(ext[f], he)
    assert (dist[3] == 100000.0).all() and len(vis[3]) == 0 and len(vis[0]) > 0
    # and once more: the kernel re-armed its minima
    again = c.cloud_assign_visibility(SRC, list(zip(slots, ropes)), D_MAX, 0.004, 0.06, coords)
    assert all(np.array_equal(AR.bits(a), AR.bits(b)) for a, b in zip(again[2], dist))


def shared_trackers(c, Y0, coords, M):
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    out = []
    for i in range(len(Y0)):
        t = B.trackdlo(*args, ctx=c, slot=i)
        t.initialize_nodes(Y0[i]); t.initialize_geodesic_coord(coords[i])
        out.append(t)
    return out


@pytest.mark.parametrize("ride", [False, True])
def test_two_crossing_ropes_over_ten_frames_equal_assign_and_frame_batch_by_hand(ride):
    from trackdlo_amd import binding as B
    M = 45
    Y0, coords, clouds = AR.crossing_ropes(M=M, frames=10)
    env = {"TDLO_ESTEP2": 0, "TDLO_ASSIGN_RIDE": 1 if ride else None}
    ca = make_ctx(env, max_frames=3, max_points=2048, max_nodes=64); cb = make_ctx(dict(env, TDLO_ASSIGN_RIDE=None), max_frames=3, max_points=2048, max_nodes=64)
    try:
        ta, tb = shared_trackers(ca, Y0, coords, M), shared_trackers(cb, Y0, coords, M)
        for fr, X in enumerate(clouds):
            ca.set_cloud(2, X); cb.set_cloud(2, X)
            before = ca.assign_route_counts()
            codes, vis, ext, n_each = B.frames_from_shared_cloud_batch(ta, 2, 0.02, 0.06)
            assert ca.assign_route_counts() == [before[0] + 1, before[1] + (1 if ride else 0)]
            hn, _ = cb.cloud_assign(2, [(i, t.get_tracking_result()) for i, t in enumerate(tb)], 0.02)
            hcodes, hvis, hext = B.frame_batch(tb, 0.06)
            assert codes == hcodes == [0, 0] and n_each == hn and min(n_each) > 300, (fr, codes, hcodes, n_each, hn)
            for i in range(2):
                assert np.array_equal(vis[i], hvis[i]) and np.array_equal(ext[i], hext[i]) and len(vis[i]) > 0
                assert np.array_equal(AR.bits(ta[i].get_tracking_result()), AR.bits(tb[i].get_tracking_result())), (fr, i)
                assert ta[i].get_sigma2() == tb[i].get_sigma2()
                assert [s["iters"] for s in ta[i].last_stats] == [s["iters"] for s in tb[i].last_stats]
        # a tracker whose rope owns nothing is left as it is, the other goes on
        moved = tb[1].get_tracking_result() + np.array([0.0, 3.0, 0.0])
        ta[1].initialize_nodes(moved)
        keep = ta[1].get_tracking_result().copy(); s2 = ta[1].get_sigma2()
        codes, vis, ext, n_each = B.frames_from_shared_cloud_batch(ta, 2, 0.02, 0.06, check=False)
        assert codes == [0, B.TDLO_E_EMPTY] and n_each[1] == 0 and n_each[0] > 300
        assert np.array_equal(ta[1].get_tracking_result(), keep) and ta[1].get_sigma2() == s2
        # refused as a whole: the source among the trackers' slots
        before = ca.assign_route_counts(); y = ta[0].get_tracking_result().copy()
        with pytest.raises(B.TdloError):
            B.frames_from_shared_cloud_batch(ta, 1, 0.02, 0.06)
        with pytest.raises(B.TdloError):
            B.frames_from_shared_cloud_batch(ta, 2, -1.0, 0.06)
        assert ca.assign_route_counts() == before and np.array_equal(ta[0].get_tracking_result(), y)
    finally:
        ca.close(); cb.close()
