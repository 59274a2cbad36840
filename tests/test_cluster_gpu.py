"""tdlo_cloud_cluster / tdlo_tracker_initialize_from_shared_cloud_batch on the device, against the statement (tests/cluster_ref.py): owners, counts, n_clusters
and every copied coordinate bit for bit on every scene, on the device route and on a TDLO_CLUSTER=host context (the variable is read when a context is made:
test_prepass_gpu.make_ctx, the way the tree tests such variables); the source unchanged; the route counters 55 / 56 in every case; every refusal; the
consequences for the calls that follow.  No test provokes the give-up path: the forced host route is the same code from the fall-back point on."""
import numpy as np
import pytest

from test_prepass_gpu import make_ctx
import assign_ref as AR
import cluster_ref as CR

pytestmark = pytest.mark.gpu
FMAX = 6                  # max_frames of the test contexts: five destinations and the source
SRC = 5
MU, ITERS = 0.05, 12


def ctx_for(host, frames=FMAX, points=2048):
    return make_ctx({"TDLO_CLUSTER": "host" if host else None}, max_frames=frames, max_points=points, max_nodes=64)


@pytest.fixture(scope="module")
def ctxs():
    both = {False: ctx_for(False), True: ctx_for(True)}
    yield both
    for c in both.values():
        c.close()


def check_cluster(c, host, name, slots=None, src=SRC):
    s, (owner, C, n_each, un, _) = CR.scene(name)
    X, F = s["X"], s["F"]
    slots = list(range(F)) if slots is None else slots
    c.set_cloud(src, X)
    before = c.cluster_route_counts()
    nc, ne, nu, own = c.cloud_cluster(src, slots, s["tol"], s["min_size"], owners=True)
    assert (nc, ne, nu) == (C, n_each, un), (name, nc, ne, nu, C, n_each, un)
    assert np.array_equal(own, owner), name
    for f, part in enumerate(CR.split(X, owner, F)):
        got = c.get_cloud(slots[f])
        assert got.shape == part.shape and np.array_equal(CR.bits(got), CR.bits(part)), (name, f)
    assert np.array_equal(CR.bits(c.get_cloud(src)), CR.bits(X))                    # the source stays
    assert c.cluster_route_counts() == [before[0] + (0 if host else 1), before[1] + (1 if host else 0)], name
    return owner, n_each


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("name", list(CR.SCENES))
def test_every_scene_on_both_routes(ctxs, name, host):
    check_cluster(ctxs[host], host, name)


@pytest.mark.parametrize("host", [False, True])
def test_destinations_in_descending_order_shrink_and_the_trailing_ones_are_empty(ctxs, host):
    c = ctxs[host]
    big = CR.ropes(1500, 1, seed=11)
    for s in (0, 1, 2, 3):
        c.set_cloud(s, big)
    _, n_each = check_cluster(c, host, "few", slots=[3, 2, 1, 0])
    assert n_each == [65, 65, 0, 0] and c.get_cloud(1).shape == (0, 3) and c.get_cloud(0).shape == (0, 3) and c.get_cloud(3).shape == (65, 3)


@pytest.mark.parametrize("host", [False, True])
def test_a_context_taken_through_scenes_of_different_sizes(host):
    """The workspace grows from a point to 1 025 and is used again for less: nothing stale survives."""
    c = ctx_for(host, frames=4, points=64)
    try:
        for name in ("ropes2_n1", "chain_stride", "ropes3_n63", "ropes3_n1025", "gate", "ropes2_n513", "non_finite", "ropes2_n1"):
            check_cluster(c, host, name, src=3)
    finally:
        c.close()


@pytest.mark.parametrize("host", [False, True])
def test_refusals_and_an_empty_source_leave_clouds_and_counters_alone(ctxs, host):
    c = ctxs[host]
    X = CR.ropes(65, 2, seed=1)
    keep = CR.ropes(64, 1, seed=8)
    c.set_cloud(SRC, X); c.set_cloud(0, keep); c.set_cloud(1, keep)
    before = c.cluster_route_counts()
    bad = [dict(d=[SRC, 1]), dict(d=[1, 1]), dict(src=FMAX), dict(src=-1), dict(d=[0, FMAX]), dict(d=[0, -1]), dict(d=[0, 1, 2, 3, 4, 0, 1]),
           dict(tol=0.0), dict(tol=-0.01), dict(tol=np.nan), dict(tol=np.inf), dict(m=0), dict(m=-1)]
    for b in bad:
        rc = c.cloud_cluster(b.get("src", SRC), b.get("d", [0, 1]), b.get("tol", CR.TOL), b.get("m", 1), check=False)[0]
        assert rc == -2, b
    assert c.lib.tdlo_cloud_cluster(c.h, SRC, None, 0, CR.TOL, 1, None, None, None, None) == -2      # F < 1
    assert c.lib.tdlo_cloud_cluster(c.h, SRC, None, 2, CR.TOL, 1, None, None, None, None) == -2      # no destinations
    assert c.cluster_route_counts() == before
    for s in (0, 1):
        assert np.array_equal(CR.bits(c.get_cloud(s)), CR.bits(keep))
    assert np.array_equal(CR.bits(c.get_cloud(SRC)), CR.bits(X))
    # a source of 0 points (what a clustering into more destinations than clusters leaves): TDLO_OK, every count 0, nothing launched
    check_cluster(c, host, "few", slots=[0, 1, 2, 3])
    c.set_cloud(0, keep)
    before = c.cluster_route_counts()
    assert c.cloud_cluster(3, [0, 1], CR.TOL, 1) == (0, [0, 0], 0)
    assert c.get_cloud(0).shape == (0, 3) and c.cluster_route_counts() == before


def test_a_source_beyond_the_all_pairs_limit_is_refused():
    c = ctx_for(False, frames=2, points=262145)
    try:
        X = np.zeros((262145, 3), order="F"); X[:, 0] = np.arange(262145)
        keep = CR.ropes(64, 1, seed=8)
        c.set_cloud(1, X); c.set_cloud(0, keep)
        assert c.cloud_cluster(1, [0], 0.5, 1, check=False)[0] == -2 and c.cluster_route_counts() == [0, 0]
        assert np.array_equal(CR.bits(c.get_cloud(0)), CR.bits(keep))
    finally:
        c.close()


def test_assign_to_the_cluster_centroids_reproduces_the_owners(ctxs):
    """tdlo_cloud_cluster, then tdlo_cloud_assign with the reference's cluster centroids as one-node ropes and no gate: on well-separated clusters the owners."""
    c = ctxs[False]
    s, (owner, C, n_each, un, _) = CR.scene("ropes3_n257")
    check_cluster(c, False, "ropes3_n257")
    cents = [np.asfortranarray(s["X"][owner == f].mean(axis=0)[None, :]) for f in range(3)]
    ne, nu, own, _ = c.cloud_assign(SRC, list(zip([0, 1, 2], cents)), np.inf, owners=True)
    assert np.array_equal(own, owner) and ne == n_each and nu == 0
    for f, part in enumerate(CR.split(s["X"], owner, 3)):
        assert np.array_equal(CR.bits(c.get_cloud(f)), CR.bits(part))


def trackers(c, F, M):
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    return [B.trackdlo(*args, ctx=c, slot=i) for i in range(F)]


_ROPES = {}


def rope_cloud(F, M=20):
    """F ropes of M nodes 5 cm apart, 200 points each interleaved point by point, and the statement's clustering of them (once per process): F clusters."""
    if F not in _ROPES:
        X, _, _ = AR.cloud_scene(200 * F, (M,) * F, seed=F, far=0.0)
        ref = CR.cluster(X, F, CR.TOL, 10)
        assert ref[1] == F and ref[2] == [200] * F
        _ROPES[F] = (X, ref)
    return _ROPES[F]


def same_state(ta, tb):
    return all(np.array_equal(CR.bits(a.get_tracking_result()), CR.bits(b.get_tracking_result())) and
               np.array_equal(CR.bits(a.get_guide_nodes()), CR.bits(b.get_guide_nodes())) and a.get_sigma2() == b.get_sigma2() for a, b in zip(ta, tb))


@pytest.mark.parametrize("F", [1, 2, 3, 5])
def test_the_tracker_call_is_cluster_then_initialize_by_hand(F):
    """Nodes, guide nodes and sigma2_out bit for bit; the chain coordinate has no getter: it is held by the frame both sets of trackers take afterwards, whose
    pre-pass reads it."""
    from trackdlo_amd import binding as B
    M = 20
    X, (owner, C, n_each, un, _) = rope_cloud(F, M)
    ca, cb = ctx_for(False), ctx_for(False)
    try:
        ta, tb = trackers(ca, F, M), trackers(cb, F, M)
        ca.set_cloud(SRC, X); cb.set_cloud(SRC, X)
        before = ca.cluster_route_counts()
        codes, s2, nc, ne = B.initialize_from_shared_cloud_batch(ta, SRC, CR.TOL, 10, MU, ITERS)
        assert ca.cluster_route_counts() == [before[0] + 1, before[1]]
        assert cb.cloud_cluster(SRC, list(range(F)), CR.TOL, 10) == (C, n_each, un)
        hcodes, hs2 = B.initialize_from_cloud_batch(tb, MU, ITERS)
        assert codes == hcodes == [0] * F and nc == C == F and ne == n_each
        assert np.array_equal(CR.bits(s2), CR.bits(hs2)) and np.isfinite(s2).all()
        assert same_state(ta, tb)
        for f, part in enumerate(CR.split(X, owner, F)):
            assert np.array_equal(CR.bits(ca.get_cloud(f)), CR.bits(part))
        for t, u, v in zip(ta, tb, s2):
            t.set_sigma2(v); u.set_sigma2(v)
        X2 = np.asfortranarray(X + np.array([0.0, 0.002, 0.0]))
        ca.set_cloud(SRC, X2); cb.set_cloud(SRC, X2)
        ra = B.frames_from_shared_cloud_batch(ta, SRC, 0.02, 0.06); rb = B.frames_from_shared_cloud_batch(tb, SRC, 0.02, 0.06)
        assert ra[0] == rb[0] == [0] * F and ra[3] == rb[3] and all(np.array_equal(p, q) for p, q in zip(ra[1] + ra[2], rb[1] + rb[2]))
        assert same_state(ta, tb)
    finally:
        ca.close(); cb.close()


def test_another_number_of_clusters_leaves_every_tracker_untouched(ctxs):
    from trackdlo_amd import binding as B
    c = ctxs[False]
    M = 20
    X, (owner, C, n_each, un, _) = rope_cloud(3, M)
    for F in (2, 4):                                                     # C = 3 > F and C = 3 < F
        ref = CR.cluster(X, F, CR.TOL, 10)
        t = trackers(c, F, M)
        _, Y, coords = AR.cloud_scene(10, (M,) * F, seed=9)
        for k in range(F):
            t[k].initialize_nodes(Y[k]); t[k].initialize_geodesic_coord(coords[k]); t[k].set_sigma2(0.125)
        keep = [(u.get_tracking_result().copy(), u.get_guide_nodes().copy()) for u in t]
        c.set_cloud(SRC, X)
        before = c.cluster_route_counts()
        rc, codes, s2, nc, ne = B.initialize_from_shared_cloud_batch(t, SRC, CR.TOL, 10, MU, ITERS, check=False)
        assert rc == B.TDLO_E_INVALID and nc == 3 and ne == ref[2] and c.cluster_route_counts() == [before[0] + 1, before[1]]
        for u, (y, g) in zip(t, keep):
            assert np.array_equal(CR.bits(u.get_tracking_result()), CR.bits(y)) and np.array_equal(CR.bits(u.get_guide_nodes()), CR.bits(g)) and u.get_sigma2() == 0.125
        for f, part in enumerate(CR.split(X, ref[0], F)):                # the slots hold the split
            assert np.array_equal(CR.bits(c.get_cloud(f)), CR.bits(part))
        # refused as a whole: the source among the trackers' slots, a bad tol, bad reg arguments -- counters and slots untouched
        before = c.cluster_route_counts()
        for kw in (dict(src=0), dict(tol=-1.0), dict(mu=1.0), dict(it=-1), dict(ms=0)):
            out = B.initialize_from_shared_cloud_batch(t, kw.get("src", SRC), kw.get("tol", CR.TOL), kw.get("ms", 10), kw.get("mu", MU), kw.get("it", ITERS), check=False)
            assert out[0] == B.TDLO_E_INVALID, kw
        assert c.cluster_route_counts() == before and np.array_equal(CR.bits(c.get_cloud(0)), CR.bits(CR.split(X, ref[0], F)[0]))


def test_three_trackers_started_from_one_cloud_then_stepped_equal_twins_started_from_split_clouds():
    from trackdlo_amd import binding as B
    M, F = 20, 3
    X, (owner, C, n_each, un, _) = rope_cloud(F, M)
    ca, cb = ctx_for(False), ctx_for(False)
    try:
        ta, tb = trackers(ca, F, M), trackers(cb, F, M)
        ca.set_cloud(SRC, X)
        codes, s2, nc, ne = B.initialize_from_shared_cloud_batch(ta, SRC, CR.TOL, 10, MU, ITERS)
        for f, part in enumerate(CR.split(X, owner, F)):
            cb.set_cloud(f, part)
        hcodes, hs2 = B.initialize_from_cloud_batch(tb, MU, ITERS)
        assert codes == hcodes == [0] * F and np.array_equal(CR.bits(s2), CR.bits(hs2))
        for t, u, v in zip(ta, tb, s2):
            t.set_sigma2(v); u.set_sigma2(v)
        for fr in range(1, 6):
            Xf = np.asfortranarray(X + np.array([0.0005 * fr, 0.001 * fr, 0.0]))
            ca.set_cloud(SRC, Xf); cb.set_cloud(SRC, Xf)
            ra = B.frames_from_shared_cloud_batch(ta, SRC, 0.02, 0.06); rb = B.frames_from_shared_cloud_batch(tb, SRC, 0.02, 0.06)
            assert ra[0] == rb[0] == [0] * F and ra[3] == rb[3] and min(ra[3]) > 0, (fr, ra[0], ra[3])      # (every tracker owns points and steps)
            assert all(np.array_equal(p, q) for p, q in zip(ra[1] + ra[2], rb[1] + rb[2])) and same_state(ta, tb), fr
    finally:
        ca.close(); cb.close()
