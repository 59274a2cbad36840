"""The self-occlusion test under a rig on the GPU (k_rig_painter_batch, csrc/tdlo_painter.hip): tdlo_rig_self_occlusion_batch equals the numpy / integer
statement (tests/rig_painter_ref.py) on every scene of tests/rig_painter_scenes.py and in batches, in sets and per-camera words, with the served-jobs counter;
whole-call refusals touch nothing; a context goes through batches of growing and shrinking size; the two rig tracker calls with the switch on against twins
stepped by hand, bit for bit, on both routes.  Every comparison is exact."""
import numpy as np
import pytest

import rig_painter_scenes as PS
import rig_ref as R
import rig_scenes as S
from test_prepass_gpu import make_ctx
from test_rig_batch_gpu import M, D_VIS, make_trackers, rope_rigs, same_bits, state, targs
from trackdlo_amd import binding as B_

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    return binding


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx({}, max_frames=4, max_points=1 << 15, max_nodes=64)
    yield c
    c.close()


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def run_batch(ctx, group, label):
    """One call for the scenes of `group` (they share an image size); sets, words and the served-jobs counter."""
    rows, cols = group[0][0].rows, group[0][0].cols
    before = ctx.rig_painter_route_counts()
    vis, seen, hidden = ctx.rig_self_occlusion_batch([s.frame() for s, *_ in group], rows, cols, words=True)
    after = ctx.rig_painter_route_counts()
    assert [a - b for a, b in zip(after, before)] == [sum(s.K for s, *_ in group), 0], label
    for i, (s, v, sw, hw, per) in enumerate(group):
        assert same((vis[i], seen[i], hidden[i]), (v, sw, hw)), (label, i, s.name)


@pytest.mark.parametrize("i", range(len(PS.scenes())), ids=[s[0].name for s in PS.scenes()])
def test_every_scene_alone(ctx, i):
    run_batch(ctx, [PS.scenes()[i]], PS.scenes()[i][0].name)


@pytest.mark.parametrize("name", ["F=1", "F=2", "F=33"])
def test_batches_of_unequal_frames(ctx, name):
    run_batch(ctx, PS.batches()[name], name)


def test_all_scenes_of_one_image_size_in_one_call_in_any_order(ctx):
    group = [e for e in PS.scenes() if (e[0].rows, e[0].cols) == (PS.ROWS, PS.COLS)]
    assert len(group) >= 15 and max(e[0].M for e in group) == 1024 and max(e[0].K for e in group) == 64
    run_batch(ctx, group, "all")
    run_batch(ctx, group[::-1], "reversed")


def test_growing_and_shrinking_batches(ctx):
    b = PS.batches()
    big = [e for e in PS.scenes() if e[0].M >= 256 and (e[0].rows, e[0].cols) == (PS.ROWS, PS.COLS)]
    for label, group in (("one", b["F=1"]), ("33", b["F=33"]), ("two", b["F=2"]), ("big", big), ("33 + big", b["F=33"] + big), ("one again", b["F=1"])):
        run_batch(ctx, group, label)


def test_whole_call_refusals_touch_nothing(B, ctx):
    s = PS.scenes()[0][0]
    good = s.frame()
    Y, cams, mats, w, dist, thr = good
    before = ctx.rig_painter_route_counts()
    bad_frames = {"width 0": (Y, cams, mats, 0, dist, thr), "width 256": (Y, cams, mats, 256, dist, thr), "no cameras": (Y, [], None, w, dist, thr),
                  "65 cameras": (Y, [PS.CAM] * 65, None, w, dist, thr), "fx = 0": (Y, [(0.0, 1.0, 1.0, 1.0), PS.CAM], mats, w, dist, thr),
                  "fy = 0": (Y, [PS.CAM, (1.0, 0.0, 1.0, 1.0)], mats, w, dist, thr), "inf intrinsic": (Y, [PS.CAM, (1.0, 1.0, np.inf, 1.0)], mats, w, dist, thr),
                  "nan in a matrix": (Y, cams, [None, np.where(np.arange(12).reshape(3, 4) == 3, np.nan, PS.BEHIND)], w, dist, thr),
                  "1025 nodes": (np.zeros((1025, 3)), cams, mats, w, np.zeros(1025), thr), "no nodes": (np.zeros((0, 3)), cams, mats, w, np.zeros(0), thr)}
    for what, f in bad_frames.items():
        for frames in ([f], [good, f], [f, good]):
            with pytest.raises(B.TdloError) as e:
                ctx.rig_self_occlusion_batch(frames, s.rows, s.cols)
            assert e.value.code == B.TDLO_E_INVALID, what
    for rows, cols in ((0, 640), (8193, 640), (480, 0), (480, 8193)):
        with pytest.raises(B.TdloError):
            ctx.rig_self_occlusion_batch([good], rows, cols)
    with pytest.raises(B.TdloError):
        ctx.rig_self_occlusion_batch([], 480, 640)
    assert ctx.rig_painter_route_counts() == before
    run_batch(ctx, [PS.scenes()[0]], "after the refusals")


# ---- the trackers ---------------------------------------------------------------------------------------------------------------------------------
WIDTH = 10
SHIFT = np.array([[0, 0, 0, 0.0004], [0, 0, 0, -0.0003], [0, 0, 0, 0.0002]])
RIG_TO_CAM = [None, S.TRANSFORMS["identity"] - SHIFT]                           # the inverse of rope_rigs' second cam_to_rig
_CROSS = {}


def crossing_rig():
    """A 30-node rope that crosses itself, the strands 5 mm apart where they cross, seen by two cameras on ONE side (rope_rigs' pair of camera and matrix): the
    lower strand's node under the crossing lies within the visibility threshold of the upper strand's points, and both cameras see it painted over.
    Returns (cams, Y0)."""
    from trackdlo_amd import synth
    if not _CROSS:
        cam = dict(synth.CAMERA)
        A = [(x, 0.0, 0.6) for x in np.linspace(-0.1, 0.1, 11)]
        link = [(0.13, 0.02, 0.601), (0.15, 0.05, 0.602), (0.15, 0.09, 0.603), (0.13, 0.12, 0.604), (0.1, 0.14, 0.604), (0.06, 0.14, 0.605), (0.03, 0.13, 0.605), (0.01, 0.115, 0.605)]
        Bs = [(0.0, y, 0.605) for y in np.linspace(0.1, -0.1, 11)]
        Y0 = np.array(A + link + Bs)
        assert len(Y0) == M
        rng = np.random.default_rng(4)
        n = 150000
        e = rng.integers(0, M - 1, n); t = rng.random(n)
        p = (1 - t)[:, None] * Y0[e] + t[:, None] * Y0[e + 1] + rng.normal(0, 0.0015, (n, 3))
        u = np.rint(p[:, 0] * cam["fx"] / p[:, 2] + cam["cx"]).astype(np.int64); v = np.rint(p[:, 1] * cam["fy"] / p[:, 2] + cam["cy"]).astype(np.int64)
        ok = (u >= 0) & (u < cam["cols"]) & (v >= 0) & (v < cam["rows"])
        depth = np.full(cam["rows"] * cam["cols"], 65535, dtype=np.int64)
        np.minimum.at(depth, v[ok] * cam["cols"] + u[ok], np.rint(p[ok, 2] * 1000.0).astype(np.int64))
        mask = ((depth != 65535).astype(np.uint8) * 255).reshape(cam["rows"], cam["cols"])
        depth[depth == 65535] = 1500
        depth = depth.astype(np.uint16).reshape(cam["rows"], cam["cols"])
        c4 = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        _CROSS["r"] = ((R.Cam(depth, mask, cam=c4), R.Cam(depth, mask, cam=c4, T=S.TRANSFORMS["identity"] + SHIFT)), Y0)
    return _CROSS["r"]


def pctx(painter_min):
    return make_ctx({"TDLO_RIG_BATCH_MIN": 1, "TDLO_ESTEP2": 0, "TDLO_RIG_PAINTER_MIN": painter_min}, max_frames=4, max_points=1 << 15, max_nodes=64)


def four_trackers(ctx, switch=True):
    """Three trackers on the rope of rope_rigs, the fourth on the crossing rope."""
    from trackdlo_amd import synth
    tr = make_trackers(ctx, 3)
    _, Y0 = crossing_rig()
    tr.append(B_.trackdlo(*targs(), ctx=ctx, slot=3))
    tr[3].initialize_nodes(Y0); tr[3].initialize_geodesic_coord(synth.geodesic_coord(Y0))
    if switch:
        for t in tr:
            t.set_rig_self_occlusion(RIG_TO_CAM, 2, WIDTH)
    return tr


def frames_of(step):
    rigs = rope_rigs()
    return [rigs[(i + step) % 4] for i in range(3)] + [crossing_rig()[0]]


def by_hand(B, ctx, t, slot, cams, bc):
    """One frame of one tracker from the single calls: rig_to_cloud, visibility_prepass, the host statement, extend_visible_nodes, tracking_step."""
    Y = t.get_tracking_result().copy()
    coord = t._coord
    _, n, nraw = ctx.rig_to_cloud(slot, bc, S.LEAF, fetch=False)
    dist, _, _ = ctx.visibility_prepass(slot, Y, t._thr, D_VIS, coord)
    rows, cols = cams[0].depth.shape
    vis = B.rig_self_occlusion_visible(Y, [c.cam for c in cams], RIG_TO_CAM, rows, cols, WIDTH, dist, t._thr)
    ext = B.extend_visible_nodes(vis, coord, D_VIS, M)
    t.tracking_step(None, vis, ext)
    return vis, ext, n, nraw


def hand_twins(B, ctx):
    from trackdlo_amd import synth
    tr = four_trackers(ctx, switch=False)
    P = synth.LAUNCH_PARAMS
    for i, t in enumerate(tr):
        t._thr = P["visibility_threshold"]
        t._coord = synth.geodesic_coord(crossing_rig()[1] if i == 3 else synth.nodes(M))
    return tr


@pytest.mark.parametrize("painter_min,route", [(1, 0), (1 << 20, 1)], ids=["kernel", "host statement"])
def test_the_batch_tracker_call_against_twins_stepped_by_hand(B, painter_min, route):
    xa, xb = pctx(painter_min), pctx(painter_min)
    try:
        ta, tb = four_trackers(xa), hand_twins(B, xb)
        sizes = []
        for step in range(3):
            fr = frames_of(step)
            bc = [S.binding_cams(B, cams) for cams in fr]
            before = xa.rig_painter_route_counts()
            codes, vis, ext, n, nraw = B.frames_from_rig_batch(ta, bc, S.LEAF, D_VIS)
            moved = [a - b for a, b in zip(xa.rig_painter_route_counts(), before)]
            assert codes == [0] * 4 and moved[route] == 8 and moved[1 - route] == 0, (step, codes, moved)
            for i in range(4):
                v1, e1, n1, nraw1 = by_hand(B, xb, tb[i], i, fr[i], bc[i])
                assert (n1, nraw1) == (n[i], nraw[i]) and np.array_equal(v1, vis[i]) and np.array_equal(e1, ext[i]), (step, i, v1, vis[i])
                a, b = state(ta[i]), state(tb[i])
                assert same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], (step, i, a[1], b[1], a[2], b[2])
            sizes.append(len(vis[3]))
        assert xb.rig_painter_route_counts() == [0, 0]
    finally:
        xa.close(); xb.close()


def test_both_routes_and_the_single_call_give_the_same_sets(B):
    """frames_from_rig_batch under TDLO_RIG_PAINTER_MIN = 1 and large, and frame_from_rig per tracker under both: the same sets, nodes and sigma2; the jobs
    counted on different counters."""
    xs = [pctx(1), pctx(1 << 20), pctx(1), pctx(1 << 20)]
    try:
        tr = [four_trackers(x) for x in xs]
        for step in range(2):
            fr = frames_of(step)
            bc = [S.binding_cams(B, cams) for cams in fr]
            out = [B.frames_from_rig_batch(tr[k], bc, S.LEAF, D_VIS) for k in (0, 1)]
            single = [[tr[k][i].frame_from_rig(bc[i], S.LEAF, D_VIS) for i in range(4)] for k in (2, 3)]
            for i in range(4):
                for k in (0, 1):
                    assert np.array_equal(out[k][1][i], single[k][i][0]) and np.array_equal(out[k][2][i], single[k][i][1]), (step, i, k)
                    assert (out[k][3][i], out[k][4][i]) == single[k][i][2:]
                assert np.array_equal(out[0][1][i], out[1][1][i]) and np.array_equal(out[0][2][i], out[1][2][i]), (step, i)
                states = [state(tr[k][i]) for k in range(4)]
                for s in states[1:]:
                    assert same_bits(s[0], states[0][0]) and s[1] == states[0][1], (step, i)
        assert [x.rig_painter_route_counts() for x in xs] == [[16, 0], [0, 16], [16, 0], [0, 16]]
    finally:
        for x in xs:
            x.close()


def test_the_switch_takes_the_painted_over_node_away(B):
    """The reason the feature exists: on the crossing rope the tracker with the switch on gets a smaller visible set than the one with it off."""
    xa, xb = pctx(1), pctx(1)
    try:
        on, off = four_trackers(xa), four_trackers(xb, switch=False)
        bc = [S.binding_cams(B, cams) for cams in frames_of(0)]
        a = B.frames_from_rig_batch(on, bc, S.LEAF, D_VIS)
        b = B.frames_from_rig_batch(off, bc, S.LEAF, D_VIS)
        assert a[0] == b[0] == [0] * 4
        assert set(a[1][3]) < set(b[1][3]) and 24 in b[1][3] and 24 not in a[1][3]            # node 24 = (0, 0, 0.605), under the crossing
        for i in range(3):
            assert set(a[1][i]) <= set(b[1][i])
        assert xb.rig_painter_route_counts() == [0, 0]
    finally:
        xa.close(); xb.close()


def test_a_rig_of_another_camera_count_and_the_single_switch_are_refused(B):
    xa = pctx(1)
    try:
        tr = four_trackers(xa)
        fr = frames_of(0)
        bc = [S.binding_cams(B, cams) for cams in fr]
        assert B.frames_from_rig_batch(tr, bc, S.LEAF, D_VIS)[0] == [0] * 4
        states = [state(t) for t in tr]
        clouds = [xa.get_cloud(i) for i in range(4)]
        counters = (xa.rig_painter_route_counts(), xa.rig_batch_route_counts(), xa.rig_route_counts())

        def untouched():
            for i in range(4):
                now = state(tr[i])
                assert same_bits(now[0], states[i][0]) and now[1] == states[i][1] and same_bits(xa.get_cloud(i), clouds[i]), i
            assert (xa.rig_painter_route_counts(), xa.rig_batch_route_counts(), xa.rig_route_counts()) == counters
        one_cam = [bc[0], bc[1], S.binding_cams(B, fr[2][:1]), bc[3]]
        with pytest.raises(B.TdloError) as e:
            B.frames_from_rig_batch(tr, one_cam, S.LEAF, D_VIS)
        assert e.value.code == B.TDLO_E_INVALID
        untouched()
        with pytest.raises(B.TdloError) as e:
            tr[2].frame_from_rig(S.binding_cams(B, fr[2][:1]), S.LEAF, D_VIS)
        assert e.value.code == B.TDLO_E_INVALID
        untouched()
        # both switches on one tracker: the single switch's refusal stands
        proj = np.zeros((3, 4)); proj[0, 0] = proj[1, 1] = 600.0; proj[0, 2] = 320.0; proj[1, 2] = 240.0; proj[2, 2] = 1.0
        tr[1].set_self_occlusion(proj, 10)
        for call in (lambda: B.frames_from_rig_batch(tr, bc, S.LEAF, D_VIS), lambda: tr[1].frame_from_rig(bc[1], S.LEAF, D_VIS)):
            with pytest.raises(B.TdloError) as e:
                call()
            assert e.value.code == B.TDLO_E_INVALID
        untouched()
        # the rig switch off again: K no longer matters
        tr[1].set_self_occlusion(None)
        tr[2].set_rig_self_occlusion(None, 0)
        assert B.frames_from_rig_batch(tr, one_cam, S.LEAF, D_VIS)[0] == [0] * 4
        assert xa.rig_painter_route_counts()[0] == counters[0][0] + 6
    finally:
        xa.close()
