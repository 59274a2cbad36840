"""tdlo_cell_occlusion_batch and tdlo_tracker_frames_from_shared_cloud_occluded_batch on the device, against the statement (tests/cell_painter_ref.py, the
scenes of tests/cell_painter_scenes.py with the verdicts the CPU tests use): every scene alone and the batches in both orders, in sets and both word arrays,
with route counters 57 / 58 in every case; one context through growing and shrinking calls; whole-call refusals; the tracker call against the composition
tdlo_cloud_assign_visibility + tdlo_cell_occlusion_visible + tdlo_extend_visible_nodes + tdlo_tracker_tracking_step_batch made by hand on a twin context, on
both routes (TDLO_CELL_PAINTER_MIN is read when a context is made: 0 and a huge value, each in a child process of its own); what the call changes against
tdlo_tracker_frames_from_shared_cloud_batch; the switch refusal; a rope that owns no point and still hides another's node.

Run as a program (`python tests/test_cell_painter_gpu.py F`) this file is the child: the tracker sequence of F ropes under the TDLO_CELL_PAINTER_MIN it finds."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from test_prepass_gpu import make_ctx
from test_assign_gpu import shared_trackers
import assign_ref as AR
import cell_painter_scenes as CS

pytestmark = pytest.mark.gpu
VIEW_CAM, VIEW_W, D_MAX, D_VIS = (500.0, 500.0, 0.0, 0.0), 10, 0.02, 0.06
HUGE = 1 << 40


def same(got, want):
    return len(got[0]) == len(want[0]) and all(np.array_equal(g, w) for g, w in zip(got[0], want[0])) and np.array_equal(got[1], want[1]) \
        and np.array_equal(got[2], want[2])


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx(max_frames=2, max_points=1024, max_nodes=64)
    yield c
    c.close()


def run_batch(c, group):
    """One call on the cells of `group`; sets and words against the reference, counter 57 by the sum of K, counter 58 by nothing."""
    before = c.cell_painter_route_counts()
    s0 = group[0][0]
    vis, seen, hidden = c.cell_occlusion_batch([e[0].cell() for e in group], s0.rows, s0.cols, words=True)
    for i, (s, rv, rs, rh, per) in enumerate(group):
        assert same((vis[i], seen[i], hidden[i]), (rv, rs, rh)), s.name
    assert c.cell_painter_route_counts() == [before[0] + sum(e[0].K for e in group), before[1]]
    plain = c.cell_occlusion_batch([e[0].cell() for e in group], s0.rows, s0.cols)
    assert all(same((plain[i], 0, 0), (e[1], 0, 0)) for i, e in enumerate(group))


@pytest.mark.parametrize("i", range(len(CS.scenes())), ids=[s[0].name for s in CS.scenes()])
def test_scene(ctx, i):
    run_batch(ctx, [CS.scenes()[i]])


def test_largest_cell(ctx):
    run_batch(ctx, [CS.largest()])


@pytest.mark.parametrize("key", ["C=1", "C=2", "C=33"])
def test_batches_in_both_orders(ctx, key):
    group = CS.batches()[key]
    run_batch(ctx, group)
    run_batch(ctx, group[::-1])


def test_one_context_through_growing_and_shrinking_calls():
    c = make_ctx(max_frames=2, max_points=1024, max_nodes=64)
    try:
        one = [CS.scenes()[0]]
        for group in (one, CS.batches()["C=33"], [CS.largest()], one):
            run_batch(c, group)
    finally:
        c.close()


def test_whole_call_refusals_touch_neither_outputs_nor_counters(ctx):
    from trackdlo_amd import binding as B
    import ctypes as C
    good, other = CS.scenes()[0][0], CS.scenes()[5][0]
    before = ctx.cell_painter_route_counts()
    big = np.zeros((1024, 3)); big[:, 2] = 1.0
    Y, d = good.ropes[0][0], good.ropes[0][1]
    bad_cells = [(good.ropes, good.cams, good.mats, 0), (good.ropes, good.cams, good.mats, 256), (good.ropes, [], None, 5), (good.ropes, [CS.CAM] * 65, None, 5),
                 ([], good.cams, None, 5), ([(np.zeros((1025, 3)), np.zeros(1025), 0.008)], good.cams, None, 5), ([(np.zeros((0, 3)), np.zeros(0), 0.008)], good.cams, None, 5),
                 ([(big, np.zeros(1024), 0.008)] * 16 + [(Y[:1], d[:1], 0.008)], good.cams, None, 5), (good.ropes, [(0.0, 500.0, 1.0, 1.0)], None, 5),
                 (good.ropes, [(500.0, np.inf, 1.0, 1.0)], None, 5)]
    for cell in bad_cells:
        with pytest.raises(B.TdloError):
            ctx.cell_occlusion_batch([other.cell(), cell], 480, 640)                 # a good cell in front: the call is refused as a whole
    for rows, cols in ((0, 640), (8193, 640), (480, 0), (480, 8193)):
        with pytest.raises(B.TdloError):
            ctx.cell_occlusion_batch([good.cell()], rows, cols)
    with pytest.raises(B.TdloError):
        ctx.cell_occlusion_batch([], 480, 640)
    with pytest.raises(B.TdloError):
        ctx.cell_occlusion_batch([good.cell()] * 1025, 480, 640)
    # the outputs of a refused call, seen from outside: a good cell and a bad one, every array filled with a pattern beforehand
    rt0, F0, N0, Ms0, k0 = B._cell_ropes(good.ropes); rt1, F1, N1, Ms1, k1 = B._cell_ropes(other.ropes)
    ct, K = B._painter_cams(good.cams)
    tab = (B.CellC * 2)()
    for q, (rt, F, w) in zip(tab, ((rt0, F0, 5), (rt1, F1, 0))):
        q.ropes = C.cast(rt, C.c_void_p).value; q.F = F; q.cams = C.cast(ct, C.c_void_p).value; q.rig_to_cam = None; q.K = K; q.dlo_pixel_width = w
    vis = np.full((F0 + F1, 16), -7, dtype=np.int32); nv = np.full(F0 + F1, -7, dtype=np.int32); sw = np.full(64, 0xABCD, dtype=np.uint32); hw = sw.copy()
    assert ctx.lib.tdlo_cell_occlusion_batch(ctx.h, 2, C.cast(tab, C.c_void_p), 480, 640, B._ptr(vis), B._ptr(nv), B._ptr(sw), B._ptr(hw)) == B.TDLO_E_INVALID
    assert (vis == -7).all() and (nv == -7).all() and (sw == 0xABCD).all() and (hw == 0xABCD).all()
    assert ctx.cell_painter_route_counts() == before
    run_batch(ctx, [CS.scenes()[0]])                                                   # and the context serves the next call


# ---- the tracker call ---------------------------------------------------------------------------------------------------------------------------------
def crossing_cell(F, M=45, frames=5, n_each=750, seed=4):
    """F ropes of M nodes in pairs: rope 2 p + 1 crosses rope 2 p in the image, every rope 3 cm further from the camera than the one before it; the pairs
    lie side by side in the image (83 rows apart under VIEW_CAM), not under one another.  And a drifting shared cloud per frame."""
    rng = np.random.default_rng(700 + seed)
    s = np.arange(M) * 0.012
    base = []
    for k in range(F):
        z = 0.60 + 0.03 * k
        y = (0.2 + 0.3 * s) if k % 2 == 0 else (0.36 - 0.3 * s)
        base.append(np.stack([(0.1 + s) * (z / 0.6), (y + 0.1 * (k // 2)) * (z / 0.6), z + 0 * s], axis=1))      # (the picture of the pair at z = 0.6, further away)
    coords = [np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(b, axis=0), axis=1))]) for b in base]
    clouds = []
    for fr in range(frames):
        pts = []
        for k, b in enumerate(base):
            t = rng.uniform(0, M - 1, n_each); i0 = np.floor(t).astype(int); w = (t - i0)[:, None]
            c = b[i0] * (1 - w) + b[np.minimum(i0 + 1, M - 1)] * w
            pts.append(c + np.array([0.0005 * fr, 0.0003 * fr * (1 - 2 * (k % 2)), 0.0]) + rng.normal(0, 8e-4, c.shape))
        X = np.concatenate(pts)
        clouds.append(np.asfortranarray(X[rng.permutation(len(X))]))
    return [np.asfortranarray(b) for b in base], coords, clouds


def by_hand(cb, tb, coords, src, thr):
    """The composition on the twin context: (codes, [visible], [extended], n_each)."""
    from trackdlo_amd import binding as B
    F, M = len(tb), tb[0].M
    Ys = [t.get_tracking_result() for t in tb]
    n_each, _, dist, _, _ = cb.cloud_assign_visibility(src, list(enumerate(Ys)), D_MAX, thr, D_VIS, coords)
    vis = B.cell_occlusion_visible([(Ys[i], dist[i], thr) for i in range(F)], [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W)
    ext = [B.extend_visible_nodes(vis[i], coords[i], D_VIS, M) for i in range(F)]
    codes = [B.TDLO_E_EMPTY if (n_each[i] == 0 or len(ext[i]) == 0) else 0 for i in range(F)]
    live = [i for i in range(F) if codes[i] == 0]
    if live:
        for i, r in zip(live, B.tracking_step_batch([tb[i] for i in live], [vis[i] for i in live], [ext[i] for i in live])):
            codes[i] = r
    for i in range(F):
        if n_each[i] == 0:
            vis[i] = vis[i][:0]; ext[i] = ext[i][:0]                                   # (a tracker without a cloud reports no set)
    return codes, vis, ext, n_each


def tracker_sequence(F):
    """Five frames of F crossing ropes: the call against the composition by hand, under the TDLO_CELL_PAINTER_MIN of this process."""
    from trackdlo_amd import binding as B, synth
    M, thr = 45, synth.LAUNCH_PARAMS["visibility_threshold"]
    kernels = int(os.environ["TDLO_CELL_PAINTER_MIN"]) == 0
    Y0, coords, clouds = crossing_cell(F, M)
    ca = make_ctx({"TDLO_ESTEP2": 0}, max_frames=F + 1, max_points=4096, max_nodes=64); cb = make_ctx({"TDLO_ESTEP2": 0}, max_frames=F + 1, max_points=4096, max_nodes=64)
    try:
        ta, tb = shared_trackers(ca, Y0, coords, M), shared_trackers(cb, Y0, coords, M)
        fewer = 0
        for fr, X in enumerate(clouds):
            ca.set_cloud(F, X); cb.set_cloud(F, X)
            before = ca.cell_painter_route_counts()
            codes, vis, ext, n_each = B.frames_from_shared_cloud_occluded_batch(ta, F, D_MAX, D_VIS, [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W)
            assert ca.cell_painter_route_counts() == [before[0] + (1 if kernels else 0), before[1] + (0 if kernels else 1)]
            hcodes, hvis, hext, hn = by_hand(cb, tb, coords, F, thr)
            assert codes == hcodes == [0] * F and n_each == hn and min(n_each) > 300, (fr, codes, hcodes, n_each, hn)
            for i in range(F):
                assert np.array_equal(vis[i], hvis[i]) and np.array_equal(ext[i], hext[i]) and len(vis[i]) > 0, (fr, i)
                assert np.array_equal(AR.bits(ta[i].get_tracking_result()), AR.bits(tb[i].get_tracking_result())), (fr, i)
                assert ta[i].get_sigma2() == tb[i].get_sigma2()
                assert [s["iters"] for s in ta[i].last_stats] == [s["iters"] for s in tb[i].last_stats]
                fewer += len(vis[i]) < M
        assert fewer >= 5                                                            # a rope under a crossing loses nodes in every frame
    finally:
        ca.close(); cb.close()


@pytest.mark.parametrize("route", ["kernels", "host"])
@pytest.mark.parametrize("F", [2, 4])
def test_tracker_call_equals_the_composition_by_hand(F, route):
    env = dict(os.environ, TDLO_CELL_PAINTER_MIN="0" if route == "kernels" else str(HUGE))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(F)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-4000:]


def pair(min_value=0):
    from trackdlo_amd import synth
    Y0, coords, clouds = crossing_cell(2)
    c = make_ctx({"TDLO_ESTEP2": 0, "TDLO_CELL_PAINTER_MIN": min_value}, max_frames=3, max_points=4096, max_nodes=64)
    return c, shared_trackers(c, Y0, coords, 45), Y0, coords, clouds, synth.LAUNCH_PARAMS["visibility_threshold"]


def test_the_feature_shows():
    """The plain shared-cloud call reports the nodes of the lower rope under the crossing as visible; the new call does not."""
    from trackdlo_amd import binding as B
    import cell_painter_ref as CR
    c, trk, Y0, coords, clouds, thr = pair()
    c2, trk2, *_ = pair()
    try:
        under = CS.hidden_set(CR.cell_verdict([(Y, np.zeros(45), thr) for Y in Y0], [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W)[3][0])
        assert under and all(n >= 45 for n in under)                                 # nodes of rope 1, which lies 3 cm behind rope 0
        c.set_cloud(2, clouds[0]); c2.set_cloud(2, clouds[0])
        _, plain, _, _ = B.frames_from_shared_cloud_batch(trk, 2, D_MAX, D_VIS)
        _, occl, _, _ = B.frames_from_shared_cloud_occluded_batch(trk2, 2, D_MAX, D_VIS, [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W)
        assert {n - 45 for n in under} <= set(plain[1].tolist()) and not ({n - 45 for n in under} & set(occl[1].tolist()))
        assert np.array_equal(plain[0], occl[0]) and set(occl[1].tolist()) == set(plain[1].tolist()) - {n - 45 for n in under}
    finally:
        c.close(); c2.close()


def test_a_tracker_with_a_self_occlusion_switch_is_refused_and_nothing_is_touched():
    from trackdlo_amd import binding as B
    import rig_painter_ref as PR
    c, trk, Y0, coords, clouds, thr = pair()
    try:
        c.set_cloud(2, clouds[0])
        keep = [c.get_cloud(s).copy() for s in (0, 1)]
        for switch in (lambda t: t.set_self_occlusion(PR.proj_of(VIEW_CAM), VIEW_W), lambda t: t.set_rig_self_occlusion(None, 1, VIEW_W)):
            switch(trk[1])
            before = (c.cell_painter_route_counts(), c.assign_route_counts())
            codes = B.frames_from_shared_cloud_occluded_batch(trk, 2, D_MAX, D_VIS, [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W, check=False)[0]
            assert c.lib.tdlo_last_error(c.h) and codes == [0, 0]
            with pytest.raises(B.TdloError):
                B.frames_from_shared_cloud_occluded_batch(trk, 2, D_MAX, D_VIS, [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W)
            assert (c.cell_painter_route_counts(), c.assign_route_counts()) == before
            for i in (0, 1):
                assert np.array_equal(trk[i].get_tracking_result(), Y0[i])
                assert np.array_equal(c.get_cloud(i), keep[i])
            trk[1].set_self_occlusion(None); trk[1].set_rig_self_occlusion(None, 0)
        # what the cell test refuses is refused here as well
        for bad in (dict(w=0), dict(rows=0), dict(cams=[])):
            with pytest.raises(B.TdloError):
                B.frames_from_shared_cloud_occluded_batch(trk, 2, D_MAX, D_VIS, bad.get("cams", [VIEW_CAM]), None, bad.get("rows", CS.ROWS), CS.COLS, bad.get("w", VIEW_W))
        assert B.frames_from_shared_cloud_occluded_batch(trk, 2, D_MAX, D_VIS, [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W)[0] == [0, 0]
    finally:
        c.close()


@pytest.mark.parametrize("min_value", [0, HUGE])
def test_a_rope_that_owns_no_point_still_hides_another_ropes_node(min_value):
    """Rope 1 is pulled half way to the camera along its rays: the same pixels, in front of rope 0 now, and 30 cm from every point of the cloud."""
    from trackdlo_amd import binding as B
    c, trk, Y0, coords, clouds, thr = pair(min_value)
    cb, tb, *_ = pair(min_value)
    try:
        near = np.asfortranarray(Y0[1] * 0.5)
        for t in (trk[1], tb[1]):
            t.initialize_nodes(near)
        c.set_cloud(2, clouds[0]); cb.set_cloud(2, clouds[0])
        s2 = trk[1].get_sigma2()
        near_enough = cb.cloud_assign_visibility(2, [(0, Y0[0]), (1, near)], D_MAX, thr, D_VIS, coords)[3][0]      # the pre-pass's set of rope 0
        codes, vis, ext, n_each = B.frames_from_shared_cloud_occluded_batch(trk, 2, D_MAX, D_VIS, [VIEW_CAM], None, CS.ROWS, CS.COLS, VIEW_W, check=False)
        hcodes, hvis, hext, hn = by_hand(cb, tb, coords, 2, thr)
        assert codes == hcodes == [0, B.TDLO_E_EMPTY] and n_each == hn and n_each[1] == 0 and n_each[0] > 300
        assert np.array_equal(trk[1].get_tracking_result(), near) and trk[1].get_sigma2() == s2
        assert np.array_equal(vis[0], hvis[0]) and np.array_equal(ext[0], hext[0]) and len(vis[1]) == 0
        assert 0 < len(vis[0]) < len(near_enough) and set(vis[0].tolist()) < set(near_enough.tolist())      # rope 1 hid nodes of rope 0
        assert np.array_equal(AR.bits(trk[0].get_tracking_result()), AR.bits(tb[0].get_tracking_result())) and trk[0].get_sigma2() == tb[0].get_sigma2()
    finally:
        c.close(); cb.close()


if __name__ == "__main__":
    tracker_sequence(int(sys.argv[1]))
    print("OK")
