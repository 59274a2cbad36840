"""tdlo_tracker_tracking_step_batch / tdlo_tracker_frame_batch: trackdlo::tracking_step for F trackers of one context in one call.

The scenes are those of test_parity_gpu.py::_tracking_step_case -- synth.scene(N = 3000, M = 30, config = 20), the five occlusion states plus "all", the
pre-processing registration's H injected.  Bit-for-bit comparisons run on contexts made under TDLO_ESTEP2=0 (both sides k_estep); the comparison with
oracle.Tracker runs on a default context at the gates of _tracking_step_case."""
import ctypes as C

import numpy as np
import pytest

from test_prepass_gpu import make_ctx

pytestmark = pytest.mark.gpu
M, N = 30, 3000
OCCL = [None, (0.45, 0.5), (0.35, 0.65), (0.0, 0.3), (0.7, 1.0), (0.0, 0.2, 0.8, 1.0)]      # all, minor, mid, head, tail, both ends
D_VIS = 0.06


def targs(**over):
    from trackdlo_amd import synth
    P = dict(synth.LAUNCH_PARAMS, **over)
    return (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"],
            P["lle_weight"])


def same_kernel_ctx(frames=8):
    return make_ctx({"TDLO_ESTEP2": 0}, max_frames=frames, max_points=1 << 14, max_nodes=64)


_CASES = {}


def case(oracle, occl, frame=0):
    """(X, vis, vext, Hpre) of one occlusion state, as _tracking_step_case builds them; computed once."""
    from trackdlo_amd import synth
    key = (occl, frame)
    if key in _CASES:
        return _CASES[key]
    Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
    if occl is None:
        X, _, _ = synth.scene(N, M, config=20, frame=frame); vis = np.arange(M, dtype=np.int32)
    elif len(occl) == 2:
        X, _, vis = synth.scene(N, M, config=20, frame=frame, occlude=occl)
    else:
        X, _, _ = synth.scene(N, M, config=20, frame=frame)
        s = np.linspace(0, 1, M)
        vis = np.nonzero((s > occl[1]) & (s < occl[2]))[0].astype(np.int32)
        d = np.linalg.norm(X[:, None, :] - Y0[None, vis, :], axis=2).min(axis=1)
        X = np.asfortranarray(X[d < 0.012])
    vext = synth.extend_visible(vis, M, coord)
    Lg = oracle.calc_lle_weights(Y0[vext], 6)
    Hpre = (np.eye(len(vext)) - Lg).T @ (np.eye(len(vext)) - Lg)
    _CASES[key] = (X, vis, vext, Hpre)
    return _CASES[key]


def make_trackers(ctx, n, **kw):
    from trackdlo_amd import binding as B, synth
    Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
    out = []
    for i in range(n):
        t = B.trackdlo(*targs(), ctx=ctx, slot=i, **kw)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        out.append(t)
    return out


def state(t):
    return (t.get_tracking_result().copy(), t.get_sigma2(), t.get_guide_nodes().copy(), t.get_correspondence_pairs().copy())


def counts(t):
    return [(s["iters"], s["converged"], s["n_kept"], s["status"]) for s in t.last_stats]


def assert_same_state(a, b, label):
    for x, y, what in zip(a, b, ("nodes", "sigma2", "guide nodes", "priors")):
        if what == "sigma2":
            assert x == y, (label, what, x, y)
        else:
            assert x.shape == y.shape, (label, what, x.shape, y.shape)
            np.testing.assert_array_equal(x, y, err_msg=f"{label}: {what}")


def test_six_occlusion_states_in_one_batch_equal_six_single_trackers(oracle):
    """n_vis_ext differs from tracker to tracker (several pre-processing groups, a main batch whose frames disagree about the visibility weights); three
    consecutive frames, so state and last_iters carry over."""
    from trackdlo_amd import binding as B
    ca, cb = same_kernel_ctx(), same_kernel_ctx()
    try:
        ta, tb = make_trackers(ca, 6), make_trackers(cb, 6)
        cs = [case(oracle, o) for o in OCCL]
        assert len({len(c[2]) for c in cs}) >= 4
        for frame in range(3):
            for i, c in enumerate(cs):
                ca.set_cloud(i, c[0])
            rcs = B.tracking_step_batch(ta, [c[1] for c in cs], [c[2] for c in cs], H_pre=[c[3] for c in cs])
            assert rcs == [0] * 6
            for i, c in enumerate(cs):
                tb[i].tracking_step(c[0], c[1], c[2], H_pre=c[3])
                assert_same_state(state(ta[i]), state(tb[i]), f"frame {frame}, tracker {i}")
                assert counts(ta[i]) == counts(tb[i]), (frame, i, counts(ta[i]), counts(tb[i]))
                assert ta[i].last_stats[1]["iters"] > 0
    finally:
        ca.close(); cb.close()


def test_six_occlusion_states_against_the_oracle(oracle):
    """The same batch on a default context against oracle.Tracker, at the gates of _tracking_step_case: 1e-5 m, 1e-3 in sigma2, iteration counts exact."""
    from trackdlo_amd import binding as B, synth
    Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
    ctx = B.Context(device=0, max_frames=8, max_points=1 << 14, max_nodes=64)
    try:
        trk = make_trackers(ctx, 6)
        cs = [case(oracle, o) for o in OCCL]
        refs = []
        for _ in cs:
            r = oracle.Tracker(*targs()); r.initialize_nodes(Y0); r.initialize_geodesic_coord(coord)
            refs.append(r)
        for i, c in enumerate(cs):
            ctx.set_cloud(i, c[0])
        for step in range(2):
            B.tracking_step_batch(trk, [c[1] for c in cs], [c[2] for c in cs], H_pre=[c[3] for c in cs])
            for i, (c, ref, t) in enumerate(zip(cs, refs, trk)):
                ref.tracking_step(c[0], c[1], c[2], H_pre=c[3])
                assert t.last_stats[0]["iters"] == ref.stats_pre.iters and t.last_stats[1]["iters"] == ref.stats_main.iters, (step, i)
                np.testing.assert_allclose(t.get_guide_nodes(), ref.get_guide_nodes(), rtol=0, atol=1e-5)
                kp, kr = t.get_correspondence_pairs(), ref.get_correspondence_pairs()
                assert kp.shape == kr.shape
                np.testing.assert_allclose(kp, kr, rtol=0, atol=1e-5)
                np.testing.assert_allclose(t.get_tracking_result(), ref.get_tracking_result(), rtol=0, atol=1e-5)
                assert abs(t.get_sigma2() - ref.get_sigma2()) <= 1e-3 * ref.get_sigma2()
    finally:
        ctx.close()


def test_eight_all_visible_trackers_fork_the_streams(oracle):
    """Eight trackers on eight different frames: one pre-processing group of eight, two stream groups; no H injected (the library's own H)."""
    from trackdlo_amd import binding as B
    ca, cb = same_kernel_ctx(), same_kernel_ctx()
    try:
        ta, tb = make_trackers(ca, 8), make_trackers(cb, 8)
        v = np.arange(M, dtype=np.int32)
        for step in range(2):
            Xs = [case(oracle, None, frame=8 * step + i)[0] for i in range(8)]
            for i in range(8):
                ca.set_cloud(i, Xs[i])
            assert B.tracking_step_batch(ta, [v] * 8, [v] * 8) == [0] * 8
            for i in range(8):
                tb[i].tracking_step(Xs[i], v, v)
                assert_same_state(state(ta[i]), state(tb[i]), f"step {step}, tracker {i}")
                assert counts(ta[i]) == counts(tb[i])
        assert len({state(t)[0].tobytes() for t in ta}) == 8
    finally:
        ca.close(); cb.close()


def test_one_tracker_is_the_single_call_and_a_batch_leaves_the_context_clean(oracle):
    """F = 1 equals tdlo_tracker_tracking_step; and a single step behind a batch equals the same step in a sequence of single calls only: the context's
    pair / hint state was left as after a single step."""
    from trackdlo_amd import binding as B
    ca, cb = same_kernel_ctx(), same_kernel_ctx()
    try:
        ta, tb = make_trackers(ca, 3), make_trackers(cb, 3)
        cs = [case(oracle, o) for o in (None, (0.35, 0.65), None)]
        # F = 1
        ca.set_cloud(0, cs[0][0])
        assert B.tracking_step_batch(ta[:1], [cs[0][1]], [cs[0][2]], H_pre=[cs[0][3]]) == [0]
        tb[0].tracking_step(cs[0][0], cs[0][1], cs[0][2], H_pre=cs[0][3])
        assert_same_state(state(ta[0]), state(tb[0]), "F = 1"); assert counts(ta[0]) == counts(tb[0])
        # a batch of three, then single steps on each of its trackers (all visible: the paired route; hidden nodes: the route launched ahead)
        for i, c in enumerate(cs):
            ca.set_cloud(i, c[0])
        B.tracking_step_batch(ta, [c[1] for c in cs], [c[2] for c in cs], H_pre=[c[3] for c in cs])
        for i, c in enumerate(cs):
            tb[i].tracking_step(c[0], c[1], c[2], H_pre=c[3])
        for i, c in enumerate(cs):
            X2 = case(oracle, OCCL[0] if len(c[2]) == M else (0.35, 0.65), frame=1)[0]
            ta[i].tracking_step(X2, c[1], c[2], H_pre=c[3])
            tb[i].tracking_step(X2, c[1], c[2], H_pre=c[3])
            assert_same_state(state(ta[i]), state(tb[i]), f"single behind the batch, tracker {i}"); assert counts(ta[i]) == counts(tb[i])
    finally:
        ca.close(); cb.close()


def test_frame_batch_equals_prepass_and_step_per_tracker(oracle):
    """tdlo_tracker_frame_batch against tdlo_visibility_prepass + tdlo_tracker_tracking_step per tracker: one tracker with the self-occlusion switch on, one
    whose cloud lies 1 m from its nodes (TDLO_E_EMPTY, untouched), the others unchanged by either."""
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    cam = synth.CAMERA
    proj = np.array([[cam["fx"], 0, cam["cx"], 0], [0, cam["fy"], cam["cy"], 0], [0, 0, 1, 0]], dtype=np.float64)
    width = 12
    ca, cb = same_kernel_ctx(), same_kernel_ctx()
    try:
        ta, tb = make_trackers(ca, 5), make_trackers(cb, 5)
        ta[1].set_self_occlusion(proj, width)
        Xs = [case(oracle, None)[0], case(oracle, None, frame=1)[0], case(oracle, (0.35, 0.65))[0], np.asfortranarray(case(oracle, None)[0] + [0.0, 0.0, 1.0]),
              case(oracle, (0.0, 0.3))[0]]
        for step in range(2):
            for i in range(5):
                ca.set_cloud(i, Xs[i]); cb.set_cloud(i, Xs[i])
            before = state(ta[3])
            codes, vis, ext = B.frame_batch(ta, D_VIS, check=False)
            assert codes == [0, 0, 0, B.TDLO_E_EMPTY, 0], codes
            assert_same_state(state(ta[3]), before, "the tracker without a visible node")
            assert len(vis[3]) == 0 and len(ext[3]) == 0
            for i in (0, 1, 2, 4):
                Y = tb[i].get_tracking_result(); coord = synth.geodesic_coord(synth.nodes(M))
                dist, v, e = cb.visibility_prepass(i, Y, P["visibility_threshold"], D_VIS, coord)
                if i == 1:
                    v = B.self_occlusion_visible(Y, proj, width, dist, P["visibility_threshold"])
                    e = B.extend_visible_nodes(v, coord, D_VIS, M)
                assert np.array_equal(vis[i], v) and np.array_equal(ext[i], e), (step, i)
                tb[i].tracking_step(None, v, e)
                assert_same_state(state(ta[i]), state(tb[i]), f"step {step}, tracker {i}"); assert counts(ta[i]) == counts(tb[i])
        assert len(ext[2]) < M and len(ext[4]) < M
    finally:
        ca.close(); cb.close()


def test_refusals_touch_nothing(oracle):
    """Two trackers on one slot, another num_of_nodes, another beta, mixed precision, an uninitialised tracker: TDLO_E_INVALID, every tracker as before."""
    from trackdlo_amd import binding as B, synth
    ctx = same_kernel_ctx()
    try:
        good = make_trackers(ctx, 2)
        X, vis, vext, H = case(oracle, None)
        for i in range(3):
            ctx.set_cloud(i, X)
        B.tracking_step_batch(good, [vis] * 2, [vext] * 2, H_pre=[H] * 2)
        Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)

        def tracker(args=None, slot=2, init=True, nodes=M, **kw):
            a = list(targs() if args is None else args); a[0] = nodes
            t = B.trackdlo(*a, ctx=ctx, slot=slot, **kw)
            if init:
                Yn = synth.nodes(nodes)
                t.initialize_nodes(Yn); t.initialize_geodesic_coord(synth.geodesic_coord(Yn))
            return t

        bad = {"one slot twice": tracker(slot=1), "num_of_nodes": tracker(nodes=M + 1), "beta": tracker(args=targs(beta=0.36)),
               "precision": tracker(precision=B.PREC_F64), "not initialised": tracker(init=False)}
        for why, t in bad.items():
            trio = good + [t]
            before = [state(x) for x in trio]
            n = t.M
            v3 = [vis, vis, np.arange(n, dtype=np.int32)]
            with pytest.raises(B.TdloError) as e:
                B.tracking_step_batch(trio, v3, v3)
            assert e.value.code == B.TDLO_E_INVALID, why
            with pytest.raises(B.TdloError) as e:
                B.frame_batch(trio, D_VIS)
            assert e.value.code == B.TDLO_E_INVALID, why
            for x, b in zip(trio, before):
                assert_same_state(state(x), b, why)
        # an index list out of range
        with pytest.raises(B.TdloError) as e:
            B.tracking_step_batch(good, [vis] * 2, [vext, np.array([0, M], dtype=np.int32)])
        assert e.value.code == B.TDLO_E_INVALID
        third = tracker()
        assert B.tracking_step_batch(good + [third], [vis] * 3, [vext] * 3, H_pre=[H] * 3) == [0, 0, 0]      # the next valid call
    finally:
        ctx.close()
