"""tdlo_depth_to_cloud_batch / tdlo_tracker_frames_batch (k_cloud_fused_batch): every slot's cloud, n and n_raw are those of the single call on that frame
alone -- compared on uint64 views, so the sign of a zero counts -- whatever else shares the call; tdlo_debug_route_count 32 / 33 in every case.

The scenes are tests/cloud_scenes.py's, the references tests/voxel_ref.py / tests/colour_ref.py.  Contexts are made under TDLO_CLOUD_BATCH_MIN=1 unless said
otherwise, so that a batch of any size takes the batch launch.

One call has one image size and one leaf, and cloud_scenes' catalogue holds its C, F and G scenes at 192 x 256 / 480 x 640 and at three leaves.  The frames of
`border_frames` are therefore BUILT with cloud_scenes' own recipe (cell_scene, fill_runs, the layout search of scene_F_pair, scene G_zero's images) at
480 x 640 for one leaf of 0.25 mm, under the catalogue's names; what each does to the kernel is asserted on the reference's structure alone
(cloud_scenes.route_rule), and the reference is voxel_ref on the frame as built.  The D scenes are the catalogue's own (scene.ref)."""
import functools

import numpy as np
import pytest

import cloud_scenes as S
import colour_ref
import voxel_ref as V
from test_prepass_gpu import make_ctx

pytestmark = pytest.mark.gpu

ROWS, COLS, LEAF_B = 480, 640, 0.00025


def bctx(frames=8, batch_min=1, **env):
    return make_ctx(dict({"TDLO_CLOUD_BATCH_MIN": batch_min}, **env), max_frames=frames, max_points=1 << 15, max_nodes=64)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def image(s):
    return dict(depth=s.depth, mask=s.mask, cam=s.cam)


def reference(s, leaf=None):
    """(X, n_raw) of a frame as built, for the call's leaf."""
    if leaf is None or leaf == s.leaf:
        return s.ref
    return V.voxel_ref(s.points(), None, leaf)


def check_slots(ctx, slots, scenes, res, leaf=None, label=""):
    n, nraw, codes = res
    assert codes == [0] * len(slots), (label, codes)
    for i, (slot, s) in enumerate(zip(slots, scenes)):
        X, n_raw = reference(s, leaf)
        assert (n[i], nraw[i]) == (X.shape[0], n_raw), (label, s.name, n[i], nraw[i], X.shape[0], n_raw)
        assert same_bits(ctx.get_cloud(slot), X), (label, s.name)


# ---- the frames at the borders of the in-LDS sort, 480 x 640, one leaf -------------------------------------------------------------------------
def _layout(name, n, span, leaf, seed):
    """cloud_scenes.layout_scene at 480 x 640."""
    runs = S.fill_runs(n, [], seed, lo=1, hi=9)
    rng = np.random.default_rng(seed + 1)
    cd = 1000 + np.sort(np.concatenate([[0, span], rng.choice(np.arange(1, span), len(runs) - 2, replace=False)]))
    return S.cell_scene(name, ROWS, COLS, runs, seed + 2, cell_depth=cd, leaf=leaf, fx=1e9)


@functools.lru_cache(maxsize=None)
def border_frames():
    """[(scene, route)]: C_1, C_1024, C_1025, C_32704, C_32705, F_rbkb33, G_zero and a frame with an all-zero mask; the routes by the reference's structure."""
    out = [S.cell_scene("C_%d" % n, ROWS, COLS, S.fill_runs(n, [], 200 + n), 300 + n, leaf=LEAF_B) for n in (1, 1024, 1025, S.kFNmax, S.kFNmax + 1)]
    f33 = None
    for span in range(24000, 64001, 8000):           # (the search of cloud_scenes.scene_F_pair: the first span at which rb + kb is 33)
        s = _layout("F_rbkb33", 20000, span, LEAF_B, 640)
        if s.structure["rb"] + s.structure["kb"] == 33:
            f33 = s
            break
    assert f33 is not None
    out.append(f33)
    g = S.get("G_zero")                               # its images under a long lens: x = y = -0.0f, z = 0.0f for the masked zero-depth pixels, as there
    out.append(S.Scene("G_zero", g.depth, g.mask, (1e8, 1e8, g.cam[2], g.cam[3]), LEAF_B, note=g.note))
    rng = np.random.default_rng(5)
    out.append(S.Scene("empty", rng.integers(1, 60000, (ROWS, COLS)).astype(np.uint16), np.zeros((ROWS, COLS), np.uint8), (1e8, 1e8, -0.5, -0.5), LEAF_B))
    for s in out:
        s.depth.setflags(write=False); s.mask.setflags(write=False)
    routes = [S.route_rule(s.structure, s.T) for s in out]
    assert routes == ["taken"] * 4 + ["passed", "passed", "taken", "taken"], routes
    assert out[5].structure["n_raw"] <= S.kFNmax and not out[5].structure["nodown"]          # passed on for its bits alone
    return list(zip(out, routes))


def run_borders(ctx, ctx2, label):
    fr = border_frames()
    scenes = [s for s, _ in fr]
    before, single = ctx.cloud_batch_route_counts(), ctx.cloud_route_counts()
    res = ctx.depth_to_cloud_batch([image(s) for s in scenes], [(i, i, None) for i in range(8)], LEAF_B)
    now = ctx.cloud_batch_route_counts()
    assert [now[0] - before[0], now[1] - before[1]] == [6, 2], (label, before, now)
    assert ctx.cloud_route_counts() == [single[0], single[1] + 2]                            # the two passed-on frames took the single call, which sent them on
    check_slots(ctx, range(8), scenes, res, label=label)
    assert res[0][7] == 0 and res[1][7] == 0                                                 # the empty frame: served, n = 0
    if ctx2 is not None:
        for i, (s, route) in enumerate(fr):
            if route == "passed":
                X, n, nraw = ctx2.depth_to_cloud(0, s.depth, s.mask, *s.cam, LEAF_B)
                assert (n, nraw) == (res[0][i], res[1][i]) and same_bits(X, ctx.get_cloud(i)) and same_bits(X, s.ref[0]), (label, s.name)


def test_smallest_multi_tile_shape_and_single_tile():
    """F = 3 at T = 7 (masked pixels only in the first, only in the last, in alternate tiles): in order, with the slots reversed, into slots that held a larger
    cloud; then F = 3 at T = 1, where a frame's only workgroup is its last."""
    ctx = bctx()
    try:
        scenes = [S.get("D_7_%s" % p) for p in S.D_PLACES]
        assert all(s.T == 7 and s.depth.shape == (149, 191) for s in scenes)
        imgs = [image(s) for s in scenes]
        check_slots(ctx, [0, 1, 2], scenes, ctx.depth_to_cloud_batch(imgs, [(0, 0, None), (1, 1, None), (2, 2, None)], S.LEAF), label="in order")
        assert ctx.cloud_batch_route_counts() == [3, 0]
        check_slots(ctx, [2, 1, 0], scenes, ctx.depth_to_cloud_batch(imgs, [(2, 0, None), (1, 1, None), (0, 2, None)], S.LEAF), label="reversed")
        assert ctx.cloud_batch_route_counts() == [6, 0]
        big = np.asfortranarray(np.random.default_rng(3).random((20000, 3)))
        for slot in (3, 4, 5):
            ctx.set_cloud(slot, big)
        check_slots(ctx, [5, 3, 4], scenes, ctx.depth_to_cloud_batch(imgs, [(5, 0, None), (3, 1, None), (4, 2, None)], S.LEAF), label="over a larger cloud")
        assert ctx.cloud_batch_route_counts() == [9, 0]
        ones = [S.get("D_1_%s" % p) for p in S.D_PLACES]
        assert all(s.T == 1 and s.depth.shape == (63, 65) for s in ones)
        check_slots(ctx, [0, 1, 2], ones, ctx.depth_to_cloud_batch([image(s) for s in ones], [(0, 0, None), (1, 1, None), (2, 2, None)], S.LEAF), label="T = 1")
        assert ctx.cloud_batch_route_counts() == [12, 0] and ctx.cloud_route_counts() == [0, 0]
    finally:
        ctx.close()


def test_borders_of_the_in_lds_sort():
    """F = 8 at 480 x 640: 1, 1024, 1025, 32 704 points served; 32 705 points and rb + kb = 33 passed on; negative zeros; an empty frame served with n = 0."""
    ctx, ctx2 = bctx(), bctx()
    try:
        run_borders(ctx, ctx2, "borders")
    finally:
        ctx.close(); ctx2.close()


def test_a_frame_does_not_depend_on_its_company():
    """One frame's cloud has the same bits for F = 1, 2 and 8, at frame index 0 and F - 1."""
    ctx = bctx()
    try:
        mine = S.get("D_7_alternate")
        others = [S.get("D_7_first"), S.get("D_7_last")]
        imgs = [image(mine)] + [image(s) for s in others]
        served = 0
        for F in (1, 2, 8):
            for at in sorted({0, F - 1}):
                frames = [(f, 0 if f == at else 1 + (f % 2), None) for f in range(F)]
                n, nraw, codes = ctx.depth_to_cloud_batch(imgs, frames, S.LEAF)
                served += F
                assert codes == [0] * F and ctx.cloud_batch_route_counts() == [served, 0]
                assert (n[at], nraw[at]) == (mine.ref[0].shape[0], mine.ref[1]) and same_bits(ctx.get_cloud(at), mine.ref[0]), (F, at)
                for f in range(F):
                    if f != at:
                        assert same_bits(ctx.get_cloud(f), others[f % 2].ref[0]), (F, at, f)
    finally:
        ctx.close()


# ---- one image, several ropes ---------------------------------------------------------------------------------------------------------------------
ROPES = [([[90, 90, 30]], [[130, 255, 255]]), ([[0, 60, 50]], [[10, 255, 255]]), ([[15, 100, 80]], [[40, 255, 255]])]      # the launch file's blue, and two of the reference's ranges


@functools.lru_cache(maxsize=None)
def rope_image():
    """A 90 x 91 colour + depth image (T = 2) with an occluder: pixels painted from the three ranges, from colours one unit outside the blue range, and at
    random; the per-range reference masks (colour_ref) and clouds (voxel_ref)."""
    rng = np.random.default_rng(91)
    rows, cols = S.D_IMAGES[2]
    P = rows * cols
    base = S.get("D_2_alternate")
    cand = rng.integers(0, 256, (400000, 3)).astype(np.uint8)
    hsv = colour_ref.bgr_to_hsv(cand).astype(np.int64)
    pools = S._colour_pools()
    colour = np.zeros((P, 3), np.uint8)
    kind = rng.integers(0, 6, P)
    for k, (lo, hi) in enumerate(ROPES):
        inside = ((hsv >= np.asarray(lo[0])) & (hsv <= np.asarray(hi[0]))).all(axis=1)
        pool = pools["in"] if k == 0 else cand[inside]
        assert len(pool) >= 100
        idx = np.nonzero(kind == k)[0]
        colour[idx] = pool[rng.integers(0, len(pool), len(idx))]
    idx = np.nonzero(kind == 3)[0]
    near = np.concatenate([pools[t] for t in ("h_lo", "h_hi", "s_lo", "v_lo")])
    colour[idx] = near[rng.integers(0, len(near), len(idx))]
    idx = np.nonzero(kind >= 4)[0]
    colour[idx] = cand[rng.integers(0, len(cand), len(idx))]
    occ = rng.integers(1, 256, P).astype(np.uint8)
    occ[rng.random(P) < 0.1] = 0
    colour = colour.reshape(rows, cols, 3); occ = occ.reshape(rows, cols)
    depth = (1 + 2 * rng.integers(0, 300, (rows, cols))).astype(np.uint16)              # mid-cell depths at leaf 2 mm, as cell_scene deals them
    cam = base.cam
    masks = [colour_ref.colour_mask(colour, lo, hi, occluder=occ) for lo, hi in ROPES]
    refs = [V.voxel_ref(V.backproject(depth, m, *cam), None, S.LEAF) for m in masks]
    assert all(300 < r[1] < P for r in refs) and len({r[1] for r in refs}) == 3
    for a in (colour, occ, depth):
        a.setflags(write=False)
    return dict(depth=depth, colour=colour, occluder=occ, cam=cam), masks, refs


def test_one_image_several_ropes():
    from trackdlo_amd import binding as B
    ctx, ctx2 = bctx(), bctx()
    try:
        img, masks, refs = rope_image()
        params = [B.make_colour_params(lo, hi) for lo, hi in ROPES]
        n, nraw, codes = ctx.depth_to_cloud_batch([img], [(k, 0, params[k]) for k in range(3)], S.LEAF)
        assert codes == [0, 0, 0] and ctx.cloud_batch_route_counts() == [3, 0] and ctx.cloud_route_counts() == [0, 0]
        for k in range(3):
            assert (n[k], nraw[k]) == (refs[k][0].shape[0], refs[k][1]), (k, n[k], nraw[k], refs[k][1])
            assert same_bits(ctx.get_cloud(k), refs[k][0]), k
            X, n1, nraw1 = ctx2.colour_depth_to_cloud(0, img["depth"], img["colour"], params[k], img["occluder"], *img["cam"], S.LEAF)
            assert (n1, nraw1) == (n[k], nraw[k]) and same_bits(X, ctx.get_cloud(k)), k
        # a mixed call -- two frames that bring a mask, two that bring ranges, interleaved -- equals the separate calls
        d7 = S.get("D_2_first")
        imgs = [dict(img, mask=masks[1]), image(d7)]
        res = ctx.depth_to_cloud_batch(imgs, [(4, 0, params[2]), (5, 1, None), (6, 0, params[0]), (7, 0, None)], S.LEAF)
        assert res[2] == [0] * 4 and ctx.cloud_batch_route_counts() == [7, 0]
        for slot, want in ((4, refs[2]), (5, d7.ref), (6, refs[0]), (7, refs[1])):
            assert same_bits(ctx.get_cloud(slot), want[0]), slot
        assert res[0] == [refs[2][0].shape[0], d7.ref[0].shape[0], refs[0][0].shape[0], refs[1][0].shape[0]] and res[1] == [refs[2][1], d7.ref[1], refs[0][1], refs[1][1]]
    finally:
        ctx.close(); ctx2.close()


def test_a_context_taken_through_sizes():
    """F = 3 at 149 x 191, F = 8 at 480 x 640, F = 2 at 63 x 65, F = 3 at 149 x 191 again, then a single call on the team route: the arena is regrown and
    reused at a smaller size, the state words are armed again at every size."""
    ctx = bctx()
    try:
        d7 = [S.get("D_7_%s" % p) for p in S.D_PLACES]
        check_slots(ctx, [0, 1, 2], d7, ctx.depth_to_cloud_batch([image(s) for s in d7], [(0, 0, None), (1, 1, None), (2, 2, None)], S.LEAF), label="149 x 191")
        run_borders(ctx, None, "480 x 640")
        d1 = [S.get("D_1_first"), S.get("D_1_alternate")]
        check_slots(ctx, [6, 7], d1, ctx.depth_to_cloud_batch([image(s) for s in d1], [(6, 0, None), (7, 1, None)], S.LEAF), label="63 x 65")
        before = ctx.cloud_batch_route_counts()
        check_slots(ctx, [3, 4, 5], d7, ctx.depth_to_cloud_batch([image(s) for s in d7], [(3, 0, None), (4, 1, None), (5, 2, None)], S.LEAF), label="149 x 191 again")
        assert ctx.cloud_batch_route_counts() == [before[0] + 3, before[1]]
        # one size, F = 8, 2, 8: what a small call brings (fewer frames, another set of planes) must not reach the state words of the frames it leaves out
        for F in (8, 2, 8):
            check_slots(ctx, range(F), [d7[f % 3] for f in range(F)], ctx.depth_to_cloud_batch([image(s) for s in d7], [(f, f % 3, None) for f in range(F)], S.LEAF),
                        label="F = %d at 149 x 191" % F)
        single = ctx.cloud_route_counts()
        s = S.get("D_7_alternate")
        X, n, nraw = ctx.depth_to_cloud(0, s.depth, s.mask, *s.cam, s.leaf)
        assert ctx.cloud_route_counts() == [single[0] + 1, single[1]] and nraw == s.ref[1] and same_bits(X, s.ref[0])
    finally:
        ctx.close()


def test_planes_in_device_memory():
    """One image's planes are torch tensors on the GPU (copied device to device into the arena), in the batch launch and -- a batch below the crossover, a
    colour frame -- through the single calls, which take them by way of the host.  (The first test of the suite that brings up torch's GPU context pays for
    it, about 11 s that tests/test_cloud_view_gpu.py paid before; the test's own work takes a fraction of a second.)"""
    import torch
    from trackdlo_amd import binding as B
    ctx, ctx2 = bctx(), bctx(batch_min=4)
    try:
        dev = torch.device("cuda:0")
        d7 = [S.get("D_7_%s" % p) for p in S.D_PLACES]
        imgs = [image(s) for s in d7]
        imgs[1] = dict(depth=torch.from_numpy(d7[1].depth.view(np.int16).copy()).to(dev), mask=torch.from_numpy(d7[1].mask.copy()).to(dev), cam=d7[1].cam)
        rope, _, refs = rope_image()
        rdev = dict(rope, **{k: torch.from_numpy(rope[k].view(np.int16).copy() if k == "depth" else rope[k].copy()).to(dev) for k in ("depth", "colour", "occluder")})
        torch.cuda.synchronize()
        params = [B.make_colour_params(lo, hi) for lo, hi in ROPES]
        for c, want in ((ctx, ([3, 0], [0, 0])), (ctx2, ([0, 0], [3, 0]))):
            check_slots(c, [3, 4, 5], d7, c.depth_to_cloud_batch(imgs, [(3, 0, None), (4, 1, None), (5, 2, None)], S.LEAF), label="device planes")
            assert (c.cloud_batch_route_counts(), c.cloud_route_counts()) == want
            n, nraw, codes = c.depth_to_cloud_batch([rdev], [(0, 0, params[1]), (1, 0, params[2])], S.LEAF)
            assert codes == [0, 0] and nraw == [refs[1][1], refs[2][1]]
            assert same_bits(c.get_cloud(0), refs[1][0]) and same_bits(c.get_cloud(1), refs[2][0])
    finally:
        ctx.close(); ctx2.close()


def test_refusals_touch_nothing():
    import ctypes as C
    from trackdlo_amd import binding as B
    ctx = bctx(frames=4)
    try:
        rng = np.random.default_rng(8)
        clouds = [np.asfortranarray(rng.random((100 + 10 * i, 3))) for i in range(4)]
        for i, X in enumerate(clouds):
            ctx.set_cloud(i, X)
        s = S.get("D_1_first")
        img = image(s)
        nomask = dict(depth=s.depth, colour=np.zeros(s.depth.shape + (3,), np.uint8), cam=s.cam)
        blue = B.make_colour_params()
        bad0, bad5 = B.make_colour_params(), B.make_colour_params()
        bad0.n_ranges, bad5.n_ranges = 0, 5
        cases = {
            "a slot twice": ([img], [(0, 0, None), (1, 0, None), (0, 0, None)], S.LEAF),
            "slot -1": ([img], [(-1, 0, None)], S.LEAF), "slot 4": ([img], [(0, 0, None), (4, 0, None)], S.LEAF),
            "no frame": ([img], [], S.LEAF), "more frames than slots": ([img], [(i, 0, None) for i in range(5)], S.LEAF),
            "image -1": ([img], [(0, -1, None)], S.LEAF), "image K": ([img], [(0, 1, None)], S.LEAF),
            "neither mask nor colour": ([img, dict(depth=s.depth, cam=s.cam)], [(0, 0, None)], S.LEAF),
            "ranges without colour": ([img], [(0, 0, blue)], S.LEAF), "no ranges without mask": ([nomask], [(0, 0, None)], S.LEAF),
            "0 ranges": ([nomask], [(0, 0, bad0)], S.LEAF), "5 ranges": ([nomask], [(0, 0, bad5)], S.LEAF),
            "leaf 0": ([img], [(0, 0, None)], 0.0), "leaf < 0": ([img], [(0, 0, None)], -0.002), "leaf nan": ([img], [(0, 0, None)], float("nan")),
            "fx 0": ([dict(img, cam=(0.0, 1e8, 0, 0))], [(0, 0, None)], S.LEAF), "fy 0": ([dict(img, cam=(1e8, 0.0, 0, 0))], [(0, 0, None)], S.LEAF),
        }

        def untouched(why):
            assert ctx.cloud_batch_route_counts() == [0, 0] and ctx.cloud_route_counts() == [0, 0], why
            for i, X in enumerate(clouds):
                assert same_bits(ctx.get_cloud(i), X), (why, i)

        for why, (images, frames, leaf) in cases.items():
            with pytest.raises(B.TdloError) as e:
                ctx.depth_to_cloud_batch(images, frames, leaf)
            assert e.value.code == B.TDLO_E_INVALID, why
            untouched(why)
        # a bad size, as the single call refuses it: straight through the C ABI (the binding takes the size from the planes)
        tab, K, rows, cols, keep = B._batch_images([img])
        fr = (B.BatchFrame * 1)(); fr[0].slot, fr[0].image = 0, 0
        n = np.zeros(1, np.int32)
        for r, c in ((0, cols), (rows, 0), (-rows, cols), (1 << 14, (1 << 12) + 1)):
            rc = ctx.lib.tdlo_depth_to_cloud_batch(ctx.h, C.cast(tab, C.c_void_p), K, r, c, C.cast(fr, C.c_void_p), 1, S.LEAF, n.ctypes.data, n.ctypes.data, None)
            assert rc == B.TDLO_E_INVALID, (r, c)
            untouched((r, c))
        for args in ((None, K, C.cast(fr, C.c_void_p)), (C.cast(tab, C.c_void_p), 0, C.cast(fr, C.c_void_p)), (C.cast(tab, C.c_void_p), K, None)):
            assert ctx.lib.tdlo_depth_to_cloud_batch(ctx.h, args[0], args[1], rows, cols, args[2], 1, S.LEAF, None, None, None) == B.TDLO_E_INVALID
            untouched("null tables")
        # the tracker call refuses the same way (and what tdlo_tracker_frame_batch refuses, a resident cloud apart)
        from trackdlo_amd import synth
        trk = []
        for i in range(2):
            t = B.trackdlo(30, ctx=ctx, slot=i)
            t.initialize_nodes(synth.nodes(30)); t.initialize_geodesic_coord(synth.geodesic_coord(synth.nodes(30)))
            trk.append(t)
        odd = B.trackdlo(31, ctx=ctx, slot=2)
        odd.initialize_nodes(synth.nodes(31)); odd.initialize_geodesic_coord(synth.geodesic_coord(synth.nodes(31)))
        twice = B.trackdlo(30, ctx=ctx, slot=1)
        twice.initialize_nodes(synth.nodes(30)); twice.initialize_geodesic_coord(synth.geodesic_coord(synth.nodes(30)))
        for why, (tl, images, io, cp) in {"image_of out of range": (trk, [img], [0, 1], None), "ranges without colour": (trk, [img], [0, 0], [None, blue]),
                                          "num_of_nodes": (trk + [odd], [img], [0, 0, 0], None), "one slot twice": (trk + [twice], [img], [0, 0, 0], None)}.items():
            Y = [t.get_tracking_result().copy() for t in tl]
            with pytest.raises(B.TdloError) as e:
                B.frames_batch(tl, images, io, cp, S.LEAF, 0.06)
            assert e.value.code == B.TDLO_E_INVALID, why
            untouched(why)
            assert all(np.array_equal(t.get_tracking_result(), y) for t, y in zip(tl, Y)), why
        # the next valid call
        check_slots(ctx, [0, 1], [s, s], ctx.depth_to_cloud_batch([img], [(0, 0, None), (1, 0, None)], S.LEAF), label="after the refusals")
        assert ctx.cloud_batch_route_counts() == [2, 0]
    finally:
        ctx.close()


# ---- trackers -------------------------------------------------------------------------------------------------------------------------------------
M, D_VIS, LEAF_T = 30, 0.06, 0.008


def targs():
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    return (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])


@functools.lru_cache(maxsize=None)
def rope_frames():
    """Four synthetic rope frames (depth, mask, cam) of one rope in motion, 480 x 640."""
    from trackdlo_amd import synth
    out = []
    for i in range(4):
        depth, mask, cam, _ = synth.depth_scene(M, config=20, frame=i)
        depth.setflags(write=False); mask.setflags(write=False)
        out.append((depth, mask, (cam["fx"], cam["fy"], cam["cx"], cam["cy"])))
    return out


def make_trackers(ctx, n):
    from trackdlo_amd import binding as B, synth
    Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
    out = []
    for i in range(n):
        t = B.trackdlo(*targs(), ctx=ctx, slot=i)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        out.append(t)
    return out


def state(t):
    return (t.get_tracking_result().copy(), t.get_sigma2(), [(s["iters"], s["converged"], s["n_kept"], s["status"]) for s in (t.last_stats or [])])


def assert_same_state(a, b, label):
    assert same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], (label, a[1], b[1], a[2], b[2])


def tctx(**env):
    return bctx(frames=8, **dict({"TDLO_ESTEP2": 0}, **env))


def test_tracker_frames_batch_equals_the_calls_made_by_hand():
    """tdlo_tracker_frames_batch against F x tdlo_depth_to_cloud + tdlo_tracker_frame_batch, and against F x tdlo_tracker_frame_from_depth: nodes, sigma2,
    visible sets and iteration counts, two steps (all three contexts under TDLO_ESTEP2=0)."""
    from trackdlo_amd import binding as B
    ca, cb, cc = tctx(), tctx(), tctx()
    try:
        ta, tb, tc = make_trackers(ca, 4), make_trackers(cb, 4), make_trackers(cc, 4)
        fr = rope_frames()
        images = [dict(depth=d, mask=m, cam=cam) for d, m, cam in fr]
        for step in range(2):
            codes, vis, ext, n, nraw = B.frames_batch(ta, images, [0, 1, 2, 3], None, LEAF_T, D_VIS)
            assert codes == [0] * 4 and ca.cloud_batch_route_counts() == [4 * (step + 1), 0]
            nb = [cb.depth_to_cloud(i, d, m, *cam, LEAF_T, fetch=False)[1:] for i, (d, m, cam) in enumerate(fr)]
            codes_b, vis_b, ext_b = B.frame_batch(tb, D_VIS)
            assert codes_b == [0] * 4 and [(a, b) for a, b in zip(n, nraw)] == nb
            for i in range(4):
                assert same_bits(ca.get_cloud(i), cb.get_cloud(i)), (step, i)
                assert np.array_equal(vis[i], vis_b[i]) and np.array_equal(ext[i], ext_b[i]), (step, i)
                assert_same_state(state(ta[i]), state(tb[i]), f"step {step}, tracker {i}: by hand")
                d, m, cam = fr[i]
                v1, e1, n1, nraw1 = tc[i].frame_from_depth(d, m, *cam, LEAF_T, D_VIS)
                assert (n1, nraw1) == (n[i], nraw[i]) and np.array_equal(v1, vis[i]) and np.array_equal(e1, ext[i]), (step, i)
                assert_same_state(state(ta[i]), state(tc[i]), f"step {step}, tracker {i}: frame_from_depth")
                assert ta[i].last_stats[1]["iters"] > 0
    finally:
        ca.close(); cb.close(); cc.close()


def test_a_tracker_whose_frame_selects_no_pixel_is_left_alone():
    from trackdlo_amd import binding as B
    ca, cb = tctx(), tctx()
    try:
        ta, tb = make_trackers(ca, 4), make_trackers(cb, 4)
        fr = rope_frames()
        images = [dict(depth=d, mask=m, cam=cam) for d, m, cam in fr]
        images[2] = dict(images[2], mask=np.zeros_like(fr[2][1]))
        before = state(ta[2])
        codes, vis, ext, n, nraw = B.frames_batch(ta, images, [0, 1, 2, 3], None, LEAF_T, D_VIS, check=False)
        assert codes == [0, 0, B.TDLO_E_EMPTY, 0] and n[2] == 0 and nraw[2] == 0 and len(vis[2]) == 0 and len(ext[2]) == 0
        assert ca.cloud_batch_route_counts() == [4, 0]
        assert same_bits(ta[2].get_tracking_result(), before[0]) and ta[2].get_sigma2() == before[1]
        with pytest.raises(B.TdloError) as e:
            B.frames_batch(ta, images, [0, 1, 2, 3], None, LEAF_T, D_VIS)
        assert e.value.code == B.TDLO_E_EMPTY
        three = [tb[i] for i in (0, 1, 3)]
        for _ in range(2):                                                                  # (the call above stepped the three a second time)
            for i in (0, 1, 3):
                cb.depth_to_cloud(i, fr[i][0], fr[i][1], *fr[i][2], LEAF_T, fetch=False)
            assert B.frame_batch(three, D_VIS)[0] == [0, 0, 0]
        for i in (0, 1, 3):
            assert_same_state(state(ta[i]), state(tb[i]), f"tracker {i} beside the empty one")
    finally:
        ca.close(); cb.close()


def test_one_and_two_frames_under_the_default_crossover():
    """Contexts made without TDLO_CLOUD_BATCH_MIN: F = 1 and F = 2 give the bits of the single calls, whichever route the crossover sends them."""
    from trackdlo_amd import binding as B
    ca, cb = tctx(batch_min=None), tctx(batch_min=None)
    try:
        fr = rope_frames()
        images = [dict(depth=d, mask=m, cam=cam) for d, m, cam in fr]
        for F in (1, 2):
            ta, tb = make_trackers(ca, F), make_trackers(cb, F)
            codes, vis, ext, n, nraw = B.frames_batch(ta, images, list(range(F)), None, LEAF_T, D_VIS)
            assert codes == [0] * F
            got = ca.cloud_batch_route_counts(), ca.cloud_route_counts()
            assert got[0][0] + got[1][0] == (1 if F == 1 else 3) and got[0][1] == 0 and got[1][1] == 0, got        # every frame served once, by one route or the other
            for i in range(F):
                d, m, cam = fr[i]
                v1, e1, n1, nraw1 = tb[i].frame_from_depth(d, m, *cam, LEAF_T, D_VIS)
                assert (n1, nraw1) == (n[i], nraw[i]) and np.array_equal(v1, vis[i]) and np.array_equal(e1, ext[i]), (F, i)
                assert same_bits(ca.get_cloud(i), cb.get_cloud(i)), (F, i)
                assert_same_state(state(ta[i]), state(tb[i]), f"F = {F}, tracker {i}")
            del ta, tb
    finally:
        ca.close(); cb.close()
