"""Result images for many ropes on the device (tdlo_render_result_batch / tdlo_tracker_render_result_batch, k_render_batch in csrc/tdlo_render_batch.hip)
against the numpy statement tests/render_batch_ref.py, byte for byte.  Every output lies between canary bytes; every call's route counters (34: images the
kernel wrote in place, 35: images copied out of the arena) are asserted, and the single call's counters (19 / 20) must not move."""
import numpy as np
import pytest

import colour_ref
import render_batch_cases as BC
import render_batch_ref as RB
import render_cases as K
import render_ref as R
from trackdlo_amd import binding as B, synth

pytestmark = pytest.mark.gpu

CANARY = 64          # a multiple of 4: an output behind it is as aligned as the buffer


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(device=0, timing=False)
    yield c
    c.close()


def _lib_ropes(ropes):
    return [dict(r, params=B.make_render_params(**r["params"]) if r.get("params") else None) for r in ropes]


def _per_image(v, n):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n


class Placed:
    """The images of one call where the test wants them: sources (pageable / pinned: the context's colour buffers / device / device+1) and destinations
    (pageable / pinned: the context's result buffer / device / device+1 / tensor: image k of one [K, rows, cols, 3] device tensor), every destination
    between CANARY poisoned bytes."""
    def __init__(self, ctx, imgs, rows, cols, src, dst, inplace=True):
        import torch
        self.torch = torch
        Kn = len(imgs); n = 3 * rows * cols
        src = _per_image(src, Kn); dst = _per_image(dst, Kn)
        self.images, self.read, self.n_direct, self.keep = [], [], 0, []
        tensor = None
        if "tensor" in dst:
            tensor = torch.full((2 * CANARY + Kn * n,), 0xa5, dtype=torch.uint8, device="cuda")
        for k, im in enumerate(imgs):
            d = {}
            for name, shape in (("colour", (rows, cols, 3)), ("occluder", (rows, cols))):
                a = im.get(name)
                if a is None:
                    continue
                if src[k] == "pageable":
                    d[name] = a
                elif src[k] == "pinned":
                    cb, ob = ctx.colour_buffers(rows, cols)
                    buf = cb if name == "colour" else ob
                    buf[:] = a; d[name] = buf
                else:
                    off = 1 if src[k] == "device+1" else 0
                    t = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")
                    t[off:off + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
                    d[name] = t[off:off + a.size].view(*shape)
                    assert d[name].data_ptr() % 4 == off
            if dst[k] == "pageable":
                buf = np.full(2 * CANARY + n, 0xa5, dtype=np.uint8)
                d["out"] = buf[CANARY:CANARY + n].reshape(rows, cols, 3)
                self.read.append(lambda buf=buf: buf.copy()); direct = False
            elif dst[k] == "pinned":
                pin = ctx.result_image_buffer(rows, cols)
                pin[:] = 0xa5; d["out"] = pin
                self.read.append(lambda pin=pin: np.concatenate([np.full(CANARY, 0xa5, np.uint8), pin.reshape(-1), np.full(CANARY, 0xa5, np.uint8)])); direct = True
            elif dst[k] == "tensor":
                at = CANARY + k * n
                d["out"] = tensor[at:at + n].view(rows, cols, 3)
                lo = at - CANARY if k == 0 else at
                hi = at + n + CANARY if k == Kn - 1 else at + n
                self.read.append(lambda lo=lo, hi=hi, k=k: np.concatenate([np.full(CANARY if k else 0, 0xa5, np.uint8), tensor[lo:hi].cpu().numpy(),
                                                                           np.full(0 if k == Kn - 1 else CANARY, 0xa5, np.uint8)]))
                direct = d["out"].data_ptr() % 4 == 0
            else:
                off = CANARY + (1 if dst[k] == "device+1" else 0)
                t = torch.full((2 * CANARY + n + 8,), 0xa5, dtype=torch.uint8, device="cuda")
                d["out"] = t[off:off + n].view(rows, cols, 3)
                self.read.append(lambda t=t, off=off: t[off - CANARY:off + n + CANARY].cpu().numpy())
                direct = d["out"].data_ptr() % 4 == 0
            self.n_direct += int(direct and inplace)
            self.images.append(d)
        torch.cuda.synchronize()


def _check(ctx, imgs, ropes, rows, cols, src="pageable", dst="pageable", inplace=True, corners=True, want=None, label=""):
    want = want or RB.render_batch(imgs, ropes, rows, cols)
    pl = Placed(ctx, imgs, rows, cols, src, dst, inplace)
    before, single = ctx.render_batch_route_counts(), ctx.render_route_counts()
    outs, cor = ctx.render_result_batch(pl.images, _lib_ropes(ropes), shape=(rows, cols), corners=corners)
    after = ctx.render_batch_route_counts()
    assert [after[0] - before[0], after[1] - before[1]] == [pl.n_direct, len(imgs) - pl.n_direct], (label, before, after, pl.n_direct)
    assert ctx.render_route_counts() == single, label
    n = 3 * rows * cols
    for k in range(len(imgs)):
        buf = pl.read[k]()
        assert np.all(buf[:CANARY] == 0xa5) and np.all(buf[CANARY + n:] == 0xa5), (label, k, "bytes before or behind the image were written")
        got = buf[CANARY:CANARY + n].reshape(rows, cols, 3)
        bad = np.argwhere(np.any(got != want[0][k], axis=2))
        assert len(bad) == 0, (label, k, len(bad), bad[:5].tolist())
    if corners:
        assert cor == want[1], (label, cor, want[1])
    else:
        assert cor is None
    return want


# ---- image tails, images without ropes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kn", [1, 2, 5])
@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (3, 1), (7, 9), (33, 65), (64, 64)])
def test_image_tails_and_images_without_ropes(ctx, shape, Kn):
    rows, cols = shape
    rng = np.random.default_rng(100 * rows + cols + Kn)
    imgs = BC.images(Kn, rows, cols, rows + cols)
    ropes = []
    for k in range(Kn):
        if k == 1:
            continue                                                       # an image with no rope
        if k == 2:
            ropes.append(BC.random_rope(rng, rows, cols, 1, k))            # an image with only a one-node rope
            continue
        ropes += [BC.random_rope(rng, rows, cols, int(rng.integers(2, 9)), k, margin=4), BC.random_rope(rng, rows, cols, 3, k, dict(line_width=2, node_radius=3), margin=4)]
    rng.shuffle(ropes)
    want = _check(ctx, imgs, ropes, rows, cols, dst="device", label="device")          # the kernel's own stores between the canaries
    _check(ctx, imgs, ropes, rows, cols, dst="pageable", want=want, label="pageable")
    for k in (1, 2):
        if k < Kn:
            assert np.array_equal(want[0][k], R.blend(imgs[k]["colour"], imgs[k]["occluder"]))


# ---- the rounds of 64 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_round_boundaries_of_the_rope_level(ctx, n):
    imgs = BC.images(1, 64, 64, 5)
    fan = BC.two_node_fan(n)
    a = _check(ctx, imgs, fan, 64, 64, dst="device", label="in order")
    b = _check(ctx, imgs, fan[::-1], 64, 64, dst="device", label="reversed")
    assert not np.array_equal(a[0][0], b[0][0])                           # the rope drawn last decides where they overlap
    assert tuple(a[0][0][32, 32]) != tuple(b[0][0][32, 32])


def _zigzag(M, seed, image=0):
    c = K.zigzag(M, seed)
    return dict(image=image, Y=c["Y"], proj=c["proj"], vis=c["vis"], params=None)


def test_round_boundaries_of_the_primitive_level(ctx):
    imgs = BC.images(2, 96, 128, 8)
    ropes = [_zigzag(22, 40, 0), _zigzag(23, 41, 1)]
    assert [3 * (len(r["Y"]) - 1) for r in ropes] == [63, 66]
    _check(ctx, imgs, ropes, 96, 128, dst="device")
    _check(ctx, imgs, [dict(ropes[0], image=1), dict(ropes[1], image=1)], 96, 128, dst="device")


def test_a_1024_node_rope_between_two_short_ones(ctx):
    imgs = BC.images(1, 96, 128, 9)
    short = dict(edge_visible=(9, 9, 200), node_visible=(200, 9, 9), line_width=9, node_radius=9)
    ropes = [BC.rope([(2, 50), (125, 40)], 0, [0], [1.0, 1.1], short), _zigzag(1024, 31), BC.rope([(64, 2), (60, 93)], 0, [1], [1.0, 1.1], dict(short, edge_visible=(50, 60, 70)))]
    want = _check(ctx, imgs, ropes, 96, 128, dst="device")
    only_long = RB.render_batch(imgs, ropes[1:2], 96, 128)[0][0]
    assert not np.array_equal(want[0][0], only_long)


# ---- ropes over each other ------------------------------------------------------------------------------------------------------------------------------
def test_crossing_clipped_and_outside_ropes_with_their_own_params(ctx):
    rows, cols = 64, 72
    c = K.crossing()["mixed"]
    self_crossing = dict(image=0, Y=c["Y"], proj=c["proj"], vis=c["vis"], params=None)
    other = BC.rope([(6, 60), (66, 4), (40, 40), (2, 2)], 0, [0, 2], [0.9, 1.5, 0.7, 1.2], dict(line_width=7, node_radius=4, edge_visible=(255, 0, 255), node_hidden=(1, 2, 3)))
    partly = BC.rope([(-30, 20), (20, 30), (100, 90), (60, -20)], 0, [1], [1.0, 1.2, 1.1, 1.3])
    outside = BC.rope([(-40, -40), (-20, -60), (-90, -15)], 0)
    imgs = BC.images(1, rows, cols, 12)
    ropes = [self_crossing, other, partly, outside]
    want = _check(ctx, imgs, ropes, rows, cols, dst="device")
    assert np.array_equal(want[0][0], RB.render_batch(imgs, ropes[:3], rows, cols)[0][0])          # wholly outside: legal, draws nothing
    assert not np.array_equal(want[0][0], RB.render_batch(imgs, [other, self_crossing, partly], rows, cols)[0][0])
    # the same list spread over three images by shuffled image fields
    imgs3 = BC.images(3, rows, cols, 13, [False, True, True])
    spread = [dict(r, image=k) for r, k in zip(ropes, (2, 0, 2, 1))]
    _check(ctx, imgs3, spread, rows, cols, dst=["device", "pageable", "device"])


# ---- occluders and corners ------------------------------------------------------------------------------------------------------------------------------
def test_occluders_and_corners_per_image(ctx):
    rows, cols = 7, 9                                                     # 63 pixels: the last 3 are the byte-wise tail
    imgs = BC.images(6, rows, cols, 20, [False] * 6)
    occ = [np.full((rows, cols), 255, dtype=np.uint8) for _ in range(6)]
    occ[1][-1, -1] = 0                                                    # zero bytes only in the last 1 .. 3 pixels
    occ[2][-1, -2:] = 0
    occ[3][-1, -3:] = 0
    occ[4][0, 0] = 0; occ[4][3, 4] = 0
    for k in (0, 1, 2, 3, 4):
        imgs[k]["occluder"] = occ[k]                                      # image 5: no occluder
    ropes = [BC.rope([(1, 1), (7, 5)], k % 6, [0], [1.0, 1.1]) for k in range(4)]
    want = _check(ctx, imgs, ropes, rows, cols, dst="device")
    assert want[1] == [[-1] * 4, [6, 8, 6, 8], [6, 7, 6, 8], [6, 6, 6, 8], [0, 0, 3, 4], [-1] * 4]
    _check(ctx, imgs, ropes, rows, cols, corners=False, want=want)


def test_colour_null_is_the_last_colour_call(ctx):
    c = K.shapes()["47x53-mixed"]
    rows, cols = c["colour"].shape[:2]
    ctx.colour_mask(c["colour"], B.make_colour_params(*colour_ref.LAUNCH_RANGE), c["occluder"])
    other = BC.images(1, rows, cols, 30, [True])[0]
    imgs = [dict(colour=c["colour"], occluder=c["occluder"]), other]
    ropes = [dict(image=0, Y=c["Y"], proj=c["proj"], vis=c["vis"], params=None), BC.rope([(5, 40), (50, 3)], 0, [], [1.0, 1.1]), BC.rope([(5, 5), (40, 40)], 1)]
    want = RB.render_batch(imgs, ropes, rows, cols)
    before = ctx.render_batch_route_counts()
    outs, cor = ctx.render_result_batch([dict(), other], _lib_ropes(ropes), shape=(rows, cols))
    assert np.array_equal(outs[0], want[0][0]) and np.array_equal(outs[1], want[0][1]) and cor == want[1]
    assert ctx.render_batch_route_counts() == [before[0], before[1] + 2]


# ---- where the bytes come from and go -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["pageable", "pinned", "device", "device+1"])
def test_sources_and_destinations(ctx, src):
    rows, cols = 33, 65
    imgs = BC.images(2, rows, cols, 40, [True, True])
    rng = np.random.default_rng(41)
    ropes = [BC.random_rope(rng, rows, cols, 6, k % 2) for k in range(4)]
    want = RB.render_batch(imgs, ropes, rows, cols)
    other = "pageable" if src == "pinned" else src                        # (the context has one pair of pinned colour buffers)
    for dst in ("pageable", "pinned", "device", "device+1"):
        _check(ctx, imgs, ropes, rows, cols, src=[src, other], dst=[dst, "device" if dst == "pinned" else dst], want=want, label=f"{src} -> {dst}")


@pytest.mark.parametrize("shape", [(33, 65), (7, 6)])
def test_one_device_tensor_of_images(ctx, shape):
    """3 P odd (33 x 65) or 2 mod 4 (7 x 6): the images of one [K, rows, cols, 3] tensor are not all 4-byte aligned -- the aligned ones are written by the
    kernel, the others through the arena; the counters say which."""
    rows, cols = shape
    Kn = 4
    imgs = BC.images(Kn, rows, cols, 50)
    rng = np.random.default_rng(51)
    ropes = [BC.random_rope(rng, rows, cols, 5, k % Kn, margin=3) for k in range(6)]
    pl = Placed(ctx, imgs, rows, cols, "pageable", "tensor")
    assert pl.n_direct == (1 if (3 * rows * cols) % 2 else 2)
    _check(ctx, imgs, ropes, rows, cols, dst="tensor")
    _check(ctx, imgs, ropes, rows, cols, src=["device", "device+1", "device", "device+1"], dst="tensor")


def test_render_inplace_0_copies_every_image(monkeypatch):
    monkeypatch.setenv("TDLO_RENDER_INPLACE", "0")
    cx = B.Context(device=0, timing=False)
    try:
        rows, cols = 33, 65
        imgs = BC.images(3, rows, cols, 60)
        ropes = [BC.random_rope(np.random.default_rng(61), rows, cols, 7, k) for k in (2, 0, 0)]
        _check(cx, imgs, ropes, rows, cols, dst=["device", "pinned", "pageable"], inplace=False)
        assert cx.render_batch_route_counts() == [0, 3]
    finally:
        cx.close()


# ---- against the single call ----------------------------------------------------------------------------------------------------------------------------
def test_one_rope_per_image_equals_the_single_calls(ctx):
    names = ["47x53-mixed", "47x53-one", "47x53-two", "47x53-tail"]
    cases = [K.shapes()[n] for n in names]
    rows, cols = 47, 53
    imgs = [dict(colour=c["colour"], occluder=c["occluder"]) for c in cases]
    ropes = [dict(image=k, Y=c["Y"], proj=c["proj"], vis=c["vis"], params=None) for k, c in enumerate(cases)]
    before = ctx.render_batch_route_counts()
    outs, cor = ctx.render_result_batch(imgs, ropes[::-1])
    assert ctx.render_batch_route_counts() == [before[0], before[1] + 4]          # pageable destinations: four copies out of the arena
    for k, c in enumerate(cases):
        img, one = ctx.render_result(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"])
        assert np.array_equal(outs[k], img) and cor[k] == one, names[k]


# ---- the trackers ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("painter", [False, True])
def test_three_trackers_in_one_picture(painter):
    P = synth.LAUNCH_PARAMS
    M, rows, cols, width = 30, 120, 160, 10
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    params = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    cx = B.Context(device=0, max_frames=3, timing=False)
    try:
        frames = [synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=f, rows=rows, cols=cols, occluder=(40, 100, 60, 72)) for f in range(4)]
        cam = frames[0][4]; a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        proj = R.pinhole(*a)
        trk = [B.trackdlo(*args, ctx=cx, slot=i) for i in range(3)]
        for t in trk:
            t.initialize_nodes(frames[0][5]); t.initialize_geodesic_coord(synth.geodesic_coord(frames[0][5]))
            if painter:
                t.set_self_occlusion(proj.reshape(3, 4), width)
        images = [dict(depth=f[0], colour=f[1], occluder=f[2], cam=a) for f in frames[1:]]
        start = [t.get_tracking_result().copy() for t in trk]
        codes = B.frames_batch(trk, images, [0, 1, 2], [params] * 3, 0.008, 0.06)[0]
        assert codes == [0, 0, 0]
        Y = [t.get_tracking_result().copy() for t in trk]; s2 = [t.get_sigma2() for t in trk]
        assert not np.array_equal(Y[0], Y[1]) and not np.array_equal(Y[1], Y[2])
        vis = [B.self_occlusion_visible(start[i], proj, width, np.zeros(M), np.inf) if painter else np.arange(M) for i in range(3)]
        if painter:
            assert all(0 < len(v) < M for v in vis)
        pics = [dict(colour=frames[1][1], occluder=frames[1][2]), dict(colour=frames[2][1], occluder=None)]
        image_of = [0, 1, 0]
        prm = [None, B.make_render_params(line_width=3, edge_visible=(255, 255, 0)), None]
        ref_prm = [None, dict(line_width=3, edge_visible=(255, 255, 0)), None]
        before = cx.render_batch_route_counts()
        outs, cor = B.render_result_batch(trk, pics, image_of, params=prm)
        assert cx.render_batch_route_counts() == [before[0], before[1] + 2]
        ropes = [dict(image=image_of[i], Y=Y[i], proj=proj, vis=vis[i], params=ref_prm[i]) for i in range(3)]
        want = RB.render_batch(pics, ropes, rows, cols)
        assert np.array_equal(outs[0], want[0][0]) and np.array_equal(outs[1], want[0][1]) and cor == want[1] == [[40, 60, 99, 71], [-1] * 4]
        assert not np.array_equal(want[0][0], RB.render_batch(pics, ropes[:1], rows, cols)[0][0])          # the third tracker's rope is in the first picture
        if painter:
            every = [dict(r, vis=np.arange(M)) for r in ropes]
            assert not np.array_equal(want[0][0], RB.render_batch(pics, every, rows, cols)[0][0])
        outs2, _ = B.render_result_batch(trk, pics, image_of, proj=[proj, None, proj], params=prm, corners=False)      # an explicit matrix: the same pictures
        assert np.array_equal(outs2[0], want[0][0]) and np.array_equal(outs2[1], want[0][1])
        for i, t in enumerate(trk):                                       # rendering leaves the trackers alone
            assert np.array_equal(t.get_tracking_result().view(np.uint64), Y[i].view(np.uint64)) and t.get_sigma2() == s2[i]
    finally:
        cx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def _refused(cx, images, ropes, rows, cols, outs_np, torch_outs=()):
    before = cx.render_batch_route_counts()
    cor = np.full((len(images), 4), -77, dtype=np.int32)
    itab, Kn, _, keep = B._render_images(images, rows, cols)
    rtab, Rn, rkeep = B._render_ropes(_lib_ropes(ropes))
    import ctypes as C
    rc = cx.lib.tdlo_render_result_batch(cx.h, C.cast(itab, C.c_void_p), Kn, rows, cols, C.cast(rtab, C.c_void_p), Rn, cor.ctypes.data)
    assert rc == B.TDLO_E_INVALID and len(cx.lib.tdlo_last_error(cx.h)) > 0
    assert np.all(cor == -77) and all(np.all(o == 0xa5) for o in outs_np) and all(bool((t == 0xa5).all()) for t in torch_outs)
    assert cx.render_batch_route_counts() == before
    return cx.lib.tdlo_last_error(cx.h).decode()


def test_refusals_are_all_or_nothing(ctx):
    import torch
    rows, cols = 33, 65
    imgs = BC.images(2, rows, cols, 70)
    good = [BC.rope([(5, 5), (50, 20), (20, 30)], 0), BC.rope([(9, 30), (60, 3)], 1, [0])]
    outs = [np.full((rows, cols, 3), 0xa5, dtype=np.uint8) for _ in range(2)]
    dev = torch.full((rows, cols, 3), 0xa5, dtype=torch.uint8, device="cuda")
    placed = [dict(imgs[0], out=outs[0]), dict(imgs[1], out=dev)]
    bad_ropes = {
        "rope 1": [good[0], dict(good[1], image=2)],
        "rope 0": [dict(good[0], image=-1), good[1]],
        "rope 1 ": [good[0], dict(good[1], vis=np.array([5], dtype=np.int32))],
        "rope 0 ": [dict(good[0], params=dict(line_width=256)), good[1]],
        "rope 1  ": [good[0], dict(good[1], params=dict(node_radius=0))],
        "rope 1   ": [good[0], dict(good[1], Y=np.asfortranarray(good[1]["Y"] * np.array([1.0, 1.0, -1.0])))],
    }
    for name, ropes in bad_ropes.items():
        assert name.strip() in _refused(ctx, placed, ropes, rows, cols, outs, [dev]), name
    # the same image_out twice; colour == NULL of another shape than the last colour call's
    assert "same image_out" in _refused(ctx, [dict(imgs[0], out=outs[0]), dict(imgs[1], out=outs[0])], good, rows, cols, outs, [dev])
    ctx.colour_mask(np.zeros((8, 8, 3), dtype=np.uint8), B.make_colour_params(*colour_ref.LAUNCH_RANGE), None)
    assert "image 1" in _refused(ctx, [dict(imgs[0], out=outs[0]), dict(out=dev)], good, rows, cols, outs, [dev])
    # a NULL image_out (the binding always supplies one: the table by hand)
    import ctypes as C
    itab, Kn, _, keep = B._render_images(placed, rows, cols)
    itab[1].image_out = None
    rtab, Rn, rkeep = B._render_ropes(_lib_ropes(good))
    cor = np.full((2, 4), -77, dtype=np.int32)
    assert ctx.lib.tdlo_render_result_batch(ctx.h, C.cast(itab, C.c_void_p), Kn, rows, cols, C.cast(rtab, C.c_void_p), Rn, cor.ctypes.data) == B.TDLO_E_INVALID
    assert np.all(cor == -77) and np.all(outs[0] == 0xa5) and b"image 1" in ctx.lib.tdlo_last_error(ctx.h)
    for bad_K, bad_shape in ((0, (rows, cols)), (257, (rows, cols)), (2, (0, cols)), (2, (rows, 8193))):
        assert ctx.lib.tdlo_render_result_batch(ctx.h, C.cast(itab, C.c_void_p), bad_K, bad_shape[0], bad_shape[1], C.cast(rtab, C.c_void_p), Rn, cor.ctypes.data) == B.TDLO_E_INVALID
    assert np.all(cor == -77) and np.all(outs[0] == 0xa5) and bool((dev == 0xa5).all())
    # the next valid call on the same context is still correct
    _check(ctx, imgs, good, rows, cols, dst=["pageable", "device"])


def test_refused_trackers_and_a_fresh_context():
    import ctypes as C
    rows, cols = 33, 65
    imgs = BC.images(1, rows, cols, 80)
    ca, cb = B.Context(device=0, max_frames=2, timing=False), B.Context(device=0, timing=False)
    try:
        out = np.full((rows, cols, 3), 0xa5, dtype=np.uint8)
        # colour == NULL without a colour call before it
        assert "image 0" in _refused(ca, [dict(out=out)], [BC.rope([(5, 5), (50, 20)], 0)], rows, cols, [out])
        Y0 = np.asfortranarray(R.nodes_from_pixels([(5, 5), (20, 9), (30, 30), (50, 12)], K.FX))
        ta, ta2, tb = B.trackdlo(4, ctx=ca, slot=0), B.trackdlo(4, ctx=ca, slot=1), B.trackdlo(4, ctx=cb)
        for t in (ta, tb):
            t.initialize_nodes(Y0)
        pics = [dict(imgs[0], out=out)]
        proj = [K.PROJ, K.PROJ]
        for pair, word in (((ta, tb), "context"), ((ta, ta2), "rope 1")):          # another context; a tracker whose nodes were never given (all zero: w = 0)
            got = B.render_result_batch(list(pair), pics, [0, 0], proj=proj, check=False)
            assert got[2] == B.TDLO_E_INVALID and word in ca.lib.tdlo_last_error(ca.h).decode() and np.all(out == 0xa5) and got[1] == [[0] * 4]
        assert B.render_result_batch([ta], pics, [0], check=False)[2] == B.TDLO_E_INVALID and np.all(out == 0xa5)          # no matrix to be had
        assert ca.render_batch_route_counts() == [0, 0]
        outs, _ = B.render_result_batch([ta], pics, [0], proj=[K.PROJ])
        want = RB.render_batch(imgs, [dict(image=0, Y=Y0, proj=K.PROJ, vis=np.arange(4), params=None)], rows, cols)
        assert np.array_equal(outs[0], want[0][0]) and ca.render_batch_route_counts() == [0, 1]
    finally:
        ca.close(); cb.close()


# ---- sensor-size frames -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(480, 640), (720, 1280)])
def test_sensor_size_frames(ctx, shape):
    rows, cols = shape
    c = K.bench_frame(rows, cols)
    imgs = [dict(colour=c["colour"], occluder=c["occluder"]), dict(colour=np.ascontiguousarray(c["colour"][::-1]), occluder=None)]
    rng = np.random.default_rng(rows)
    ropes = []
    for k in range(2):
        ropes.append(dict(image=k, Y=c["Y"], proj=c["proj"], vis=c["vis"], params=None))
        ropes += [BC.random_rope(rng, rows, cols, 45, k, dict(edge_visible=(255, 128 * k, 0))) for _ in range(2)]
    want = _check(ctx, imgs, ropes, rows, cols, dst=["device", "pageable"])
    assert np.count_nonzero(np.any(want[0][0] != R.blend(c["colour"], c["occluder"]), axis=2)) > 9000
