"""tdlo_frame_views_to_cloud_batch / tdlo_tracker_frame_views_batch / tdlo_view_batch_images (k_image_import_batch into the batch arena, then
k_cloud_fused_batch): every slot's cloud, n and n_raw are, bit for bit, those of tdlo_frame_to_cloud_view on that frame alone, whatever else shares the call.

Each case is held to three things: the single view call per frame on a second context; tests/voxel_ref.py / tests/colour_ref.py on the canonical images of
tests/image_view_ref.py; and, for the canonical planes, tdlo_view_batch_images read back against image_view_ref.canonical byte for byte (the arena's padding
is not compared).  Each case asserts tdlo_debug_route_count 42 / 43 / 44.  Every comparison is on uint64 / byte views; there is no tolerance anywhere.
Contexts are made under TDLO_FRAME_VIEW_BATCH_MIN=1 unless said otherwise, so that a batch of any size takes the batch launches."""
import functools

import numpy as np
import pytest

import colour_ref
import image_view_ref as R
import voxel_ref as V
from test_prepass_gpu import make_ctx
from test_image_view_gpu import _place, _sources

pytestmark = pytest.mark.gpu

NAMES = ("depth", "colour", "occluder", "mask")
CAM = (600.0, 601.0, 3.5, 2.25)
LEAF = 1.0                                             # random depths of up to 65 m: a leaf of a metre keeps the clouds small
HALF_A = ([[0, 0, 0]], [[90, 255, 255]])               # ranges that pass about half of random colours, each another half
HALF_B = ([[60, 0, 0]], [[180, 255, 255]])
HALF_C = ([[0, 100, 0], [0, 0, 0]], [[180, 255, 200], [30, 99, 255]])
NOTHING = ([[10, 10, 10]], [[5, 5, 5]])


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    return binding


@pytest.fixture(scope="module")
def synth():
    from trackdlo_amd import synth
    return synth


def vctx(frames=10, batch_min=1, **env):
    return make_ctx(dict({"TDLO_FRAME_VIEW_BATCH_MIN": batch_min}, **env), max_frames=frames, max_points=1 << 15, max_nodes=64)


@pytest.fixture(scope="module")
def ctxs():
    a, b = vctx(), vctx()
    yield a, b
    a.close(); b.close()


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class _Raw:
    def __init__(self, address, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="|u1", data=(int(address), False), version=2)


def read_device(torch, address, n):
    return torch.as_tensor(_Raw(address, n), device="cuda").cpu().numpy().copy()


def pick(rows, cols, fmt, name, rng):
    return next(l for l in R.layouts(rows, cols, fmt, rng) if l[0] == name)


class Img:
    """One image of a batch: per role an ImageView (where the test put it) and the canonical plane it stands for."""
    def __init__(self, rows, cols, cam=CAM):
        self.rows, self.cols, self.cam, self.views, self.canon = rows, cols, cam, {}, {}

    def lay(self, B, torch, name, fmt, layout, device, ready_stream=None):
        """A layout of image_view_ref.layouts: random content, poisoned surroundings, poisoned alpha."""
        _, buf, off, stride = layout
        v = _place(B, torch, buf, off, fmt, stride, self.rows, self.cols, device)
        if ready_stream:
            v.ready_stream = ready_stream
        self.views[name] = v
        self.canon[name] = R.canonical(buf, off, fmt, stride, self.rows, self.cols)
        return self

    def plain(self, B, torch, name, arr, device, canon=None):
        """A given image as a contiguous array (uint16 depth carried in int16 on the device, which has no uint16 tensors everywhere)."""
        arr = np.ascontiguousarray(arr)
        if not device:
            v = B.image_view(arr)
        elif arr.dtype == np.uint16:
            v = B.image_view(torch.from_numpy(arr.view(np.int16).copy()).cuda(), format=B.IMG_U16C1)
        else:
            v = B.image_view(torch.from_numpy(arr.copy()).cuda())
        self.views[name] = v
        self.canon[name] = arr if canon is None else canon
        return self

    def share(self, other, name):
        self.views[name], self.canon[name] = other.views[name], other.canon[name]
        return self

    def image(self):
        return dict(cam=self.cam, **self.views)

    def frame_view(self, B, colour):
        v = self.views
        return B.frame_view(v["depth"], v["colour"], v.get("occluder")) if colour else B.frame_view(v["depth"], mask=v["mask"])


def expected(img, rng, leaf):
    m = img.canon["mask"] if rng is None else colour_ref.colour_mask(img.canon["colour"], *rng, occluder=img.canon.get("occluder"))
    return V.voxel_ref(V.backproject(img.canon["depth"], m, *img.cam), None, leaf)


def run(B, torch, ctx, ctx2, imgs, frames, leaf, want, label, arena=True, refs=None):
    """frames: (slot, image, ranges or None).  want: what the call adds to counters 42 / 43 / 44."""
    before, packed, single = ctx.frame_view_batch_route_counts(), ctx.cloud_batch_route_counts(), ctx.cloud_route_counts()
    params = [None if r is None else B.make_colour_params(*r) for _, _, r in frames]
    n, nraw, codes = ctx.frame_views_to_cloud_batch([i.image() for i in imgs], [(s, k, p) for (s, k, _), p in zip(frames, params)], leaf)
    after = ctx.frame_view_batch_route_counts()
    assert [a - b for a, b in zip(after, before)] == list(want), (label, before, after)
    assert ctx.cloud_batch_route_counts() == packed, label                                      # 32 / 33 are the packed batch's
    if want[1] == 0:
        assert ctx.cloud_route_counts() == single, label                                        # nothing took the single route
    assert codes == [0] * len(frames), (label, codes)
    for i, (slot, k, r) in enumerate(frames):
        X, nr = refs[i] if refs is not None else expected(imgs[k], r, leaf)
        assert (n[i], nraw[i]) == (X.shape[0], nr), (label, i, n[i], nraw[i], X.shape[0], nr)
        got = ctx.get_cloud(slot)
        assert same_bits(got, X), (label, i)
        if ctx2 is not None:
            X1, n1, nraw1 = ctx2.frame_to_cloud_view(0, imgs[k].frame_view(B, r is not None), params[i], *imgs[k].cam, leaf)
            assert (n1, nraw1) == (n[i], nraw[i]) and same_bits(X1, got), (label, i)
    used = {(k, "depth") for _, k, _ in frames} | {(k, "mask") for _, k, r in frames if r is None}
    for _, k, r in frames:
        if r is not None:
            used |= {(k, "colour")} | ({(k, "occluder")} if "occluder" in imgs[k].views else set())
    for k, img in enumerate(imgs):
        planes = ctx.view_batch_images(k)
        for name in NAMES:
            if arena and (k, name) in used:
                c = img.canon[name]
                assert planes[name] is not None and planes[name] % 256 == 0, (label, k, name)
                assert read_device(torch, planes[name], c.nbytes).tobytes() == c.tobytes(), (label, k, name)
            else:
                assert planes[name] is None, (label, k, name)
    return n, nraw


# ---- image tails and the grid's second dimension ---------------------------------------------------------------------------------------------------
def tail_image(B, torch, rows, cols, rng, odd):
    """odd: the image whose views are misaligned -- data offsets 1 / 2, odd pitches, bottom-up rows -- among images that are as aligned as the width allows."""
    im = Img(rows, cols)
    if odd:
        im.lay(B, torch, "depth", R.U16C1, pick(rows, cols, R.U16C1, "off-and-pitch", rng), True)
        im.lay(B, torch, "colour", R.U8C3, pick(rows, cols, R.U8C3, "pitch+1", rng), True)
        im.lay(B, torch, "occluder", R.U8C1, pick(rows, cols, R.U8C1, "off1", rng), True)
        im.lay(B, torch, "mask", R.U8C1, pick(rows, cols, R.U8C1, "bottom-up", rng), True)
    else:
        im.lay(B, torch, "depth", R.F32C1, pick(rows, cols, R.F32C1, "pitch+16", rng), True)
        im.lay(B, torch, "colour", R.U8C4, pick(rows, cols, R.U8C4, "off0", rng), True)
        im.lay(B, torch, "mask", R.U8C1, pick(rows, cols, R.U8C1, "pitch+4", rng), True)
    return im


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (5, 7), (32, 32), (2, 514)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_tails_and_the_second_grid_dimension(B, torch, ctxs, shape, K):
    """1 x 1, 3 x 5 and 5 x 7 end in a lane of 1 or 3 pixels; 32 x 32 is exactly one workgroup of lanes, 2 x 514 one lane into a second.  K images, a mask
    frame and a colour frame each; the misaligned image first, in the middle and last."""
    ctx, ctx2 = ctxs
    rows, cols = shape
    rng = np.random.default_rng(1000 * rows + cols + K)
    for at in sorted({0, K // 2, K - 1}):
        imgs = [tail_image(B, torch, rows, cols, rng, k == at) for k in range(K)]
        frames = [(2 * k, k, None) for k in range(K)] + [(2 * k + 1, k, HALF_A if k % 2 else HALF_B) for k in range(K)]
        planes = sum(len(i.views) for i in imgs)
        run(B, torch, ctx, ctx2, imgs, frames, LEAF, (2 * K, 0, planes), f"{shape} K={K} odd at {at}")


# ---- forms in one launch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 8), (32, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_forms_in_one_launch(B, torch, ctxs, shape):
    """K = 5 images in one call: wide loads (data and pitch multiples of 16), dword loads (data offset 4), element by element (data offset 1 / 2, odd
    pitches), a pitch larger than the row, bottom-up rows; all five formats.  The poison around the rows and in the alpha bytes shows in no plane: run()
    compares every plane with the canonical image."""
    ctx, ctx2 = ctxs
    rows, cols = shape
    rng = np.random.default_rng(77 + rows)
    spec = [
        dict(depth=(R.F32C1, "pitch+16"), colour=(R.U8C4, "off0"), occluder=(R.U8C1, "off8"), mask=(R.U8C1, "pitch+4")),
        dict(depth=(R.U16C1, "off4"), colour=(R.U8C4, "off4"), mask=(R.U8C1, "off4")),
        dict(depth=(R.U16C1, "off-and-pitch"), colour=(R.U8C3, "pitch+1"), occluder=(R.U8C1, "off1"), mask=(R.U8C1, "pitch+1")),
        dict(depth=(R.U16C1, "pitch+12"), colour=(R.U8C3, "pitch+12"), mask=(R.U8C1, "pitch+16")),
        dict(depth=(R.F32C1, "bottom-up"), colour=(R.U8C4, "bottom-up-pitch+16"), occluder=(R.U8C1, "bottom-up"), mask=(R.U8C1, "bottom-up-pitch+16")),
    ]
    imgs = []
    for s in spec:
        im = Img(rows, cols)
        for name, (fmt, lay) in s.items():
            im.lay(B, torch, name, fmt, pick(rows, cols, fmt, lay, rng), True)
        imgs.append(im)
    forms = [{name: B.image_view_form(v) for name, v in im.views.items()} for im in imgs]
    assert forms[0] == dict(depth=2, colour=2, occluder=1, mask=1) and set(forms[1].values()) == {1} and set(forms[2].values()) == {0}, forms
    assert forms[3] == dict(depth=1, colour=1, mask=1) and forms[4]["depth"] == 2 and forms[4]["colour"] == 2, forms
    assert {v.format for im in imgs for v in im.views.values()} == {B.IMG_U8C1, B.IMG_U8C3, B.IMG_U8C4, B.IMG_U16C1, B.IMG_F32C1}
    frames = [(k, k, None) for k in range(5)] + [(5 + k, k, (HALF_A, HALF_B, HALF_C)[k % 3]) for k in range(5)]
    run(B, torch, ctx, ctx2, imgs, frames, LEAF, (10, 0, sum(len(i.views) for i in imgs)), f"forms {shape}")


# ---- 32FC1 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_f32_depths_at_the_rounding_borders(B, torch, ctxs, device):
    """Depths at k mm and k +- half a millimetre, NaN, +-inf, negatives and >= 65.5355 m: the millimetres of exact rational arithmetic."""
    ctx, ctx2 = ctxs
    ks = [0, 1, 2, 499, 500, 1000, 1001, 32767, 32768, 65534, 65535]
    vals = []
    for k in ks:
        for d in (k / 1000.0, (k - 0.5) / 1000.0, (k + 0.5) / 1000.0):
            f = np.float32(d)
            vals += [f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))]
    vals += [np.nan, np.inf, -np.inf, -0.0, -1e-9, -0.0004, -0.0006, -1.0, 65.5354, 65.5355, 65.53551, 65.536, 100.0, 3e38, 1e-45, 0.125e-3, 0.0004999]
    rows, cols = 8, 16
    assert len(vals) <= rows * cols
    metres = np.resize(np.array(vals, dtype=np.float32), rows * cols).reshape(rows, cols)
    exact = np.array([R.f32_to_mm_exact(v) for v in metres.reshape(-1)], dtype=np.uint16).reshape(rows, cols)
    assert np.array_equal(R.f32_to_mm(metres), exact) and len(set(exact.reshape(-1).tolist())) >= 15 and np.count_nonzero(exact == 0) > 10
    im = Img(rows, cols).plain(B, torch, "depth", metres, device, canon=exact)
    im.plain(B, torch, "mask", np.full((rows, cols), 255, np.uint8), device)
    run(B, torch, ctx, ctx2, [im], [(0, 0, None)], LEAF, (1, 0, 2 if device else 0), f"f32 {device}")


# ---- sharing -----------------------------------------------------------------------------------------------------------------------------------------
def test_sharing(B, torch, ctxs):
    ctx, ctx2 = ctxs
    rows, cols = 9, 20
    rng = np.random.default_rng(31)

    def full(k):
        im = Img(rows, cols, cam=(600.0 + k, 601.0, 3.5, 2.25))
        for name, fmt, lay in (("depth", R.F32C1, "pitch+4"), ("colour", R.U8C4, "pitch+16"), ("occluder", R.U8C1, "off0"), ("mask", R.U8C1, "off2")):
            im.lay(B, torch, name, fmt, pick(rows, cols, fmt, lay, rng), True)
        return im
    a = full(0)
    # three frames out of one colour image, each with its own ranges: depth, colour and occluder once
    run(B, torch, ctx, ctx2, [a], [(0, 0, HALF_A), (1, 0, HALF_B), (2, 0, HALF_C)], LEAF, (3, 0, 3), "three ropes, one image")
    # two images that name the same depth view with different colour views: the depth once
    b = Img(rows, cols, cam=a.cam).share(a, "depth").lay(B, torch, "colour", R.U8C3, pick(rows, cols, R.U8C3, "off1", rng), True)
    run(B, torch, ctx, ctx2, [a, b], [(0, 0, HALF_A), (1, 1, HALF_A)], LEAF, (2, 0, 4), "one depth view, two colour views")
    # an image carrying both mask and colour, used by a mask frame and a colour frame
    run(B, torch, ctx, ctx2, [a], [(4, 0, None), (3, 0, HALF_B)], LEAF, (2, 0, 4), "mask frame and colour frame of one image")
    # a plane no frame reads is not imported: the colour and the occluder of a, all of an image no frame names
    run(B, torch, ctx, ctx2, [a, full(1)], [(0, 0, None)], LEAF, (1, 0, 2), "planes nobody reads")


# ---- location ----------------------------------------------------------------------------------------------------------------------------------------
def test_host_and_device_views(B, torch, ctxs):
    ctx, ctx2 = ctxs
    rows, cols = 7, 12
    rng = np.random.default_rng(41)

    def make(where):
        im = Img(rows, cols)
        for (name, fmt, lay), dev in zip((("depth", R.U16C1, "pitch+2"), ("colour", R.U8C4, "bottom-up"), ("occluder", R.U8C1, "pitch+12"), ("mask", R.U8C1, "off4")), where):
            im.lay(B, torch, name, fmt, pick(rows, cols, fmt, lay, rng), dev)
        return im
    frames = lambda K: [(k, k, None) for k in range(K)] + [(K + k, k, HALF_A) for k in range(K)]
    mixed = [make((True, False, True, False)), make((False, True, False, True)), make((True, True, True, True)), make((False, False, False, False))]
    run(B, torch, ctx, ctx2, mixed, frames(4), LEAF, (8, 0, 8), "host and device views mixed inside images and across")
    hosts = [make((False,) * 4) for _ in range(3)]
    run(B, torch, ctx, ctx2, hosts, frames(3), LEAF, (6, 0, 0), "all host")
    devs = [make((True,) * 4) for _ in range(3)]
    run(B, torch, ctx, ctx2, devs, frames(3), LEAF, (6, 0, 12), "all device")


def test_ready_stream(B, torch, ctxs):
    """Device images filled by torch work on a side stream, behind enough work that it has not run when the call is made, handed over with that stream as
    ready_stream and no host wait; a second image comes ready on the default stream."""
    ctx, ctx2 = ctxs
    rows, cols = 60, 80
    rng = np.random.default_rng(9)
    mm = rng.integers(0, 65536, (rows, cols)).astype(np.uint16)
    bgra = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    src_d = torch.from_numpy((mm / 1000.0).astype(np.float32)).cuda()
    src_c = torch.from_numpy(bgra).cuda()
    dst_d, dst_c = torch.zeros_like(src_d), torch.zeros_like(src_c)
    big = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):
            big = big @ big * 1e-4
        dst_d.copy_(src_d); dst_c.copy_(src_c)
    a = Img(rows, cols)
    a.views = dict(depth=B.image_view(dst_d, ready_stream=side.cuda_stream), colour=B.image_view(dst_c, ready_stream=side.cuda_stream))
    a.canon = dict(depth=mm, colour=np.ascontiguousarray(bgra[:, :, :3]))
    b = Img(rows, cols).plain(B, torch, "depth", mm[::-1], True).plain(B, torch, "mask", (bgra[:, :, 3] > 200).astype(np.uint8), True)
    run(B, torch, ctx, None, [a, b], [(0, 0, HALF_A), (1, 1, None), (2, 0, HALF_B)], LEAF, (3, 0, 4), "ready_stream")
    torch.cuda.synchronize()
    assert np.array_equal(dst_d.cpu().numpy(), src_d.cpu().numpy())


# ---- slots -------------------------------------------------------------------------------------------------------------------------------------------
def test_slots_and_interleaved_calls(B, torch, ctxs):
    ctx, ctx2 = ctxs
    rows, cols = 24, 36
    rng = np.random.default_rng(51)

    def make(k):
        im = Img(rows, cols, cam=(500.0 + 10 * k, 505.0, 17.5, 11.5))
        for name, fmt, lay in (("depth", R.F32C1, "off0"), ("colour", R.U8C4, "off0"), ("mask", R.U8C1, "pitch+4")):
            im.lay(B, torch, name, fmt, pick(rows, cols, fmt, lay, rng), True)
        return im
    imgs = [make(k) for k in range(8)]
    empty = Img(rows, cols).share(imgs[0], "depth").plain(B, torch, "mask", np.zeros((rows, cols), np.uint8), True)
    for F in (1, 2, 8):
        run(B, torch, ctx, ctx2, imgs[:F], [(f, f, None if f % 2 else HALF_A) for f in range(F)], LEAF, (F, 0, 2 * F), f"F = {F}")
    run(B, torch, ctx, ctx2, imgs[:8], [(7 - f, f, None) for f in range(8)], LEAF, (8, 0, 16), "reversed slots")
    big = np.asfortranarray(np.random.default_rng(3).random((20000, 3)))
    for slot in (3, 4, 5):
        ctx.set_cloud(slot, big)
    n, _ = run(B, torch, ctx, ctx2, imgs[:2] + [empty], [(5, 0, None), (3, 2, None), (4, 1, HALF_B)], LEAF, (3, 0, 5), "over larger clouds, with an empty frame")   # (the empty image's depth is image 0's)
    assert n[1] == 0 and ctx.get_cloud(3).shape[0] == 0
    # the call made twice, the second with a smaller F; then a packed batch and single view calls in between on the same context
    run(B, torch, ctx, ctx2, imgs[:6], [(f, f, None) for f in range(6)], LEAF, (6, 0, 12), "F = 6")
    run(B, torch, ctx, ctx2, imgs[:2], [(f, f, HALF_C) for f in range(2)], LEAF, (2, 0, 4), "F = 2 behind F = 6")
    one = imgs[3]
    X1, n1, nraw1 = ctx.frame_to_cloud_view(9, one.frame_view(B, False), None, *one.cam, LEAF)
    ref = expected(one, None, LEAF)
    assert (n1, nraw1) == (ref[0].shape[0], ref[1]) and same_bits(X1, ref[0])
    with pytest.raises(B.TdloError):
        ctx.view_batch_images(2)                                                                # (k out of range: the last batch had two images)
    was = ctx.frame_view_batch_route_counts()
    packed = dict(depth=one.canon["depth"], mask=one.canon["mask"], cam=one.cam)
    # (the packed batch loops over the single calls below its own crossover: whichever route it takes, it leaves counters 42 .. 44 alone)
    n2, nraw2, codes = ctx.depth_to_cloud_batch([packed], [(8, 0, None)], LEAF)
    assert codes == [0] and (n2[0], nraw2[0]) == (n1, nraw1) and same_bits(ctx.get_cloud(8), ref[0]) and ctx.frame_view_batch_route_counts() == was
    run(B, torch, ctx, ctx2, imgs[:3], [(f, f, None) for f in range(3)], LEAF, (3, 0, 6), "behind the other entrances")
    assert same_bits(ctx.get_cloud(9), ref[0]) and same_bits(ctx.get_cloud(8), ref[0])        # slots the call did not name keep their clouds


def test_the_packed_batch_invalidates_the_planes(B, torch):
    """tdlo_view_batch_images after a packed batch that wrote the arena: TDLO_E_INVALID (the pointers are valid until the next batch call)."""
    ctx = vctx(frames=2, TDLO_CLOUD_BATCH_MIN=1)
    try:
        rows, cols = 5, 8
        rng = np.random.default_rng(61)
        im = Img(rows, cols).lay(B, torch, "depth", R.U16C1, pick(rows, cols, R.U16C1, "off0", rng), True).lay(B, torch, "mask", R.U8C1, pick(rows, cols, R.U8C1, "off0", rng), False)
        with pytest.raises(B.TdloError) as e:
            ctx.view_batch_images(0)                                                            # no view batch yet
        assert e.value.code == B.TDLO_E_INVALID
        run(B, torch, ctx, None, [im], [(0, 0, None)], LEAF, (1, 0, 1), "one frame")
        ctx.depth_to_cloud_batch([dict(depth=im.canon["depth"], mask=im.canon["mask"], cam=im.cam)], [(1, 0, None)], LEAF)
        assert ctx.cloud_batch_route_counts() == [1, 0] and same_bits(ctx.get_cloud(0), ctx.get_cloud(1))
        with pytest.raises(B.TdloError) as e:
            ctx.view_batch_images(0)
        assert e.value.code == B.TDLO_E_INVALID
    finally:
        ctx.close()


# ---- passed on ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_frame_the_cloud_kernel_passes_on():
    """32 705 masked pixels: through the single view call for its slot alone, the same bits; 32 704 in the same call: served."""
    import torch
    from trackdlo_amd import binding as B
    from test_cloud_batch_gpu import border_frames, LEAF_B
    fr = border_frames()
    (full, r_full), (over, r_over) = fr[3], fr[4]
    assert (full.name, r_full, over.name, r_over) == ("C_32704", "taken", "C_32705", "passed")
    ctx, ctx2 = vctx(frames=2), vctx(frames=2)
    try:
        imgs = []
        for s in (over, full):
            rows, cols = s.depth.shape
            im = Img(rows, cols, cam=s.cam).plain(B, torch, "depth", (s.depth / 1000.0).astype(np.float32), True, canon=np.asarray(s.depth))
            assert np.array_equal(R.f32_to_mm(im.views["depth"].owner.cpu().numpy()), s.depth)
            imgs.append(im.plain(B, torch, "mask", s.mask, True))
        single = ctx.cloud_route_counts()
        n, nraw = run(B, torch, ctx, ctx2, imgs, [(0, 0, None), (1, 1, None)], LEAF_B, (1, 1, 4), "32 705 and 32 704", refs=[over.ref, full.ref])
        assert nraw == [32705, 32704]
        assert ctx.cloud_route_counts() == [single[0], single[1] + 1]                          # the single call sent the frame on to the multi-launch form
    finally:
        ctx.close(); ctx2.close()


# ---- below the crossover -------------------------------------------------------------------------------------------------------------------------------
def test_below_the_crossover_the_call_loops_over_the_single_calls(B, torch):
    """A context made without TDLO_FRAME_VIEW_BATCH_MIN (make_ctx takes the variable out of the environment while the context is made, which is when it
    is read): F = 1 lies below the default constant whatever the measurement made it (it is at least 2), counter 43 moves, the bits are the same."""
    ctx, ctx2 = vctx(batch_min=None), vctx()
    try:
        rows, cols = 9, 20
        rng = np.random.default_rng(71)
        im = Img(rows, cols)
        for name, fmt, lay in (("depth", R.F32C1, "pitch+4"), ("colour", R.U8C4, "pitch+16"), ("occluder", R.U8C1, "off0"), ("mask", R.U8C1, "off2")):
            im.lay(B, torch, name, fmt, pick(rows, cols, fmt, lay, rng), name != "mask")
        run(B, torch, ctx, ctx2, [im], [(0, 0, HALF_A)], LEAF, (0, 1, 0), "F = 1, colour", arena=False)
        run(B, torch, ctx, ctx2, [im], [(1, 0, None)], LEAF, (0, 1, 0), "F = 1, mask", arena=False)
    finally:
        ctx.close(); ctx2.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(B, torch):
    import ctypes as C
    ctx = vctx(frames=4)
    try:
        rows, cols = 6, 8
        rng = np.random.default_rng(81)
        clouds = [np.asfortranarray(rng.random((100 + 10 * i, 3))) for i in range(4)]
        for i, X in enumerate(clouds):
            ctx.set_cloud(i, X)

        def good(device=True):
            im = Img(rows, cols)
            for name, fmt, lay in (("depth", R.U16C1, "off0"), ("colour", R.U8C4, "off0"), ("occluder", R.U8C1, "off0"), ("mask", R.U8C1, "off0")):
                im.lay(B, torch, name, fmt, pick(rows, cols, fmt, lay, rng), device)
            return im

        def without(im, *names):
            d = im.image()
            for nme in names:
                del d[nme]
            return d

        def changed(im, name, **kw):
            v0 = im.views[name]
            v = B.ImageView(v0.data, v0.format, v0.location, v0.row_stride, v0.ready_stream)
            v.rows, v.cols, v.owner = rows, cols, v0.owner
            for k, x in kw.items():
                setattr(v, k, x)
            return dict(im.image(), **{name: v})

        g, h = good(), good(False)
        img = g.image()
        blue = B.make_colour_params()
        bad0, bad5 = B.make_colour_params(), B.make_colour_params()
        bad0.n_ranges, bad5.n_ranges = 0, 5
        counters = lambda: [int(ctx.lib.tdlo_debug_route_count(ctx.h, k)) for k in range(45)]
        zero = counters()

        def untouched(why):
            assert counters() == zero, why
            for i, X in enumerate(clouds):
                assert same_bits(ctx.get_cloud(i), X), (why, i)

        cases = {
            # what the packed batch refuses
            "a slot twice": ([img], [(0, 0, None), (1, 0, None), (0, 0, None)], LEAF), "slot -1": ([img], [(-1, 0, None)], LEAF),
            "slot 4": ([img], [(0, 0, None), (4, 0, None)], LEAF), "no frame": ([img], [], LEAF),
            "more frames than slots": ([img], [(i, 0, None) for i in range(5)], LEAF),
            "image -1": ([img], [(0, -1, None)], LEAF), "image K": ([img], [(0, 1, None)], LEAF),
            "neither mask nor colour": ([img, without(g, "mask", "colour", "occluder")], [(0, 0, None)], LEAF),
            "ranges without colour": ([without(g, "colour", "occluder")], [(0, 0, blue)], LEAF),
            "no ranges without mask": ([without(g, "mask")], [(0, 0, None)], LEAF),
            "0 ranges": ([img], [(0, 0, bad0)], LEAF), "5 ranges": ([img], [(0, 0, bad5)], LEAF),
            "leaf 0": ([img], [(0, 0, None)], 0.0), "leaf < 0": ([img], [(0, 0, None)], -0.002), "leaf nan": ([img], [(0, 0, None)], float("nan")),
            "fx 0": ([dict(img, cam=(0.0, 1e8, 0, 0))], [(0, 0, None)], LEAF), "fy 0": ([dict(img, cam=(1e8, 0.0, 0, 0))], [(0, 0, None)], LEAF),
            # per plane, what tdlo_image_view_check refuses -- also of an image or a plane no frame reads
            "rows overlap": ([changed(g, "colour", row_stride=4 * cols - 4)], [(0, 0, None)], LEAF),
            "misaligned depth": ([changed(h, "depth", data=h.views["depth"].data + 1)], [(0, 0, None)], LEAF),
            "a depth format for the mask": ([changed(g, "mask", format=B.IMG_U16C1)], [(0, 0, None)], LEAF),
            "an unknown format": ([img, changed(g, "occluder", format=9)], [(0, 0, None)], LEAF),
            "an unknown location": ([changed(g, "depth", location=7)], [(0, 0, None)], LEAF),
            # a mask together with an occluder and no colour
            "mask + occluder, no colour": ([without(g, "colour")], [(0, 0, None)], LEAF),
            # locations
            "host memory called device memory": ([changed(h, "depth", location=B.MEM_DEVICE)], [(0, 0, None)], LEAF),
        }
        if torch.cuda.device_count() > 1:
            other = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda:1")
            cases["a pointer on another GPU"] = ([dict(img, mask=B.image_view(other))], [(0, 0, None)], LEAF)      # (needs a second GPU to exist)
        for why, (images, frames, leaf) in cases.items():
            with pytest.raises(B.TdloError) as e:
                ctx.frame_views_to_cloud_batch(images, frames, leaf)
            assert e.value.code == B.TDLO_E_INVALID, why
            untouched(why)
        # a host view inside the context's pinned image buffers
        pd, pm = ctx.image_buffers(rows, cols)
        pd[:] = g.canon["depth"]; pm[:] = g.canon["mask"]
        pc, po = ctx.colour_buffers(rows, cols)
        for why, image in (("pinned depth", dict(depth=pd, mask=h.views["mask"], cam=CAM)), ("pinned mask", dict(depth=h.views["depth"], mask=pm, cam=CAM)),
                           ("pinned colour", dict(depth=h.views["depth"], colour=pc, cam=CAM)), ("pinned occluder", dict(img, occluder=po))):
            with pytest.raises(B.TdloError) as e:
                ctx.frame_views_to_cloud_batch([image], [(0, 0, blue if "colour" in image and "mask" not in image else None)], LEAF)
            assert e.value.code == B.TDLO_E_INVALID, why
            untouched(why)
        # a device view that overlaps the resident cloud of a slot the call names -- of ANY such slot, not only the frame's own
        adr, cap = ctx.debug_slot_cloud(2)
        assert adr and cap >= 120 and cap * 24 >= 2 * rows * cols
        inside = B.ImageView(adr + 24 * cap - 2 * rows * cols, B.IMG_U16C1, B.MEM_DEVICE, 2 * cols, None)
        inside.rows, inside.cols = rows, cols
        for frames in ([(2, 0, None)], [(0, 0, None), (2, 0, None)], [(2, 0, None), (1, 0, None)]):
            with pytest.raises(B.TdloError) as e:
                ctx.frame_views_to_cloud_batch([dict(img, depth=inside)], frames, LEAF)
            assert e.value.code == B.TDLO_E_INVALID
            untouched("a view inside slot 2's cloud")
        # bad sizes and null tables, straight through the C ABI (the binding takes the size from the views)
        tab, K, r0, c0, keep = B._view_images([img])
        fr = (B.BatchFrame * 1)(); fr[0].slot, fr[0].image = 0, 0
        n = np.zeros(1, np.int32)
        for r, c in ((0, cols), (rows, 0), (-rows, cols), (1 << 14, (1 << 12) + 1)):
            rc = ctx.lib.tdlo_frame_views_to_cloud_batch(ctx.h, C.cast(tab, C.c_void_p), K, r, c, C.cast(fr, C.c_void_p), 1, LEAF, n.ctypes.data, n.ctypes.data, None)
            assert rc == B.TDLO_E_INVALID, (r, c)
            untouched((r, c))
        for args in ((None, K, C.cast(fr, C.c_void_p)), (C.cast(tab, C.c_void_p), 0, C.cast(fr, C.c_void_p)), (C.cast(tab, C.c_void_p), K, None)):
            assert ctx.lib.tdlo_frame_views_to_cloud_batch(ctx.h, args[0], args[1], rows, cols, args[2], 1, LEAF, None, None, None) == B.TDLO_E_INVALID
            untouched("null tables")
        # the first valid call; then a device view that overlaps the batch arena it left
        ctx2 = vctx(frames=1)
        try:
            run(B, torch, ctx, ctx2, [g], [(3, 0, None), (1, 0, HALF_A)], LEAF, (2, 0, 4), "after the refusals")
        finally:
            ctx2.close()
        clouds[3], clouds[1] = ctx.get_cloud(3), ctx.get_cloud(1)
        zero = counters()
        planes = ctx.view_batch_images(0)
        arena = B.ImageView(planes["depth"], B.IMG_U16C1, B.MEM_DEVICE, 2 * cols, None)
        arena.rows, arena.cols = rows, cols
        with pytest.raises(B.TdloError) as e:
            ctx.frame_views_to_cloud_batch([dict(img, depth=arena)], [(0, 0, None)], LEAF)
        assert e.value.code == B.TDLO_E_INVALID
        untouched("a view inside the arena")
        assert ctx.view_batch_images(0) == planes                                               # a refused call leaves the planes of the last one
    finally:
        ctx.close()


# ---- trackers ------------------------------------------------------------------------------------------------------------------------------------------
def test_trackers_over_twenty_frames_and_the_result_images(B, torch, synth):
    """tdlo_tracker_frame_views_batch on F = 3 trackers over 20 frames against twins stepped by tdlo_tracker_frame_view on a second context (both under
    TDLO_ESTEP2=0): nodes, sigma2, visible sets, n and n_raw; then a tracker whose frame selects nothing; then tdlo_tracker_render_result_batch over the
    colour planes tdlo_view_batch_images returns, byte for byte tdlo_tracker_render_result of the twins."""
    P = synth.LAUNCH_PARAMS
    M, rows, cols, F = 30, 120, 160, 3
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    params = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    nothing = B.make_colour_params(*NOTHING)
    ca, cb = vctx(frames=4, TDLO_ESTEP2=0), vctx(frames=4, TDLO_ESTEP2=0)
    try:
        ta = [B.trackdlo(*args, ctx=ca, slot=i) for i in range(F)]
        tb = [B.trackdlo(*args, ctx=cb, slot=i) for i in range(F)]

        def bits(t):
            return t.get_tracking_result().view(np.uint64).copy(), np.float64(t.get_sigma2()).view(np.uint64)

        def same(a, b):
            return np.array_equal(a[0], b[0]) and a[1] == b[1]

        def scenes(step):
            out = []
            for i in range(F):
                depth, colour, occ, _, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9 + i, frame=step, rows=rows, cols=cols, occluder=(40, 100, 60, 72))
                out.append((depth, colour, occ, (cam["fx"], cam["fy"], cam["cx"], cam["cy"]), Y0))
            return out
        twin_pics = []
        for step in range(20):
            sc = scenes(step)
            if step == 0:
                for i in range(F):
                    for t in (ta[i], tb[i]):
                        t.initialize_nodes(sc[i][4]); t.initialize_geodesic_coord(synth.geodesic_coord(sc[i][4]))
            images = [dict(fv=_sources(B, torch, d, c, o, None, "device" if (i + step) % 3 else "host"), cam=a) for i, (d, c, o, a, _) in enumerate(sc)]
            codes, vis, ext, n, nraw = B.frame_views_batch(ta, images, [0, 1, 2], [params] * F, 0.008, 0.06)
            assert codes == [0] * F and ca.frame_view_batch_route_counts()[:2] == [F * (step + 1), 0], step
            for i, (d, c, o, a, _) in enumerate(sc):
                v1, e1, n1, nraw1 = tb[i].frame_view(_sources(B, torch, d, c, o, None, "device"), params, *a, 0.008, 0.06)
                assert (n1, nraw1) == (n[i], nraw[i]) and n1 > 50 and np.array_equal(v1, vis[i]) and np.array_equal(e1, ext[i]), (step, i)
                assert same(bits(ta[i]), bits(tb[i])), (step, i)
                assert [s["iters"] for s in ta[i].last_stats] == [s["iters"] for s in tb[i].last_stats], (step, i)
                if step == 19:
                    twin_pics.append(tb[i].render_result())               # (now: the twins share a context, whose last colour frame is the one drawn over)
        # the result images over the canonical colour planes of the last call
        pics = []
        for k in range(F):
            pl = ca.view_batch_images(k)
            assert pl["colour"] % 4 == 0 and pl["mask"] is None
            pics.append(dict(colour=B.DevicePlane(pl["colour"], (rows, cols, 3)), occluder=B.DevicePlane(pl["occluder"], (rows, cols))))
        outs, cor = B.render_result_batch(ta, pics, [0, 1, 2])
        for i in range(F):
            img, one = twin_pics[i]
            assert np.array_equal(outs[i], img) and cor[i] == one, i
            assert np.count_nonzero(np.any(outs[i] != sc[i][1], axis=2)) > 500
        # a tracker whose frame selects nothing: TDLO_E_EMPTY, untouched; the others go on
        sc = scenes(20)
        images = [dict(fv=_sources(B, torch, d, c, o, None, "device"), cam=a) for d, c, o, a, _ in sc]
        before = bits(ta[1])
        codes, vis, ext, n, nraw = B.frame_views_batch(ta, images, [0, 1, 2], [params, nothing, params], 0.008, 0.06, check=False)
        assert codes == [0, B.TDLO_E_EMPTY, 0] and n[1] == 0 and nraw[1] == 0 and len(vis[1]) == 0 and same(bits(ta[1]), before)
        with pytest.raises(B.TdloError) as e:
            B.frame_views_batch(ta[1:2], images, [1], [nothing], 0.008, 0.06)
        assert e.value.code == B.TDLO_E_EMPTY and same(bits(ta[1]), before)
        for i in (0, 2):
            d, c, o, a, _ = sc[i]
            tb[i].frame_view(_sources(B, torch, d, c, o, None, "host"), params, *a, 0.008, 0.06)
            assert same(bits(ta[i]), bits(tb[i])), i
    finally:
        ca.close(); cb.close()


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sensor_frames(rows, cols):
    from trackdlo_amd import synth
    out = []
    for f in range(4):
        depth, colour, occ, _, cam, _ = synth.colour_scene(30, *colour_ref.LAUNCH_RANGE, config=9, frame=f, rows=rows, cols=cols)
        out.append((depth, colour, (cam["fx"], cam["fy"], cam["cx"], cam["cy"])))
    return out


@pytest.mark.parametrize("shape", [(480, 640), (720, 1280)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_sensor_sizes(B, torch, shape):
    """K = F = 4 at 640 x 480 and 1280 x 720: RGBA8 + 32FC1 device views, as a renderer's [K, H, W, 4] and [K, H, W] tensors hold them."""
    rows, cols = shape
    ctx, ctx2 = vctx(frames=4), vctx(frames=1)
    try:
        fr = sensor_frames(rows, cols)
        rng = np.random.default_rng(rows)
        rgba = np.empty((4, rows, cols, 4), np.uint8); metres = np.empty((4, rows, cols), np.float32)
        for k, (d, c, _) in enumerate(fr):
            rgba[k, :, :, :3] = c; rgba[k, :, :, 3] = rng.integers(1, 256, (rows, cols), dtype=np.uint8)
            metres[k] = (d / 1000.0).astype(np.float32)
        tc, td = torch.from_numpy(rgba).cuda(), torch.from_numpy(metres).cuda()
        imgs = []
        for k, (d, c, cam) in enumerate(fr):
            im = Img(rows, cols, cam=cam)
            im.views = dict(depth=B.image_view(td[k]), colour=B.image_view(tc[k]))
            im.canon = dict(depth=np.asarray(d), colour=np.asarray(c))
            assert B.image_view_form(im.views["depth"]) == 2 and B.image_view_form(im.views["colour"]) == 2
            imgs.append(im)
        n, nraw = run(B, torch, ctx, ctx2, imgs, [(k, 3 - k, colour_ref.LAUNCH_RANGE) for k in range(4)], 0.008, (4, 0, 8), f"{shape}")
        assert min(n) > 100
    finally:
        ctx.close(); ctx2.close()
