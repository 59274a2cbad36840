"""The tracking-result image on the device (tdlo_render_result / tdlo_tracker_render_result, k_render in csrc/tdlo_render.hip) against the numpy statement
tests/render_ref.py, byte for byte.  The inputs come from tests/render_cases.py; tests/test_render_ref.py confirms on a machine without a GPU that they
pass the reference's guards."""
import numpy as np
import pytest

import colour_ref
import render_cases as K
import render_ref as R
from trackdlo_amd import binding as B, synth

pytestmark = pytest.mark.gpu

CANARY = 64


@pytest.fixture(scope="module")
def ctx():
    c = B.Context(device=0, timing=False)
    yield c
    c.close()


def _params(c):
    return B.make_render_params(**c["params"]) if c["params"] else None


def _want(c):
    return R.render(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"], c["params"])


def _render_with_canary(ctx, c):
    """render_result twice, each time into the front of a buffer whose last 64 bytes must stay as they are.  A pageable numpy array receives a copy of the
    context's device image, so its canary guards the length of that copy; a device tensor is written by k_render itself (unless TDLO_RENDER_INPLACE=0),
    so its canary guards the kernel's own stores, the byte-wise tail of an image with rows * cols % 4 != 0 among them.  Both images must agree."""
    import torch
    rows, cols = c["colour"].shape[:2]
    n = 3 * rows * cols
    buf = np.full(n + CANARY, 0xa5, dtype=np.uint8)
    img, cor = ctx.render_result(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"], _params(c), out=buf[:n].reshape(rows, cols, 3))
    assert np.all(buf[n:] == 0xa5), "bytes behind image_out were written"
    dev = torch.full((n + CANARY,), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _, dcor = ctx.render_result(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"], _params(c), out=dev[:n].view(rows, cols, 3))
    host = dev.cpu().numpy()
    assert np.all(host[n:] == 0xa5), "bytes behind the device image were written"
    assert np.array_equal(host[:n].reshape(rows, cols, 3), img) and dcor == cor, "the device destination differs from the host one"
    return img, cor


def _check(ctx, c, name=""):
    want, wcor = _want(c)
    img, cor = _render_with_canary(ctx, c)
    bad = np.argwhere(np.any(img != want, axis=2))
    assert len(bad) == 0, (name, len(bad), bad[:5].tolist())
    assert cor == wcor, (name, cor, wcor)
    return want


# ---- 1 .. 4: shapes, borders, order, many primitives per wave -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.shapes()))
def test_small_shapes_and_every_kind_of_edge(ctx, name):
    c = K.shapes()[name]
    want = _check(ctx, c, name)
    if len(c["Y"]) == 1:
        assert np.array_equal(want, R.blend(c["colour"], c["occluder"]))          # one node: the blend alone


@pytest.mark.parametrize("name", sorted(K.borders()))
def test_borders_and_nodes_outside_the_image(ctx, name):
    _check(ctx, K.borders()[name], name)


def test_a_rope_that_crosses_itself_is_drawn_farthest_first(ctx):
    cases = K.crossing()
    wants = {k: _check(ctx, c, k) for k, c in cases.items()}
    assert not np.array_equal(wants["all"], wants["none"]) and not np.array_equal(wants["all"], wants["mixed"])
    # the picture depends on the order: the same primitives painted in index order give another image
    c = cases["mixed"]
    prims = R.primitives(c["Y"], c["proj"], c["vis"])
    order = R.edge_order(c["Y"])
    by_index = np.concatenate([prims[3 * order.index(i):3 * order.index(i) + 3] for i in range(len(order))])
    assert not np.array_equal(R.paint(R.blend(c["colour"], c["occluder"]), by_index), wants["mixed"])


def test_more_than_64_primitives_per_wave(ctx):
    c = K.zigzag(300)
    prims = R.primitives(c["Y"], c["proj"], c["vis"])
    rows, cols = c["colour"].shape[:2]
    for first in range(0, rows * cols, 256):                  # every wave's row span meets more than 64 bounding boxes
        r_lo, r_hi = first // cols, min(first + 255, rows * cols - 1) // cols
        assert sum(1 for p in prims if p[0] == 0 and min(p[2], p[4]) - 3 <= r_hi and max(p[2], p[4]) + 3 >= r_lo) > 64
    _check(ctx, c, "zigzag/300")


def test_1024_nodes():
    big = B.Context(device=0, max_nodes=1024, timing=False)
    try:
        _check(big, K.zigzag(1024, 31), "zigzag/1024")
    finally:
        big.close()


# ---- 5: blend and corners -----------------------------------------------------------------------------------------------------------------------------
def test_the_blend_over_every_byte_pair(ctx):
    c = K.all_byte_pairs()
    want = _check(ctx, c, "blend")
    assert np.array_equal(want, R.blend(c["colour"], c["occluder"]))


@pytest.mark.parametrize("name", sorted(K.corner_cases()))
def test_occlusion_corners(ctx, name):
    c = K.corner_cases()[name]
    _check(ctx, c, name)
    _, cor = ctx.render_result(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"])
    rows, cols = c["colour"].shape[:2]
    assert cor == dict(none=[-1] * 4, first=[0, 0, 0, 0], last=[rows - 1, cols - 1] * 2, rect=[7, 21, 18, 39])[name.replace("no-occluder", "none")]
    img, none = ctx.render_result(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"], corners=False)          # corners == NULL
    assert none is None and np.array_equal(img, _want(c)[0])


# ---- 6: where the bytes come from and go ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", ["default", "0"])
def test_sources_and_destinations(monkeypatch, inplace):
    import torch
    if inplace == "0":
        monkeypatch.setenv("TDLO_RENDER_INPLACE", "0")
    c = K.shapes()["47x53-mixed"]
    rows, cols = c["colour"].shape[:2]
    want, wcor = _want(c)
    cx = B.Context(device=0, timing=False)
    try:
        cbuf, obuf = cx.colour_buffers(rows, cols)
        cbuf[:] = c["colour"]; obuf[:] = c["occluder"]
        pinned = cx.result_image_buffer(rows, cols)
        dev = torch.full((3 * rows * cols + CANARY,), 0xa5, dtype=torch.uint8, device="cuda")
        for source in ("pageable", "colour_buffers", "null"):
            for dest in ("pageable", "pinned", "device"):
                if source == "null":          # the images of the last colour call, read where it left them: its device copy, then the pinned buffers
                    for a, o in ((c["colour"], c["occluder"]), (cbuf, obuf)):
                        cx.colour_mask(a, B.make_colour_params(*colour_ref.LAUNCH_RANGE), o)
                        before = cx.render_route_counts()
                        img, cor = _one(cx, c, None, None, dest, pinned, dev, torch)
                        _routes(cx, before, dest, inplace)
                        assert np.array_equal(img, want) and cor == wcor, (source, dest)
                    continue
                a, o = (c["colour"], c["occluder"]) if source == "pageable" else (cbuf, obuf)
                before = cx.render_route_counts()
                img, cor = _one(cx, c, a, o, dest, pinned, dev, torch)
                _routes(cx, before, dest, inplace)
                assert np.array_equal(img, want) and cor == wcor, (source, dest)
        assert bool((dev[3 * rows * cols:] == 0xa5).all()), "bytes behind the device image were written"
    finally:
        cx.close()


def _one(cx, c, colour, occluder, dest, pinned, dev, torch):
    rows, cols = c["colour"].shape[:2]
    if dest == "pageable":
        return cx.render_result(colour, occluder, c["Y"], c["proj"], c["vis"], shape=(rows, cols))
    if dest == "pinned":
        pinned[:] = 0
        img, cor = cx.render_result(colour, occluder, c["Y"], c["proj"], c["vis"], shape=(rows, cols), out=pinned)
        return img.copy(), cor
    dev[:3 * rows * cols] = 0
    torch.cuda.synchronize()
    t = dev[:3 * rows * cols].view(rows, cols, 3)
    _, cor = cx.render_result(colour, occluder, c["Y"], c["proj"], c["vis"], shape=(rows, cols), out=t)
    return t.cpu().numpy(), cor


def _routes(cx, before, dest, inplace):
    now = cx.render_route_counts()
    direct = dest != "pageable" and inplace == "default"
    assert [now[0] - before[0], now[1] - before[1]] == ([1, 0] if direct else [0, 1]), (dest, inplace, before, now)


# ---- 7: the tracker -----------------------------------------------------------------------------------------------------------------------------------
# The self-occlusion test's line width for the tracker test.  The scene's rope never crosses itself in the image and its nodes lie about 5 pixels apart
# at 160 columns, so the reference's width of 3 hides nothing: the not-self-occluded set would be every node, as without the test.  At 10 pixels an edge
# reaches the nodes next to its own ends, and which of them it covers hangs on the sub-pixel position of the nodes: the set is a proper subset and
# changes when the nodes move by a fraction of a pixel, which a tracking step does.
PAINTER_WIDTH = 10


@pytest.mark.parametrize("painter", [False, True])
def test_tracker_frames(painter):
    P = synth.LAUNCH_PARAMS
    M, rows, cols = 30, 120, 160
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    params = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    ca, cb = B.Context(device=0, timing=False), B.Context(device=0, timing=False)
    try:
        ta, tb = B.trackdlo(*args, ctx=ca), B.trackdlo(*args, ctx=cb)          # tb never renders
        proj = None
        decided = 0          # frames on which "the nodes the frame STARTED from" gives another set, and another picture, than the result nodes would
        for f in range(4):
            depth, colour, occ, _, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=f, rows=rows, cols=cols, occluder=(40, 100, 60, 72))
            a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
            if f == 0:
                proj = R.pinhole(*a)
                for t in (ta, tb):
                    t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
                    if painter:
                        t.set_self_occlusion(proj.reshape(3, 4), PAINTER_WIDTH)
            start = ta.get_tracking_result()
            ta.frame_from_colour(depth, colour, params, occ, *a, 0.008, 0.06)
            tb.frame_from_colour(depth, colour, params, occ, *a, 0.008, 0.06)
            img, cor = ta.render_result()
            Ya = ta.get_tracking_result()
            assert np.array_equal(Ya.view(np.uint64), tb.get_tracking_result().view(np.uint64)), f      # rendering leaves the tracker alone
            if painter:
                vis = B.self_occlusion_visible(start, proj, PAINTER_WIDTH, np.zeros(M), np.inf)
                late = B.self_occlusion_visible(Ya, proj, PAINTER_WIDTH, np.zeros(M), np.inf)          # (the wrong rule: the set of the result nodes)
                print(f"frame {f}: vis from the start nodes {[int(k) for k in vis]}, from the result nodes {[int(k) for k in late]}")
                assert 0 < len(vis) < M, (f, len(vis))          # neither every node nor none: the set is the test's, not a constant
                if list(vis) != list(late):
                    other, _ = R.render(colour, occ, Ya, proj, late)
                    decided += int(not np.array_equal(other, R.render(colour, occ, Ya, proj, vis)[0]))
            else:
                vis = np.arange(M)
            want, wcor = R.render(colour, occ, Ya, proj, vis)
            assert np.array_equal(img, want) and cor == wcor == [40, 60, 99, 71], (f, cor, wcor)
            assert np.count_nonzero(np.any(want != R.blend(colour, occ), axis=2)) > 500          # (a rope was drawn)
            if painter:
                assert not np.array_equal(want, R.render(colour, occ, Ya, proj, np.arange(M))[0]), f      # the set decides pixels: not the picture of "every node"
            # an explicit matrix and the defaults' struct give the same picture
            img2, _ = ta.render_result(proj, B.make_render_params())
            assert np.array_equal(img2, want)
        assert decided >= 1 or not painter, "on no frame did the start nodes' set differ from the result nodes': the rule is not tested"
    finally:
        ca.close(); cb.close()


# ---- 8: sensor-size frames ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(480, 640), (720, 1280)])
def test_sensor_size_frames(ctx, shape):
    c = K.bench_frame(*shape)
    want = _check(ctx, c, str(shape))
    assert np.count_nonzero(np.any(want != R.blend(c["colour"], c["occluder"]), axis=2)) > 3000


# ---- 9: errors leave image_out untouched -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["w<=0", "nan", "beyond", "vis", "line_width", "fresh-null", "shape"])
def test_refusals_leave_the_image_untouched(what):
    c = dict(K.shapes()["48x53-mixed"])
    rows, cols = c["colour"].shape[:2]
    Y = np.array(c["Y"]); vis = c["vis"]; params = None; colour, occ = c["colour"], c["occluder"]
    shape = (rows, cols)
    cx = B.Context(device=0, timing=False)
    try:
        if what == "w<=0":
            Y[2, 2] = 0.0
        elif what == "nan":
            Y[1, 0] = np.nan
        elif what == "beyond":
            Y[3] = R.nodes_from_pixels([(9000, 3)], K.FX)[0]
        elif what == "vis":
            vis = np.array([0, len(Y)], dtype=np.int32)
        elif what == "line_width":
            params = B.make_render_params(line_width=0)
        elif what == "fresh-null":
            colour = occ = None
            with pytest.raises(B.TdloError):          # (no colour call yet: the library has no shape to tell)
                cx.last_colour_shape()
        else:
            cx.colour_mask(colour, B.make_colour_params(*colour_ref.LAUNCH_RANGE), occ)
            img, _ = cx.render_result(None, None, Y, c["proj"], vis, shape=shape)          # (the same shape is served)
            assert np.array_equal(img, _want(c)[0])
            assert cx.last_colour_shape() == (rows, cols)
            colour = occ = None
            shape = (rows + 1, cols)
        for dest in ("pageable", "pinned"):
            out = cx.result_image_buffer(*shape) if dest == "pinned" else np.zeros(shape + (3,), dtype=np.uint8)
            out[:] = 0x3c
            with pytest.raises(B.TdloError) as e:
                cx.render_result(colour, occ, Y, c["proj"], vis, params, shape=shape, out=out)
            assert e.value.code == B.TDLO_E_INVALID and np.all(out == 0x3c), (what, dest)
        ok, _ = cx.render_result(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"])          # the context serves the next call
        assert np.array_equal(ok, _want(c)[0])
    finally:
        cx.close()
