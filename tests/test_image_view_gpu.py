"""GPU suite for image views (tdlo_frame_to_cloud_view, tdlo_frame_to_cloud_visibility_view, tdlo_tracker_frame_view; k_image_import in
csrc/tdlo_image.hip): a frame taken as it arrives -- pitched or bottom-up rows, RGBA8 colour, 32FC1 depth in metres, device or host memory -- must leave,
BYTE FOR BYTE, the canonical images of tests/image_view_ref.py (read back with tdlo_debug_read_images), and everything computed from it must be the
bits of the packed call fed those canonical images.  Every comparison is on bits; there is no tolerance anywhere."""
import numpy as np
import pytest

import colour_ref
import image_view_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (3, 5), (2, 7), (5, 8), (4, 12), (33, 68)]
NOTHING = ([[10, 10, 10]], [[5, 5, 5]])                # a colour range that passes no pixel: the import is under test, not the cloud behind it


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


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(device=0, max_frames=2, max_points=1 << 15, max_nodes=64, timing=False)
    yield c
    c.close()


def _place(B, torch, buf, off, fmt, stride, rows, cols, device):
    """An ImageView of the layout (buf, off, stride) in device memory (a torch byte tensor: its allocation is aligned, so `off` sets data's alignment)
    or in host memory (the numpy buffer itself)."""
    if device:
        owner = torch.from_numpy(buf).cuda()
        addr = owner.data_ptr()
        assert addr % 256 == 0
    else:
        owner = buf
        addr = buf.ctypes.data
    v = B.ImageView(addr + off, fmt, B.MEM_DEVICE if device else B.MEM_HOST, stride, None)
    v.rows, v.cols, v.owner = rows, cols, owner
    return v


def _expect(lay, fmt, rows, cols):
    _, buf, off, stride = lay
    return R.canonical(buf, off, fmt, stride, rows, cols)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_canonical_images_byte_for_byte(B, torch, ctx, shape, device):
    """Every layout of image_view_ref.layouts -- data offsets 0, 1, 2, 4, 8, pitches of row bytes + {0, one element, 4, 12, 16}, bottom-up rows, a poisoned
    alpha byte, every byte outside the rows poisoned -- in all five formats, as colour frames (depth + colour + occluder) and mask frames (depth + mask)."""
    rows, cols = shape
    rng = np.random.default_rng(1000 * rows + cols)
    L = {f: R.layouts(rows, cols, f, rng) for f in (R.U8C1, R.U8C3, R.U8C4, R.U16C1, R.F32C1)}
    nothing = B.make_colour_params(*NOTHING)
    forms = set()
    for k in range(max(len(v) for v in L.values())):
        for dfmt, cfmt in ((R.U16C1, R.U8C3), (R.F32C1, R.U8C4), (R.U16C1, R.U8C4), (R.F32C1, R.U8C3)):
            ld, lc, lo = L[dfmt][k % len(L[dfmt])], L[cfmt][k % len(L[cfmt])], L[R.U8C1][(k + 5) % len(L[R.U8C1])]
            views = [_place(B, torch, lay[1], lay[2], f, lay[3], rows, cols, device) for lay, f in ((ld, dfmt), (lc, cfmt), (lo, R.U8C1))]
            forms.update((f, B.image_view_form(v)) for f, v in zip((dfmt, cfmt, R.U8C1), views))
            # a colour frame: depth + colour + occluder
            _, n, nraw = ctx.frame_to_cloud_view(0, B.frame_view(views[0], views[1], views[2]), nothing, 600.0, 600.0, cols / 2, rows / 2, 0.05)
            assert n == 0 and nraw == 0
            got = ctx.debug_read_images(rows, cols, depth=True, colour=True, occluder=True)
            for name, lay, f in (("depth", ld, dfmt), ("colour", lc, cfmt), ("occluder", lo, R.U8C1)):
                np.testing.assert_array_equal(got[name], _expect(lay, f, rows, cols), err_msg=f"{name} {lay[0]} format {f} frame {k}")
        # a mask frame: depth + mask (random bytes: n_raw counts the nonzero ones; a leaf of a metre keeps the cloud behind it small)
        for dfmt in (R.U16C1, R.F32C1):
            ld, lm = L[dfmt][(k + 3) % len(L[dfmt])], L[R.U8C1][k % len(L[R.U8C1])]
            vd = _place(B, torch, ld[1], ld[2], dfmt, ld[3], rows, cols, device)
            vm = _place(B, torch, lm[1], lm[2], R.U8C1, lm[3], rows, cols, device)
            _, n, nraw = ctx.frame_to_cloud_view(0, B.frame_view(vd, mask=vm), None, 600.0, 600.0, cols / 2, rows / 2, 1.0)
            want = _expect(lm, R.U8C1, rows, cols)
            assert nraw == np.count_nonzero(want)
            got = ctx.debug_read_images(rows, cols, depth=True, mask=True)
            np.testing.assert_array_equal(got["depth"], _expect(ld, dfmt, rows, cols), err_msg=f"depth {ld[0]} format {dfmt} frame {k}")
            np.testing.assert_array_equal(got["mask"], want, err_msg=f"mask {lm[0]} frame {k}")
            with pytest.raises(B.TdloError):
                ctx.debug_read_images(rows, cols, colour=True)                     # the frame had no colour image
    if cols % 4 == 0:                                                              # every vector form was taken, and the element-wise one beside it
        assert forms >= {(R.U8C1, 1), (R.U8C3, 1), (R.U8C4, 1), (R.U8C4, 2), (R.U16C1, 1), (R.U16C1, 2), (R.F32C1, 1), (R.F32C1, 2), (R.U8C1, 0), (R.U16C1, 0)}, forms
    else:
        assert {f for _, f in forms} == {0}


def test_numpy_arrays_through_image_view(B, ctx):
    """The same from numpy arrays handed to image_view(): a slice of a wider image (rows not contiguous), a flipped one, uint16 carried in int16."""
    rng = np.random.default_rng(5)
    rows, cols = 9, 20
    big = rng.integers(0, 256, (rows + 2, cols + 7, 4), dtype=np.uint8)
    colour = big[1:1 + rows, 3:3 + cols][::-1]
    depth16 = rng.integers(0, 32768, (rows, cols + 3)).astype(np.int16)[:, 2:2 + cols]
    occ = (rng.random((rows, cols * 2)) < 0.5).astype(np.uint8)[:, :cols] * 255
    fv = B.frame_view(B.image_view(depth16, format=B.IMG_U16C1), colour, occ)
    ctx.frame_to_cloud_view(0, fv, B.make_colour_params(*NOTHING), 600.0, 600.0, 10.0, 4.5, 0.05)
    got = ctx.debug_read_images(rows, cols, depth=True, colour=True, occluder=True)
    np.testing.assert_array_equal(got["depth"], depth16.astype(np.uint16))
    np.testing.assert_array_equal(got["colour"], colour[:, :, :3])
    np.testing.assert_array_equal(got["occluder"], occ)


@pytest.mark.parametrize("shape", [(480, 640), (720, 1280)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sensor_sizes(B, torch, ctx, shape):
    rows, cols = shape
    rng = np.random.default_rng(rows)
    nothing = B.make_colour_params(*NOTHING)
    mm = rng.integers(0, 65536, (rows, cols)).astype(np.uint16)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    # packed 3-channel + U16, as the camera driver delivers them
    fv = B.frame_view(B.image_view(torch.from_numpy(mm.view(np.int16)).cuda(), format=B.IMG_U16C1), torch.from_numpy(bgr).cuda())      # (uint16 carried in int16)
    ctx.frame_to_cloud_view(0, fv, nothing, 600.0, 600.0, cols / 2, rows / 2, 0.05)
    got = ctx.debug_read_images(rows, cols, depth=True, colour=True)
    assert np.array_equal(got["depth"], mm) and np.array_equal(got["colour"], bgr)
    # RGBA + F32, pitched, as a renderer delivers them
    rgba = np.full((rows, cols + 16, 4), 0xA5, dtype=np.uint8)
    rgba[:, :cols, :3] = bgr; rgba[:, :cols, 3] = rng.integers(1, 256, (rows, cols), dtype=np.uint8)
    metres = np.full((rows, cols + 4), 1.2345, dtype=np.float32)
    metres[:, :cols] = (mm / 1000.0).astype(np.float32)
    tc, td = torch.from_numpy(rgba).cuda(), torch.from_numpy(metres).cuda()
    fv = B.frame_view(td[:, :cols], tc[:, :cols])
    assert (fv.colour.format, fv.colour.row_stride, fv.depth.format, fv.depth.row_stride) == (B.IMG_U8C4, 4 * (cols + 16), B.IMG_F32C1, 4 * (cols + 4))
    assert R.canonical(metres, 0, R.F32C1, 4 * (cols + 4), rows, cols).tobytes() == mm.tobytes()      # the k / 1000 round trip, by the statement
    ctx.frame_to_cloud_view(0, fv, nothing, 600.0, 600.0, cols / 2, rows / 2, 0.05)
    got = ctx.debug_read_images(rows, cols, depth=True, colour=True)
    assert np.array_equal(got["depth"], mm) and np.array_equal(got["colour"], bgr)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _sources(B, torch, depth, colour, occ, mask, kind):
    """The frame's images in another shape than the packed calls take.  'device': RGBA8 with a poisoned alpha + float32 metres, both bottom-up, pitched, in
    device memory; 'host': pitched numpy images (BGR rows of cols * 3 + 5 bytes, uint16 depth with 3 spare pixels a row)."""
    rows, cols = depth.shape
    rng = np.random.default_rng(7)
    if kind == "host":
        c = np.full((rows, cols * 3 + 5), 0xA5, dtype=np.uint8); c[:, :cols * 3] = colour.reshape(rows, -1)
        d = np.full((rows, cols + 3), 777, dtype=np.uint16); d[:, :cols] = depth
        vc = B.ImageView(c.ctypes.data, B.IMG_U8C3, B.MEM_HOST, c.strides[0], None); vc.rows, vc.cols, vc.owner = rows, cols, c
        wrap = lambda a: None if a is None else B.image_view(np.pad(a, ((0, 0), (0, 9)), constant_values=0xA5)[:, :cols])
        return B.frame_view(B.image_view(d[:, :cols]), vc if mask is None else None, wrap(occ), wrap(mask))

    def flipped(a):                                               # the image stored bottom-up behind a positive pitch: data = its last stored row, stride < 0
        t = torch.from_numpy(np.ascontiguousarray(a[::-1])).cuda()
        pitch = t.stride(0) * t.element_size()
        fmt = {(torch.uint8, 2): B.IMG_U8C1, (torch.uint8, 3): B.IMG_U8C4, (torch.float32, 2): B.IMG_F32C1}[(t.dtype, t.dim())]
        v = B.ImageView(t.data_ptr() + (rows - 1) * pitch, fmt, B.MEM_DEVICE, -pitch, None)
        v.rows, v.cols, v.owner = rows, cols, t
        return v
    rgba = np.full((rows, cols + 2, 4), 0xA5, dtype=np.uint8)
    rgba[:, :cols, :3] = colour; rgba[:, :cols, 3] = rng.integers(1, 256, (rows, cols), dtype=np.uint8)
    metres = np.full((rows, cols + 1), 1.2345, dtype=np.float32); metres[:, :cols] = (depth / 1000.0).astype(np.float32)
    pad = lambda a: None if a is None else flipped(np.pad(a, ((0, 0), (0, 4)), constant_values=0xA5))
    return B.frame_view(flipped(metres), flipped(rgba) if mask is None else None, pad(occ), pad(mask))


@pytest.mark.parametrize("kind", ["device", "host"])
def test_clouds_and_visibility_against_the_packed_calls(B, torch, synth, kind):
    M, rows, cols = 30, 120, 160
    params = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    depth, colour, occ, mask, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=1, rows=rows, cols=cols, occluder=(40, 100, 60, 72))
    a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    coord = synth.geodesic_coord(Y0)
    ca, cb = B.Context(device=0, timing=False), B.Context(device=0, timing=False)
    try:
        # the mask route, then the colour route: the cloud, n, n_raw
        Xp, n, nraw = ca.depth_to_cloud(0, depth, mask, *a, 0.008)
        Xv, nv, nrawv = cb.frame_to_cloud_view(0, _sources(B, torch, depth, colour, None, mask, kind), None, *a, 0.008)
        assert (n, nraw) == (nv, nrawv) and n > 100 and np.array_equal(_bits(Xp), _bits(Xv))
        np.testing.assert_array_equal(cb.debug_read_images(rows, cols, mask=True)["mask"], mask)
        Xp, n, nraw = ca.colour_depth_to_cloud(0, depth, colour, params, occ, *a, 0.008)
        Xv, nv, nrawv = cb.frame_to_cloud_view(0, _sources(B, torch, depth, colour, occ, None, kind), params, *a, 0.008)
        assert (n, nraw) == (nv, nrawv) and n > 100 and np.array_equal(_bits(Xp), _bits(Xv))
        assert np.array_equal(_bits(ca.get_cloud(0)), _bits(cb.get_cloud(0)))
        # the _visibility forms
        for m, o, p in ((mask, None, None), (None, occ, params)):
            if m is not None:
                want = ca.depth_to_cloud_visibility(0, depth, m, *a, 0.008, Y0, 0.008, 0.06, coord)
            else:
                want = ca.colour_depth_to_cloud_visibility(0, depth, colour, p, o, *a, 0.008, Y0, 0.008, 0.06, coord)
            got = cb.frame_to_cloud_visibility_view(0, _sources(B, torch, depth, colour, o, m, kind), p, *a, 0.008, Y0, 0.008, 0.06, coord)
            assert np.array_equal(_bits(want[0]), _bits(got[0])) and list(want[1]) == list(got[1]) and list(want[2]) == list(got[2]) and want[3:] == got[3:]
            assert len(got[1]) > 0
    finally:
        ca.close(); cb.close()


@pytest.mark.parametrize("kind", ["device", "host"])
def test_tracker_frames_and_result_image(B, torch, synth, kind):
    P = synth.LAUNCH_PARAMS
    M, rows, cols = 30, 120, 160
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    params = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    ca, cb = B.Context(device=0, timing=False), B.Context(device=0, timing=False)
    try:
        ta, tb = B.trackdlo(*args, ctx=ca), B.trackdlo(*args, ctx=cb)
        for f in range(3):
            depth, colour, occ, _, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=f, rows=rows, cols=cols, occluder=(40, 100, 60, 72))
            a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
            if f == 0:
                for t in (ta, tb):
                    t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
            want = ta.frame_from_colour(depth, colour, params, occ, *a, 0.008, 0.06)
            got = tb.frame_view(_sources(B, torch, depth, colour, occ, None, kind), params, *a, 0.008, 0.06)
            assert list(want[0]) == list(got[0]) and list(want[1]) == list(got[1]) and want[2:] == got[2:], f
            assert np.array_equal(_bits(ta.get_tracking_result()), _bits(tb.get_tracking_result())), f
            assert np.float64(ta.get_sigma2()).view(np.uint64) == np.float64(tb.get_sigma2()).view(np.uint64), f
            assert [s["iters"] for s in ta.last_stats] == [s["iters"] for s in tb.last_stats]
            ia, cora = ta.render_result()
            ib, corb = tb.render_result()
            assert np.array_equal(ia, ib) and cora == corb == [40, 60, 99, 71], f
            assert np.count_nonzero(np.any(ib != colour, axis=2)) > 500          # (a picture was drawn over this frame's colour image)
    finally:
        ca.close(); cb.close()


def test_ready_stream(B, torch, ctx):
    """An image filled by torch kernels on another stream, behind enough work that they have not run when the view call is made, handed over with that
    stream as ready_stream and no host wait: the same bytes."""
    rows, cols = 240, 320
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
    fv = B.frame_view(B.image_view(dst_d, ready_stream=side.cuda_stream), B.image_view(dst_c, ready_stream=side.cuda_stream))
    ctx.frame_to_cloud_view(0, fv, B.make_colour_params(*NOTHING), 600.0, 600.0, cols / 2, rows / 2, 0.05)
    got = ctx.debug_read_images(rows, cols, depth=True, colour=True)
    assert np.array_equal(got["depth"], mm) and np.array_equal(got["colour"], bgra[:, :, :3])
    torch.cuda.synchronize()


def test_refusals_touch_nothing(B, torch, synth):
    P = synth.LAUNCH_PARAMS
    M, rows, cols = 30, 120, 160
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    params = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    depth, colour, occ, mask, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=0, rows=rows, cols=cols, occluder=(40, 100, 60, 72))
    a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    c = B.Context(device=0, timing=False)
    try:
        t = B.trackdlo(*args, ctx=c)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
        t.frame_from_colour(depth, colour, params, occ, *a, 0.008, 0.06)
        cloud, nodes, sigma2 = c.get_cloud(0), t.get_tracking_result(), t.get_sigma2()
        image, _ = t.render_result()

        def overlapping():                                         # rows that overlap: fails tdlo_image_view_check
            fv = _sources(B, torch, depth, colour, occ, None, "device")
            fv.colour.row_stride = -(4 * cols - 4)
            return fv

        def misaligned():
            fv = _sources(B, torch, depth, colour, occ, None, "host")
            fv.depth.data += 1
            return fv

        def wrong_format():
            fv = _sources(B, torch, depth, colour, occ, None, "host")
            fv.depth.format = B.IMG_U8C1
            return fv

        def both():                                                # a mask AND a colour image
            fv = _sources(B, torch, depth, colour, None, mask, "host")
            fv.colour = B.image_view(colour)
            return fv

        def neither():
            return B.frame_view(B.image_view(depth))

        for make in (overlapping, misaligned, wrong_format, both, neither):
            for call in (lambda fv: c.frame_to_cloud_view(0, fv, params, *a, 0.008), lambda fv: t.frame_view(fv, params, *a, 0.008, 0.06),
                         lambda fv: c.frame_to_cloud_visibility_view(0, fv, params, *a, 0.008, Y0, 0.008, 0.06, synth.geodesic_coord(Y0))):
                with pytest.raises(B.TdloError) as e:
                    call(make())
                assert e.value.code == B.TDLO_E_INVALID, make.__name__
                assert np.array_equal(_bits(c.get_cloud(0)), _bits(cloud)), make.__name__
                assert np.array_equal(_bits(t.get_tracking_result()), _bits(nodes)) and t.get_sigma2() == sigma2, make.__name__
        assert np.array_equal(t.render_result()[0], image)          # ... and the last colour frame is still the one to draw over
        # the context serves the next frame
        t.frame_view(_sources(B, torch, depth, colour, occ, None, "device"), params, *a, 0.008, 0.06)
    finally:
        c.close()
