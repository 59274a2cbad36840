"""GPU suite for depth aligned to the colour camera (tdlo_align_depth, tdlo_frame_to_cloud_view_aligning, tdlo_tracker_frame_view_aligning; k_align_splat and
k_align_pack in csrc/tdlo_align.hip): the aligned plane and the four counts must be, BIT FOR BIT, those of the numpy statement (tests/align_ref.py) on every
scene, from host and device sources, into host and device destinations between canary bytes; the composed calls must be tdlo_align_depth followed by the view
call on a device view of the aligned plane, made by hand on a second context.  Every comparison is on bits; there is no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref as AR
import colour_ref

pytestmark = pytest.mark.gpu

SCENES = AR.all_scenes()
_REF = {}


def ref(name):
    if name not in _REF:
        A, n = AR.align(SCENES[name]["D"], SCENES[name]["p"])
        A.setflags(write=False)
        _REF[name] = (A, n)
    return _REF[name]


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


def _view(B, torch, D, kind, device):
    """An ImageView of D laid out as `kind` (packed, pitched, bottom_up) in host or device memory"""
    buf, off, stride = AR.as_view_array(D, kind)
    owner = torch.from_numpy(buf.view(np.int16) if buf.dtype == np.uint16 else buf).cuda() if device else buf
    base = owner.data_ptr() if device else buf.ctypes.data
    v = B.ImageView(base + off, B.IMG_F32C1 if D.dtype == np.float32 else B.IMG_U16C1, B.MEM_DEVICE if device else B.MEM_HOST, stride, None)
    v.rows, v.cols, v.owner = D.shape[0], D.shape[1], owner
    return v


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("name", list(SCENES))
def test_plane_and_counts_against_the_statement(B, torch, ctx, name, device):
    """every scene, as a packed, a pitched and a bottom-up view: the plane copied out to host memory and the counts"""
    A, n = ref(name)
    p = B.make_align_params(**SCENES[name]["p"])
    for kind in ("packed", "pitched", "bottom_up"):
        before = ctx.align_route_counts()
        G, gn, plane = ctx.align_depth(_view(B, torch, SCENES[name]["D"], kind, device), p)
        assert gn == n and np.array_equal(G, A), (name, kind, gn, n, int((G != A).sum()))
        assert plane != 0 and ctx.align_route_counts() == [before[0] + 1, before[1]]


@pytest.mark.parametrize("name", ["upscale", "border", "5x7", "1x65", "ratio20_mf64", "all_zero"])
def test_destinations_between_canaries_and_the_device_plane(B, torch, ctx, name):
    """aligned_out in host memory and in device memory at an address aligned to 2 bytes but not to 4; the bytes on both sides of each stay; the context's
    device plane holds the same bits; aligned_out = NULL copies nothing"""
    A, n = ref(name)
    p = B.make_align_params(**SCENES[name]["p"])
    P = A.size
    D = SCENES[name]["D"]
    hostbuf = np.full(P + 16, 0xBEEF, np.uint16)
    out = hostbuf[8:8 + P]
    _, gn, plane = ctx.align_depth(D, p, out=out)
    assert gn == n and np.array_equal(out.reshape(A.shape), A) and (hostbuf[:8] == 0xBEEF).all() and (hostbuf[8 + P:] == 0xBEEF).all()
    dev = torch.full((P + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
    addr = dev.data_ptr() + 2 * 7                                                    # 2-byte aligned, not 4-byte aligned
    assert addr % 4 == 2
    _, gn, _ = ctx.align_depth(_view(B, torch, D, "packed", True), p, out=addr)
    torch.cuda.synchronize()
    got = dev.cpu().numpy().view(np.uint16)
    assert gn == n and np.array_equal(got[7:7 + P].reshape(A.shape), A) and (got[:7] == 0x5A5A).all() and (got[7 + P:] == 0x5A5A).all()
    # the context's plane (valid until the next align call), read back as the canonical depth image of a view call on a device view of it
    nothing, gn, plane = ctx.align_depth(D, p, out=None)
    assert nothing is None and gn == n and plane != 0
    v = B.ImageView(plane, B.IMG_U16C1, B.MEM_DEVICE, 2 * A.shape[1], None); v.rows, v.cols = A.shape
    mask = torch.full(A.shape, 255, dtype=torch.uint8, device="cuda")
    ctx.frame_to_cloud_view(0, B.frame_view(v, mask=B.image_view(mask)), None, 50.0, 50.0, A.shape[1] / 2, A.shape[0] / 2, 1.0, fetch=False)
    assert np.array_equal(ctx.debug_read_images(A.shape[0], A.shape[1], depth=True)["depth"], A)


def test_stale_state_and_size_changes_on_one_context(B, torch):
    """a full plane, then the same size with an all-zero depth image: all zeros (the pack arms the scratch again); then a smaller and a larger size"""
    c = B.Context(device=0, max_frames=1, max_points=1 << 14, max_nodes=64, timing=False)
    try:
        s = SCENES["downscale"]
        p = B.make_align_params(**s["p"])
        A, n = ref("downscale")
        for device in (False, True):
            G, gn, _ = c.align_depth(_view(B, torch, s["D"], "packed", device), p)
            assert np.array_equal(G, A) and gn == n and (A != 0).all()
            G, gn, _ = c.align_depth(_view(B, torch, np.zeros_like(s["D"]), "packed", device), p)
            assert not G.any() and gn == [0, 0, 0, 0]
        for name in ("5x7", "upscale", "1x1", "ratio20_mf64", "downscale", "border", "3x257"):      # smaller, larger, smaller ... on the same buffers
            G, gn, _ = c.align_depth(SCENES[name]["D"], B.make_align_params(**SCENES[name]["p"]))
            assert np.array_equal(G, ref(name)[0]) and gn == ref(name)[1], name
        assert c.align_route_counts() == [11, 0]
    finally:
        c.close()


def test_full_size(B, torch, ctx):
    """640 x 480 -> 1280 x 720: a rope-like depth band with 30 % holes"""
    s = AR.scene_rope()
    A, n = AR.align(s["D"], s["p"])
    p = B.make_align_params(**s["p"])
    for device in (True, False):
        G, gn, _ = ctx.align_depth(_view(B, torch, s["D"], "packed", device), p)
        assert gn == n and np.array_equal(G, A) and n[1] > 5000


def test_ready_stream(B, torch, ctx):
    """a depth image filled on another stream behind enough work that it has not run when the call is made, handed over with ready_stream"""
    s = SCENES["upscale"]
    src = torch.from_numpy(s["D"].view(np.int16)).cuda()
    dst = torch.zeros_like(src)
    big = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):
            big = big @ big * 1e-4
        dst.copy_(src)
    G, gn, _ = ctx.align_depth(B.image_view(dst, format=B.IMG_U16C1, ready_stream=side.cuda_stream), B.make_align_params(**s["p"]))
    assert np.array_equal(G, ref("upscale")[0]) and gn == ref("upscale")[1]
    torch.cuda.synchronize()


_HOST_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import align_ref as AR
from trackdlo_amd import binding as B
import torch
c = B.Context(device=0, max_frames=1, max_points=1 << 14, max_nodes=64, timing=False)
sc = AR.all_scenes()
calls = 0
for name, s in sc.items():
    A, n = AR.align(s["D"], s["p"])
    p = B.make_align_params(**s["p"])
    D = s["D"]
    dev = torch.from_numpy(D.view(np.int16) if D.dtype == np.uint16 else D).cuda()
    for src in (D, B.image_view(dev, format=B.IMG_F32C1 if D.dtype == np.float32 else B.IMG_U16C1)):
        G, gn, _ = c.align_depth(src, p)
        calls += 1
        assert np.array_equal(G, A) and gn == n, (name, gn, n)
        assert c.align_route_counts() == [0, calls]
c.close()
print("host route ok", calls)
"""


def test_the_host_route_gives_the_same_bits(B):
    """TDLO_ALIGN=host (read when the context is made), in a child process: every scene from host and device sources; counter 60 counts, 59 stays 0"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _HOST_SCRIPT, root], env=dict(os.environ, TDLO_ALIGN="host"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "host route ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the composed calls against the composition by hand ----------------------------------------------------------------------------------------------
def _two_streams(synth, M, frame, occluder=None):
    """A frame as a sensor with two raw streams delivers it: colour, occluder and mask at the colour camera's 120 x 160, the depth image at the depth
    camera's 96 x 128 (the colour camera's rays at 0.8 of its focal length, 2 mm beside it): each depth pixel holds the scene's depth along its own ray"""
    depth_c, colour, occ, mask, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=frame, rows=120, cols=160, occluder=occluder)
    v = np.clip(np.rint((np.arange(96) + 0.5) / 0.8 - 0.5).astype(int), 0, 119)
    u = np.clip(np.rint((np.arange(128) + 0.5) / 0.8 - 0.5).astype(int), 0, 159)
    D = np.ascontiguousarray(depth_c[v][:, u])
    p = AR.params(96, 128, (0.8 * cam["fx"], 0.8 * cam["fy"]), (0.8 * (cam["cx"] + 0.5) - 0.5, 0.8 * (cam["cy"] + 0.5) - 0.5), 120, 160, (cam["fx"], cam["fy"]),
                  (cam["cx"], cam["cy"]), AR.transform(AR.rot("z", 0.1), (0.002, 0.0, 0.0)))
    return D, colour, occ, mask, p, Y0


def _frame(B, torch, D, colour, occ, mask, kind, colour_frame):
    """the aligning frame view: device (float32 metres depth, RGBA colour) or host (uint16 depth pitched, BGR)"""
    if kind == "device":
        d = B.image_view(torch.from_numpy((D / 1000.0).astype(np.float32)).cuda())
        rgba = np.concatenate([colour, np.full(colour.shape[:2] + (1,), 0xA5, np.uint8)], axis=2)
        c = B.image_view(torch.from_numpy(rgba).cuda()) if colour_frame else None
        o = B.image_view(torch.from_numpy(occ).cuda()) if colour_frame and occ is not None else None
        m = None if colour_frame else B.image_view(torch.from_numpy(mask).cuda())
    else:
        wide = np.full((D.shape[0], D.shape[1] + 3), 777, np.uint16); wide[:, :D.shape[1]] = D
        d = B.image_view(wide[:, :D.shape[1]])
        c = B.image_view(colour) if colour_frame else None
        o = B.image_view(occ) if colour_frame and occ is not None else None
        m = None if colour_frame else B.image_view(mask)
    return B.aligning_frame_view(d, c, o, m)


def _by_hand(B, cb, fv, p, rows, cols):
    """tdlo_align_depth, then the frame with a device view of the aligned plane as its depth"""
    _, counts, plane = cb.align_depth(fv.owners[0], p, out=None)
    v = B.ImageView(plane, B.IMG_U16C1, B.MEM_DEVICE, 2 * cols, None); v.rows, v.cols = rows, cols
    return B.frame_view(v, fv.owners[1], fv.owners[2], fv.owners[3]), counts


@pytest.mark.parametrize("kind", ["device", "host"])
def test_clouds_against_the_composition_by_hand(B, torch, synth, kind):
    ca, cb = B.Context(device=0, timing=False), B.Context(device=0, timing=False)
    try:
        cp = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
        D, colour, occ, mask, pd, _ = _two_streams(synth, 45, 1, occluder=(40, 100, 60, 72))
        p = B.make_align_params(**pd)
        A, n = AR.align(D if kind == "host" else (D / 1000.0).astype(np.float32), pd)
        for colour_frame in (False, True):
            fv = _frame(B, torch, D, colour, occ, mask, kind, colour_frame)
            Xa, na, nrawa, counts = ca.frame_to_cloud_view_aligning(0, fv, p, cp if colour_frame else None, 0.008)
            fv2, counts2 = _by_hand(B, cb, fv, p, 120, 160)
            Xb, nb, nrawb = cb.frame_to_cloud_view(0, fv2, cp if colour_frame else None, pd["fx_c"], pd["fy_c"], pd["cx_c"], pd["cy_c"], 0.008)
            assert counts == counts2 == n and (na, nrawa) == (nb, nrawb) and na > 100 and np.array_equal(_bits(Xa), _bits(Xb))
            assert np.array_equal(ca.debug_read_images(120, 160, depth=True)["depth"], A)
        assert ca.align_route_counts() == [2, 0] == cb.align_route_counts()
    finally:
        ca.close(); cb.close()


@pytest.mark.parametrize("kind,colour_frame", [("device", True), ("host", False)], ids=["device-colour-occluder", "host-mask"])
def test_tracker_frames_against_the_composition_by_hand(B, torch, synth, kind, colour_frame):
    P = synth.LAUNCH_PARAMS
    M = 45
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    cp = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    ca, cb = B.Context(device=0, timing=False), B.Context(device=0, timing=False)
    try:
        ta, tb = B.trackdlo(*args, ctx=ca), B.trackdlo(*args, ctx=cb)
        for f in range(10):
            D, colour, occ, mask, pd, Y0 = _two_streams(synth, M, f, occluder=(40, 100, 60, 72) if colour_frame else None)
            p = B.make_align_params(**pd)
            if f == 0:
                for t in (ta, tb):
                    t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
            fv = _frame(B, torch, D, colour, occ, mask, kind, colour_frame)
            got = ta.frame_view_aligning(fv, p, cp if colour_frame else None, 0.008, 0.06)
            fv2, counts2 = _by_hand(B, cb, fv, p, 120, 160)
            want = tb.frame_view(fv2, cp if colour_frame else None, pd["fx_c"], pd["fy_c"], pd["cx_c"], pd["cy_c"], 0.008, 0.06)
            assert list(want[0]) == list(got[0]) and list(want[1]) == list(got[1]) and want[2:] == got[2:4] and got[4] == counts2 and got[2] > 100, f
            assert np.array_equal(_bits(ta.get_tracking_result()), _bits(tb.get_tracking_result())), f
            assert np.float64(ta.get_sigma2()).view(np.uint64) == np.float64(tb.get_sigma2()).view(np.uint64), f
            assert [s["iters"] for s in ta.last_stats] == [s["iters"] for s in tb.last_stats]
            if colour_frame:
                ia, cora = ta.render_result()
                ib, corb = tb.render_result()
                assert np.array_equal(ia, ib) and cora == corb, f
                assert np.count_nonzero(np.any(ib != colour, axis=2)) > 300          # (a picture was drawn over this frame's canonical colour plane)
        assert ca.align_route_counts() == [10, 0] == cb.align_route_counts()
    finally:
        ca.close(); cb.close()


def test_refusals_touch_nothing(B, torch, synth):
    P = synth.LAUNCH_PARAMS
    M = 45
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    cp = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    D, colour, occ, mask, pd, Y0 = _two_streams(synth, M, 0, occluder=(40, 100, 60, 72))
    p = B.make_align_params(**pd)
    c, c2 = B.Context(device=0, timing=False), B.Context(device=0, timing=False)
    try:
        t = B.trackdlo(*args, ctx=c)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
        t.frame_view_aligning(_frame(B, torch, D, colour, occ, mask, "device", True), p, cp, 0.008, 0.06)
        twin = B.trackdlo(*args, ctx=c2)                                              # the tracker's whole state as it stands before the refusals
        twin.copy_state_from(t)
        cloud, nodes, sigma2 = c.get_cloud(0), t.get_tracking_result(), t.get_sigma2()
        image, _ = t.render_result()
        canon = c.debug_read_images(120, 160, depth=True, colour=True)
        counters = [int(c.lib.tdlo_debug_route_count(c.h, k)) for k in range(61)]

        def good():
            return _frame(B, torch, D, colour, occ, mask, "host", True)

        def misaligned():
            fv = good(); fv.depth.data += 1; return fv, p

        def wrong_format():
            fv = good(); fv.depth.format = B.IMG_U8C1; return fv, p

        def colour_of_the_depth_size():
            fv = good(); fv.colour.row_stride = 3 * 160 - 3; return fv, p

        def both():
            fv = _frame(B, torch, D, colour, occ, mask, "host", False); fv.colour = B.image_view(colour); return fv, p

        def neither():
            return B.aligning_frame_view(B.image_view(D)), p

        def device_says_host_pointer():
            fv = good(); fv.colour.location = B.MEM_DEVICE; return fv, p

        def params(**bad):
            return lambda: (good(), B.make_align_params(**dict(pd, **bad)))

        cases = [misaligned, wrong_format, colour_of_the_depth_size, both, neither, device_says_host_pointer, params(fx_d=0.0), params(fy_c=np.nan),
                 params(max_footprint=65), params(rows_c=0), params(T=np.full((3, 4), np.inf)), params(cols_d=0)]
        for make in cases:
            for call in (lambda fv, q: c.frame_to_cloud_view_aligning(0, fv, q, cp, 0.008), lambda fv, q: t.frame_view_aligning(fv, q, cp, 0.008, 0.06)):
                with pytest.raises(B.TdloError) as e:
                    call(*make())
                assert e.value.code == B.TDLO_E_INVALID, make
                assert np.array_equal(_bits(c.get_cloud(0)), _bits(cloud)), make
                assert np.array_equal(_bits(t.get_tracking_result()), _bits(nodes)) and t.get_sigma2() == sigma2, make
                assert [int(c.lib.tdlo_debug_route_count(c.h, k)) for k in range(61)] == counters, make
        with pytest.raises(B.TdloError):
            c.frame_to_cloud_view_aligning(0, good(), p, cp, -1.0)                    # a bad leaf
        with pytest.raises(B.TdloError):
            c.frame_to_cloud_view_aligning(99, good(), p, cp, 0.008)                  # a bad slot
        for bad in (dict(fx_c=-1.0), dict(max_footprint=-3)):
            with pytest.raises(B.TdloError):
                c.align_depth(D, B.make_align_params(**dict(pd, **bad)))
        with pytest.raises(B.TdloError):
            c.align_depth(B.image_view(np.zeros((96, 128), np.uint8)), p)
        c3 = B.Context(device=0, timing=False)
        try:
            fresh = B.trackdlo(*args, ctx=c3)                                         # a tracker without nodes
            with pytest.raises(B.TdloError):
                fresh.frame_view_aligning(good(), p, cp, 0.008, 0.06)
            assert c3.align_route_counts() == [0, 0]
        finally:
            c3.close()
        assert [int(c.lib.tdlo_debug_route_count(c.h, k)) for k in range(61)] == counters
        got = c.debug_read_images(120, 160, depth=True, colour=True)
        assert np.array_equal(got["depth"], canon["depth"]) and np.array_equal(got["colour"], canon["colour"])
        assert np.array_equal(t.render_result()[0], image)                            # ... and the last colour frame is still the one to draw over
        assert np.array_equal(_bits(t.get_tracking_result()), _bits(nodes))
        # the context serves the next frame, and the tracker steps as its untouched twin does
        D1, colour1, occ1, mask1, pd1, _ = _two_streams(synth, M, 1, occluder=(40, 100, 60, 72))
        got = t.frame_view_aligning(_frame(B, torch, D1, colour1, occ1, mask1, "device", True), p, cp, 0.008, 0.06)
        want = twin.frame_view_aligning(_frame(B, torch, D1, colour1, occ1, mask1, "device", True), p, cp, 0.008, 0.06)
        assert list(got[0]) == list(want[0]) and list(got[1]) == list(want[1]) and got[2:] == want[2:]
        assert np.array_equal(_bits(t.get_tracking_result()), _bits(twin.get_tracking_result())) and t.get_sigma2() == twin.get_sigma2()
    finally:
        c.close(); c2.close()
