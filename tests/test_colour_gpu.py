"""GPU suite for the colour segmentation on the device (tdlo_colour_*; trackdlo_node.cpp:84-119, :158-180 in front of :195-369).

The device code is held to tests/colour_ref.py -- the numpy statement of OpenCV's integer BGR -> HSV routine, cv::inRange and the AND with the occluder
image -- bit for bit: over the whole colour cube, on shapes where the four-pixel word handling can go wrong, from pageable pointers and from the
context's pinned buffers.  Everything behind the segmentation is compared, as arrays, with the mask calls (tests/test_cloud_gpu.py holds those to the
oracle) fed the reference's mask: the cloud on the one-launch route and on each comparator route, the riding visibility pre-pass, four frames of a tracker.
"""
import os

import numpy as np
import pytest

import colour_ref as R

pytestmark = pytest.mark.gpu

_SWITCHES = ("TDLO_COLOUR_FUSED", "TDLO_CLOUD_FUSED", "TDLO_CLOUD_TEAM")


def _ctx(B, **env):
    """A context made under the given switches (they are read when a context is made); the environment is left as it was."""
    old = {k: os.environ.get(k) for k in _SWITCHES}
    try:
        for k in _SWITCHES:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = v
        return B.Context(device=0, max_nodes=128)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _args(cam):
    return (cam["fx"], cam["fy"], cam["cx"], cam["cy"])


_scenes = {}


def _scene(shape, M, frame, ranges="launch", occ=None):
    """(depth, colour, occluder image, the REFERENCE's mask, cam, Y0) of a colour_scene, made once."""
    key = (shape, M, frame, ranges, occ)
    if key not in _scenes:
        from trackdlo_amd import synth
        rg = R.LAUNCH_RANGE if ranges == "launch" else R.MULTI_RANGES
        depth, colour, occl, _, cam, Y0 = synth.colour_scene(M, *rg, config=9, frame=frame, rows=shape[0], cols=shape[1], occluder=occ)
        for a in (depth, colour):
            a.setflags(write=False)
        ref = R.colour_mask(colour, *rg, occluder=occl)
        ref.setflags(write=False)
        _scenes[key] = (depth, colour, occl, ref, cam, Y0)
    return _scenes[key]


@pytest.fixture(scope="module")
def cube():
    c = R.cube()
    hsv = R.bgr_to_hsv(c)
    c.setflags(write=False); hsv.setflags(write=False)
    return c, hsv


def test_whole_colour_cube(cube):
    """One 4096 x 4096 image holds every colour once: the HSV image and the masks of four parameter sets equal the reference byte for byte."""
    from trackdlo_amd import binding as B
    c, hsv = cube
    ctx = _ctx(B)
    try:
        m, h = ctx.colour_mask(c, B.make_colour_params(*R.LAUNCH_RANGE), hsv=True)
        assert np.array_equal(h, hsv)
        assert np.array_equal(m, R.in_ranges(hsv, *R.LAUNCH_RANGE))
        assert np.array_equal(ctx.colour_mask(c, B.make_colour_params(*R.MULTI_RANGES)), R.in_ranges(hsv, *R.MULTI_RANGES))
        m1, h1 = ctx.colour_mask(c, B.make_colour_params(*R.LAUNCH_RANGE, rgb_order=1), hsv=True)
        hsv1 = R.bgr_to_hsv(c, rgb_order=1)
        assert np.array_equal(h1, hsv1) and np.array_equal(m1, R.in_ranges(hsv1, *R.LAUNCH_RANGE))
        for v in ([50, 240, 200], [0, 0, 7], [179, 255, 255]):
            assert np.array_equal(ctx.colour_mask(c, B.make_colour_params([v], [v])), R.in_ranges(hsv, [v], [v]))
        # bounds are clamped to 0 .. 255; a range whose lower bound lies above its upper bound passes nothing, the others still count
        assert np.array_equal(ctx.colour_mask(c, B.make_colour_params([[-5, 90, 30], [100, 0, 0]], [[10, 300, 255], [90, 255, 255]])),
                              R.in_ranges(hsv, [[0, 90, 30]], [[10, 255, 255]]))
        for n in (0, 5):
            p = B.make_colour_params()
            p.n_ranges = n
            with pytest.raises(B.TdloError) as e:
                ctx.colour_mask(c[:4, :8], p)
            assert e.value.code == B.TDLO_E_INVALID
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [(1, 77), (97, 43), (120, 161), (480, 640)])
def test_shapes_where_the_word_handling_can_go_wrong(shape):
    """A thread takes four pixels: a last word of one to three pixels, more than one tile, one row; with and without an occluder, with one range and
    with four; from pageable pointers and from the context's pinned buffers (read in place)."""
    from trackdlo_amd import binding as B
    rows, cols = shape
    ctx = _ctx(B)
    try:
        for k, (ranges, occ) in enumerate((("launch", None), ("multi", (rows // 3, rows // 3 + max(1, rows // 4), cols // 4, cols // 2)))):
            rg = R.LAUNCH_RANGE if ranges == "launch" else R.MULTI_RANGES
            _, colour, occl, ref, _, _ = _scene(shape, 40, 3 + k, ranges, occ)
            p = B.make_colour_params(*rg)
            m, h = ctx.colour_mask(colour, p, occl, hsv=True)
            assert np.array_equal(m, ref) and np.array_equal(h, R.bgr_to_hsv(colour))
            cb, ob = ctx.colour_buffers(rows, cols)
            cb[:] = colour
            if occl is not None:
                ob[:] = occl
            assert np.array_equal(ctx.colour_mask(cb, p, ob if occl is not None else None), ref)
            # every pixel of a random image, not only the scene's two classes
            rnd = np.random.default_rng(rows * cols + k).integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
            assert np.array_equal(ctx.colour_mask(rnd, p, occl), R.colour_mask(rnd, *rg, occluder=occl))
    finally:
        ctx.close()


@pytest.mark.parametrize("env,colour_routes,cloud_routes", [
    ({}, [6, 0], [6, 0]),                                        # the segmentation rides in the one launch (k_cloud_team, colour instantiation)
    ({"TDLO_CLOUD_TEAM": "0"}, [6, 0], [6, 0]),                  # ... in k_cloud_fused's
    ({"TDLO_COLOUR_FUSED": "0"}, [0, 6], [6, 0]),                # the mask kernel, then the mask route as it is
    ({"TDLO_CLOUD_FUSED": "0"}, [0, 6], [0, 0]),                 # the mask kernel, then the multi-launch form
])
def test_colour_cloud_equals_the_mask_route_fed_the_references_mask(env, colour_routes, cloud_routes):
    from trackdlo_amd import binding as B
    a, b = _ctx(B, **env), _ctx(B)
    try:
        for shape, M, occ in (((480, 640), 30, None), ((720, 1280), 50, (300, 420, 500, 640)), ((97, 43), 30, None)):
            depth, colour, occl, ref, cam, _ = _scene(shape, M, 5, "launch", occ)
            p = B.make_colour_params(*R.LAUNCH_RANGE)
            Xb, nb, nrb = b.depth_to_cloud(0, depth, ref, *_args(cam), 0.008)
            assert nrb == np.count_nonzero(ref) and nb > 0
            for rep in range(2):                                  # (twice in a row on one context: the second time from the pinned buffers, in place)
                if rep == 0:
                    d, c, o = depth, colour, occl
                else:
                    d, _ = a.image_buffers(*shape)
                    c, o = a.colour_buffers(*shape)
                    d[:] = depth; c[:] = colour
                    if occl is None:
                        o = None
                    else:
                        o[:] = occl
                Xa, na, nra = a.colour_depth_to_cloud(0, d, c, p, o, *_args(cam), 0.008)
                assert na == nb and nra == nrb and np.array_equal(Xa, Xb)
        assert a.colour_route_counts() == colour_routes and a.cloud_route_counts() == cloud_routes
        assert b.colour_route_counts() == [0, 0]
    finally:
        a.close(); b.close()


def test_a_frame_every_pixel_of_which_passes_is_passed_on():
    """The range 0 .. 255 on every channel at 640 x 480: 307 200 masked pixels, more than the one-launch kernel takes -- the frame comes back through the
    mask kernel and the multi-launch form with the bits of the mask route, and is counted as passed on."""
    from trackdlo_amd import binding as B
    depth, colour, _, _, cam, _ = _scene((480, 640), 30, 5)
    a, b = _ctx(B), _ctx(B)
    try:
        p = B.make_colour_params([[0, 0, 0]], [[255, 255, 255]])
        Xa, na, nra = a.colour_depth_to_cloud(0, depth, colour, p, None, *_args(cam), 0.008)
        Xb, nb, nrb = b.depth_to_cloud(0, depth, np.full(depth.shape, 255, dtype=np.uint8), *_args(cam), 0.008)
        assert nra == nrb == 307200 and na == nb and np.array_equal(Xa, Xb)
        assert a.colour_route_counts() == [0, 1] and a.cloud_route_counts() == [0, 1]
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("M,rides", [(30, True), (70, False)])
def test_visibility_form_and_frame_from_colour(M, rides):
    """tdlo_colour_depth_to_cloud_visibility and tdlo_tracker_frame_from_colour against the mask calls fed the reference's mask: node distances, both index
    sets, the nodes of four consecutive frames and both registrations' iteration counts, equal as arrays.  30 nodes: the pre-pass rides in the launch; 70: it
    runs behind it."""
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    shape = (480, 640)
    a, b = _ctx(B), _ctx(B)
    try:
        depth, colour, occl, ref, cam, Y0 = _scene(shape, M, 0, "multi", (100, 380, 300, 360))
        coord = synth.geodesic_coord(Y0)
        p = B.make_colour_params(*R.MULTI_RANGES)
        da, va, ea, na, nra = a.colour_depth_to_cloud_visibility(0, depth, colour, p, occl, *_args(cam), 0.008, Y0, 0.008, 0.06, coord)
        db, vb, eb, nb, nrb = b.depth_to_cloud_visibility(0, depth, ref, *_args(cam), 0.008, Y0, 0.008, 0.06, coord)
        assert na == nb and nra == nrb and np.array_equal(da, db) and np.array_equal(va, vb) and np.array_equal(ea, eb)
        assert 0 < len(va) < M                                    # (the occluder hides a stretch of the rope)
        assert a.cloud_vis_rides() == b.cloud_vis_rides() == (1 if rides else 0)
        targs = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
        ta, tb = B.trackdlo(*targs, ctx=a), B.trackdlo(*targs, ctx=b)
        for t in (ta, tb):
            t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        dbuf, _ = a.image_buffers(*shape)
        cbuf, obuf = a.colour_buffers(*shape)
        for fr in range(4):
            occ = (100, 380, 300, 360) if fr == 2 else None
            depth, colour, occl, ref, _, _ = _scene(shape, M, fr, "multi", occ)
            dbuf[:] = depth; cbuf[:] = colour
            if occl is not None:
                obuf[:] = occl
            va, ea, na, nra = ta.frame_from_colour(dbuf, cbuf, p, obuf if occl is not None else None, *_args(cam), 0.008, 0.06)
            vb, eb, nb, nrb = tb.frame_from_depth(depth, ref, *_args(cam), 0.008, 0.06)
            assert na == nb and nra == nrb and np.array_equal(va, vb) and np.array_equal(ea, eb)
            assert np.array_equal(ta.get_tracking_result(), tb.get_tracking_result()) and ta.get_sigma2() == tb.get_sigma2()
            assert [s["iters"] for s in ta.last_stats] == [s["iters"] for s in tb.last_stats]
        assert a.colour_route_counts() == [5, 0] and a.cloud_vis_rides() == (5 if rides else 0)
    finally:
        a.close(); b.close()


def test_a_colour_frame_whose_team_gives_its_launch_up():
    """TDLO_CLOUD_TEAM_FORCE_TIMEOUT=2: the process's second team launch loses a member; that colour frame comes back through the mask kernel and the
    multi-launch form, the pre-pass behind it -- the bits of the frames before and after, which ride."""
    import subprocess, sys, textwrap
    code = textwrap.dedent('''
        import sys
        sys.path.insert(0, "tests")
        import numpy as np
        import colour_ref as R
        from trackdlo_amd import binding as B, synth
        depth, colour, occl, _, cam, Y0 = synth.colour_scene(30, *R.LAUNCH_RANGE, config=9, frame=3, occluder=(0, 480, 100, 140))
        ref = R.colour_mask(colour, *R.LAUNCH_RANGE, occluder=occl)
        coord = synth.geodesic_coord(Y0)
        args = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        a = B.Context(device=0); b = B.Context(device=0)
        p = B.make_colour_params(*R.LAUNCH_RANGE)
        out = [a.colour_depth_to_cloud_visibility(0, depth, colour, p, occl, *args, 0.008, Y0, 0.008, 0.06, coord) for rep in range(3)]
        _, n2, nraw2 = b.depth_to_cloud(0, depth, ref, *args, 0.008, fetch=False)
        d2, v2, e2 = b.visibility_prepass(0, Y0, 0.008, 0.06, coord)
        for d1, v1, e1, n1, nraw1 in out:
            assert n1 == n2 and nraw1 == nraw2 and np.array_equal(d1, d2) and np.array_equal(v1, v2) and np.array_equal(e1, e2)
        print("rides", a.cloud_vis_rides(), "cloud", a.cloud_route_counts(), "colour", a.colour_route_counts())
    ''')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TDLO_CLOUD_TEAM_FORCE_TIMEOUT="2", PYTHONPATH=root)
    for k in _SWITCHES:
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rides 2 cloud [2, 1] colour [2, 1]" in r.stdout, r.stdout


def test_an_image_none_of_whose_pixels_pass():
    """n = 0 from the cloud call, no error; TDLO_E_EMPTY from frame_from_colour with the tracker's state untouched -- frame_from_depth's behaviour."""
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    depth, colour, _, ref, cam, Y0 = _scene((480, 640), 30, 1)
    grey = np.repeat(colour[:, :, :1], 3, axis=2)                    # S = 0 everywhere: nothing passes S >= 90
    assert not R.colour_mask(grey, *R.LAUNCH_RANGE).any()
    a = _ctx(B)
    try:
        p = B.make_colour_params(*R.LAUNCH_RANGE)
        X, n, nraw = a.colour_depth_to_cloud(0, depth, grey, p, None, *_args(cam), 0.008)
        assert n == 0 and nraw == 0 and X.shape == (0, 3)
        X, n, nraw = a.colour_depth_to_cloud(0, depth, colour, p, np.zeros(depth.shape, dtype=np.uint8), *_args(cam), 0.008)      # everything occluded
        assert n == 0 and nraw == 0
        M = 30
        coord = synth.geodesic_coord(Y0)
        t = B.trackdlo(M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"],
                       P["lle_weight"], ctx=a)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        t.frame_from_colour(depth, colour, p, None, *_args(cam), 0.008, 0.06)
        Yk, sk = t.get_tracking_result().copy(), t.get_sigma2()
        with pytest.raises(B.TdloError) as e:
            t.frame_from_colour(depth, grey, p, None, *_args(cam), 0.008, 0.06)
        assert e.value.code == B.TDLO_E_EMPTY
        assert np.array_equal(t.get_tracking_result(), Yk) and t.get_sigma2() == sk
        t.frame_from_colour(depth, colour, p, None, *_args(cam), 0.008, 0.06)      # ... and the next frame is served as usual
        assert a.colour_route_counts() == [5, 0]
    finally:
        a.close()
