"""GPU suite for one cloud from several cameras (tdlo_rig_to_cloud, tdlo_rig_to_cloud_visibility, tdlo_tracker_frame_from_rig: k_cloud_team's rig
instantiations, csrc/tdlo_cloud.hip + csrc/tdlo_rig_point.h).  Every case asserts cloud, n and n_raw bit for bit against tests/rig_ref.py (whose power on the
scenes of tests/rig_scenes.py is established in tests/test_rig_ref.py) and the route it took through tdlo_debug_route_count 45 / 46 / 47
(Context.rig_route_counts)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import colour_ref
import prepass_ref
import rig_ref as R
import rig_scenes as S
import voxel_ref as V
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    return binding


def _make(**kw):
    from trackdlo_amd import binding as B
    return B.Context(device=0, timing=False, **dict(dict(max_frames=2, max_points=1 << 15, max_nodes=64), **kw))


@pytest.fixture(scope="module")
def ctx():
    c = _make()
    yield c
    c.close()


@pytest.fixture(scope="module")
def other():
    """A second context: the single calls and the view call the consequences are held against."""
    c = _make()
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what=None):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).any(axis=1).sum()), "rows differ")


def _check(got, want, what=None):
    """(X, n, n_raw) of rig_to_cloud against (X, n_raw) of rig_ref."""
    X, n, n_raw = got
    assert n == want[0].shape[0] and n_raw == want[1], (what, n, n_raw, want[0].shape, want[1])
    _same_bits(X, want[0], what)


class _Counted:
    """with _Counted(ctx, [taken, passed, rides], what): the route counters 45 / 46 / 47 move by exactly that."""

    def __init__(self, ctx, delta, what=None):
        self.ctx, self.delta, self.what = ctx, list(delta), what

    def __enter__(self):
        self.before = self.ctx.rig_route_counts()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            after = self.ctx.rig_route_counts()
            assert [a - b for a, b in zip(after, self.before)] == self.delta, (self.what, self.before, after, self.delta)
        return False


def _delta(route, calls=1):
    return {"taken": [calls, 0, 0], "passed": [0, calls, 0]}[route]


def _dev(torch):
    """place() of rig_scenes.binding_cams: the plane as a packed device tensor (uint16 planes as int16 bits: the element size is what counts)."""
    return lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _run(B, ctx, scene, what, slot=0, place=None, route=None):
    cams, leaf = scene
    want = R.rig_ref(cams, leaf)
    with _Counted(ctx, _delta(route or S.route(cams, leaf)), what):
        _check(ctx.rig_to_cloud(slot, S.binding_cams(B, cams, place), leaf), want, what)
    return want


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("rows,cols", [(64, 64), (65, 64), (1, 1), (3, 5)])
def test_sizes(B, ctx, rows, cols, K):
    """One tile exactly, a second tile with a tail, one pixel, an image shorter than a word's worth of lanes -- for one, two and three cameras."""
    want = _run(B, ctx, S.sized(rows, cols, K), (rows, cols, K))
    assert want[1] > 0


# ---- 2. the two consequences ----------------------------------------------------------------------------------------------------------------------------
def test_one_camera_without_a_transform_is_the_single_call(B, ctx, other):
    """(a): K = 1, cam_to_rig == NULL against tdlo_depth_to_cloud on a second context -- an ordinary frame, and the pass-through frame with a zero-depth
    masked pixel left of cx whose -0.0f must come through."""
    for scene, what in ((S.sized(65, 64, 1), "frame"), (S.minus_zero(), "-0.0f, pass-through")):
        (cam, ), leaf = scene
        want = _run(B, ctx, scene, what)
        Xs, ns, nraws = other.depth_to_cloud(0, cam.depth, cam.mask, *cam.cam, leaf)
        _check((Xs, ns, nraws), want, (what, "single call"))
        _same_bits(ctx.get_cloud(0), Xs, what)
    X = ctx.get_cloud(0)
    assert ((_bits(X)[:, 0] == 1 << 63) & (_bits(X)[:, 1] == 1 << 63)).sum() == 1


def test_one_colour_camera_without_a_transform_is_the_single_colour_call(B, ctx, other):
    for scene, what in ((S.colour_rig(), "frame"), (S.minus_zero(True), "-0.0f, pass-through")):
        cams, leaf = scene
        cam = cams[0]
        want = R.rig_ref([cam], leaf)
        with _Counted(ctx, _delta(S.route([cam], leaf)), what):
            _check(ctx.rig_to_cloud(0, S.binding_cams(B, [cam]), leaf), want, what)
        p = B.make_colour_params(cam.ranges[0], cam.ranges[1], rgb_order=cam.ranges[2])
        Xs, ns, nraws = other.colour_depth_to_cloud(0, cam.depth, cam.colour, p, cam.occluder, *cam.cam, leaf)
        _check((Xs, ns, nraws), want, (what, "single call"))


@pytest.mark.parametrize("name,args", [("irrational", ()), ("fused_boundary", ()), ("shared_cells", ()), ("sized", (65, 64, 3)), ("overflow", ()), ("colour_rig", ())])
def test_the_view_call_on_the_host_point_list_leaves_the_same_cloud(B, ctx, other, name, args):
    """(b): tdlo_cloud_view_voxel_grid on rig_points_host's float32 array, on a second context."""
    cams, leaf = getattr(S, name)(*args)
    want = _run(B, ctx, (cams, leaf), name)
    Rh = ctx.rig_points_host(S.binding_cams(B, cams))
    assert Rh.dtype == np.float32 and np.array_equal(Rh.view(np.uint32), R.points(cams).view(np.uint32))
    _check(other.voxel_grid_view(0, Rh, leaf), want, (name, "view call"))
    _same_bits(ctx.get_cloud(0), other.get_cloud(0), name)


# ---- 3. empty cameras, shared cells, transforms, dropped points -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [0, 1, 2, "all"])
def test_empty_cameras(B, ctx, where):
    """A camera with no kept pixel first, in the middle, last; none at all: n = 0, no error, an empty slot."""
    ctx.set_cloud(0, np.random.default_rng(3).standard_normal((200, 3)))
    want = _run(B, ctx, S.empties(where), where)
    if where == "all":
        assert want[1] == 0 and ctx.get_cloud(0).shape == (0, 3)


def test_two_cameras_that_share_cells_in_both_orders(B, ctx):
    cams, leaf = S.shared_cells()
    wab = _run(B, ctx, (cams, leaf), "a, b", slot=0)
    wba = _run(B, ctx, (cams[::-1], leaf), "b, a", slot=1)
    Xab, Xba = ctx.get_cloud(0), ctx.get_cloud(1)
    _same_bits(Xab, wab[0]); _same_bits(Xba, wba[0])
    assert Xab.shape == Xba.shape and (_bits(Xab) != _bits(Xba)).any(axis=1).sum() >= 10


@pytest.mark.parametrize("kind", list(S.TRANSFORMS))
def test_transforms(B, ctx, kind):
    """The identity given as a matrix, a pure translation, the rotation by 0.3 rad about an oblique axis, an anisotropic scale."""
    _run(B, ctx, S.transform(kind), kind)


def test_no_fused_multiply_add_in_the_transform(B, ctx, torch):
    """The scene whose sums lie at float rounding boundaries (tests/test_rig_ref.py: a fused transform gives another R and another cloud there): the one
    launch leaves the statement's bits, from host and from device planes, and they are not the fused reading's.  The multi-launch form runs the scene in
    the child process below."""
    cams, leaf = S.fused_boundary()
    want = _run(B, ctx, (cams, leaf), "host planes")
    _run(B, ctx, (cams, leaf), "device planes", place=_dev(torch))
    for form in (0, 1):
        Xf, _ = V.voxel_ref(R.points_fused(cams, form), None, leaf)
        assert Xf.shape != want[0].shape or (_bits(Xf) != _bits(want[0])).any(), form


def test_points_that_overflow_float_are_dropped(B, ctx):
    cams, leaf = S.overflow()
    want = _run(B, ctx, (cams, leaf), "overflow")
    assert want[1] == int((cams[0].mask != 0).sum()) + cams[1].depth.shape[0] < sum(int((c.mask != 0).sum()) for c in cams)


# ---- 4. the borders of the one launch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32704, 32705])
def test_the_point_border(B, ctx, n):
    """32 704 kept pixels over two 128 x 128 cameras are served; 32 705 are passed on (counter 46): the same bits."""
    scene = S.border(n)
    want = _run(B, ctx, scene, n, route="taken" if n == 32704 else "passed")
    assert want[1] == n


@pytest.mark.parametrize("K,cols,route", [(63, 262145, "taken"), (64, 262144, "passed")])
def test_the_tile_border(B, ctx, torch, K, cols, route):
    """63 cameras of 1 x 262 145 pixels are 4 095 tiles and are served; 64 cameras of 1 x 262 144 are 4 096 tiles and take the multi-launch form.  Masks almost
    empty, one depth plane for all cameras; planes in device memory."""
    scene = S.many_tiles(K, cols)
    assert S.tiles(scene[0]) == (S.kFTmax if route == "taken" else S.kFTmax + 1)
    depth = _dev(torch)(scene[0][0].depth)
    want = _run(B, ctx, scene, (K, cols), place=lambda a: depth if a.dtype == np.uint16 else _dev(torch)(a), route=route)
    assert want[1] == 3 * K


# ---- 5. where the planes lie -----------------------------------------------------------------------------------------------------------------------------------
def test_planes_in_device_memory_and_mixed(B, ctx, torch):
    cams, leaf = S.irrational()
    dev = _dev(torch)
    _run(B, ctx, (cams, leaf), "device", place=dev)
    flip = [0]

    def mixed(a):
        flip[0] += 1
        return dev(a) if flip[0] % 2 else a
    _run(B, ctx, (cams, leaf), "mixed", place=mixed)
    ccams, cleaf = S.colour_rig()
    _run(B, ctx, (ccams, cleaf), "colour, device", place=dev)
    flip[0] = 1
    _run(B, ctx, (ccams, cleaf), "colour, mixed", place=mixed)


# ---- 6. colour rigs ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_colour_rig_with_its_own_ranges_and_an_occluder(B, ctx):
    cams, leaf = S.colour_rig()
    # the statement of the segmentation is tests/colour_ref.py
    for c in cams:
        assert np.array_equal(c.kept(), colour_ref.colour_mask(c.colour, c.ranges[0], c.ranges[1], c.ranges[2], c.occluder) != 0)
    want = _run(B, ctx, (cams, leaf), "colour rig")
    assert want[1] == sum(int(c.kept().sum()) for c in cams)
    _run(B, ctx, (cams[::-1], leaf), "colour rig, reversed")


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import rig_ref as R, rig_scenes as S
from trackdlo_amd import binding as B
ctx = B.Context(device=0, timing=False, max_frames=1, max_points=1 << 15, max_nodes=64)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
for name, scene in (("colour", S.colour_rig()), ("irrational", S.irrational()), ("fused boundary", S.fused_boundary()), ("empty", S.empties("all")), ("tail", S.sized(65, 64, 3)), ("border", S.border(32705))):
    cams, leaf = scene
    want = R.rig_ref(cams, leaf)
    X, n, nraw = ctx.rig_to_cloud(0, S.binding_cams(B, cams), leaf)
    assert n == want[0].shape[0] and nraw == want[1] and X.shape == want[0].shape and np.array_equal(bits(X), bits(want[0])), (name, n, nraw)
assert ctx.rig_route_counts() == [0, 6, 0], ctx.rig_route_counts()
ctx.close()
print("child ok")
"""


def test_the_multi_launch_form_forced_in_a_child_process():
    """TDLO_CLOUD_FUSED=0 (read when the context is made): every rig takes the multi-launch form over the RigSrc -- a colour rig's masks by k_colour_mask per
    camera into the arena first -- and leaves the same bits."""
    env = dict(os.environ, TDLO_CLOUD_FUSED="0")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


# ---- 7. the ride -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [45, 65])
def test_the_visibility_pre_pass_rides_in_the_launch(B, ctx, other, M):
    """tdlo_rig_to_cloud_visibility against the two calls on a second context and against tests/prepass_ref.py: cloud, node distances and both index sets bit
    for bit; with 45 nodes the pre-pass rode (counter 47), with 65 it ran behind the launch."""
    cams, leaf = S.irrational()
    want = R.rig_ref(cams, leaf)
    X = want[0]
    rng = np.random.default_rng(M)
    Y = np.ascontiguousarray(X[rng.choice(len(X), M, replace=False)] + (np.arange(M)[:, None] % 3 == 2) * 0.03)      # (a third of the nodes beyond the threshold)
    coord = np.arange(M) * 0.01
    thr, d_vis = 0.008, 0.06
    bc = S.binding_cams(B, cams)
    with _Counted(ctx, [1, 0, 1 if M <= 64 else 0], M):
        dist, vis, ext, n, nraw = ctx.rig_to_cloud_visibility(0, bc, leaf, Y, thr, d_vis, coord)
    Xb, nb, nrawb = other.rig_to_cloud(0, bc, leaf)
    db, vb, eb = other.visibility_prepass(0, Y, thr, d_vis, coord)
    assert (n, nraw) == (nb, nrawb) == (X.shape[0], want[1])
    _same_bits(ctx.get_cloud(0), X, M); _same_bits(Xb, X, M)
    assert np.array_equal(dist.view(np.uint64), db.view(np.uint64)) and np.array_equal(vis, vb) and np.array_equal(ext, eb)
    rd, rv, re = prepass_ref.prepass(X, Y, thr, d_vis, coord)
    assert np.array_equal(dist.view(np.uint64), np.asarray(rd).view(np.uint64)) and np.array_equal(vis, rv) and np.array_equal(ext, re)
    assert 0 < len(vis) < M
    # a rig that keeps nothing: no cloud, nothing visible, no error -- and the next ride finds the minima armed
    with _Counted(ctx, [1, 0, 0], (M, "nothing kept")):
        dist, vis, ext, n, nraw = ctx.rig_to_cloud_visibility(0, S.binding_cams(B, S.empties("all")[0]), leaf, Y, thr, d_vis, coord)
    assert (n, nraw, len(vis), len(ext)) == (0, 0, 0, 0)
    with _Counted(ctx, [1, 0, 1 if M <= 64 else 0], (M, "again")):
        d2, v2, e2, n, nraw = ctx.rig_to_cloud_visibility(0, bc, leaf, Y, thr, d_vis, coord)
    assert np.array_equal(d2.view(np.uint64), np.asarray(rd).view(np.uint64)) and np.array_equal(v2, rv) and np.array_equal(e2, re)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_resident_cloud_and_the_counters(B, ctx, torch):
    cams, leaf = S.irrational()
    a, b = cams
    d, m = a.depth, a.mask
    img = S.paint(m, 3)
    blue = (*colour_ref.LAUNCH_RANGE, 0)
    Xres = np.random.default_rng(9).standard_normal((300, 3))
    ctx.set_cloud(0, Xres)
    big = np.zeros((4096, 4096), np.uint16), np.zeros((4096, 4096), np.uint8)
    bad = {
        "no cameras": [],
        "65 cameras": [a] * 65,
        "too many pixels": [R.Cam(big[0], big[1], cam=S.CAM)] * 5,
        "neither mask nor colour": [a, R.Cam(d, cam=S.CAM)],
        "mixed kinds": [a, R.Cam(d, colour=img, ranges=blue, cam=S.CAM)],
        "fx = 0": [a.replaced(cam=(0.0, 600.0, 1.0, 1.0))],
        "fy = 0": [a, b.replaced(cam=(600.0, 0.0, 1.0, 1.0))],
        "nan in cam_to_rig": [a, b.replaced(T=np.where(np.arange(12).reshape(3, 4) == 7, np.nan, b.T))],
        "inf in cam_to_rig": [a.replaced(T=np.where(np.arange(12).reshape(3, 4) == 0, np.inf, b.T))],
    }
    E = B.TDLO_E_INVALID

    def refused(bc, leaf_size=leaf, slot=0, what=None):
        with pytest.raises((B.TdloError, ValueError)) as e:
            ctx.rig_to_cloud(slot, bc, leaf_size)
        assert isinstance(e.value, ValueError) or e.value.code == E, what
    with _Counted(ctx, [0, 0, 0], "refusals"):
        for what, cs in bad.items():
            refused(S.binding_cams(B, cs), what=what)
        # a camera without depth; colour without ranges, bad ranges (the table by hand: the binding would not build these)
        tab, K, rows, cols, keep = B._rig_cameras(S.binding_cams(B, [a, b]))
        n = B.C.c_int(0); nraw = B.C.c_int(0)
        tab[1].depth = None
        assert ctx.lib.tdlo_rig_to_cloud(ctx.h, 0, B.C.cast(tab, B.C.c_void_p), K, rows, cols, leaf, None, 0, B.C.byref(n), B.C.byref(nraw)) == E
        cc = S.binding_cams(B, [R.Cam(d, colour=img, ranges=blue, cam=S.CAM)])
        cc[0].params = None
        refused(cc, what="colour without ranges")
        p = B.make_colour_params(); p.n_ranges = 0
        cc[0].params = p
        refused(cc, what="bad ranges")
        good = S.binding_cams(B, [a, b])
        for lf in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
            refused(good, leaf_size=lf, what=("leaf", lf))
        refused(good, slot=-1, what="slot"); refused(good, slot=2, what="slot")
        # K = 0 at the ABI
        assert ctx.lib.tdlo_rig_to_cloud(ctx.h, 0, B.C.cast(tab, B.C.c_void_p), 0, rows, cols, leaf, None, 0, B.C.byref(n), B.C.byref(nraw)) == E
    _same_bits(ctx.get_cloud(0), Xres, "the resident cloud")
    # V's own refusal (a cloud 1e9 leaf sizes from the origin) comes from the multi-launch form, the kernel having passed the rig on: the cloud intact as well
    far = [a.replaced(T=S.TRANSFORMS["translation"] + np.array([[0, 0, 0, 1.0e9], [0, 0, 0, 0], [0, 0, 0, 0]]))]
    with pytest.raises(V.TooFar):
        R.rig_ref(far, leaf)
    with _Counted(ctx, [0, 1, 0], "too far"):
        with pytest.raises(B.TdloError) as e:
            ctx.rig_to_cloud(0, S.binding_cams(B, far), leaf)
    assert e.value.code == E and "too far" in str(e.value)
    _same_bits(ctx.get_cloud(0), Xres, "the resident cloud")


def test_a_tracker_with_the_self_occlusion_switch_is_refused(B):
    from trackdlo_amd import synth
    ctx = _make(max_frames=1)
    M = 20
    Pm = synth.LAUNCH_PARAMS
    args = (M, Pm["visibility_threshold"], Pm["beta"], Pm["lambda_"], Pm["alpha"], Pm["k_vis"], Pm["mu"], 30, Pm["tol"], Pm["beta_pre_proc"], Pm["lambda_pre_proc"], Pm["lle_weight"])
    t = B.trackdlo(*args, ctx=ctx, precision=0)
    try:
        Y0 = synth.nodes(M)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
        proj = np.zeros((3, 4)); proj[0, 0] = proj[1, 1] = 600.0; proj[0, 2] = 320.0; proj[1, 2] = 240.0; proj[2, 2] = 1.0
        t.set_self_occlusion(proj, 10)
        cams, leaf = S.irrational()
        with pytest.raises(B.TdloError) as e:
            t.frame_from_rig(S.binding_cams(B, cams), leaf, 0.06)
        assert e.value.code == B.TDLO_E_INVALID and ctx.rig_route_counts() == [0, 0, 0]
        _same_bits(t.get_tracking_result(), Y0)
    finally:
        del t
        ctx.close()


# ---- 9. one context through single calls, a rig, another image size ---------------------------------------------------------------------------------------------------
def test_one_context_through_single_calls_a_rig_and_another_image_size(B):
    """The state words, the team's sort buffers and `cloud_fused_first` are one set for every kind of call, and the batch arena is the rig's plane store."""
    ctx = _make()
    try:
        (one, ), leaf1 = S.sized(65, 64, 1)
        rig, leaf = S.irrational()
        big, leafb = S.border(32704)
        small, leafs = S.sized(3, 5, 3)
        w1 = V.voxel_ref(V.backproject(one.depth, one.mask, *one.cam), None, leaf1)
        for rep in range(2):
            _check(ctx.depth_to_cloud(0, one.depth, one.mask, *one.cam, leaf1), w1, ("single", rep))
            _check(ctx.rig_to_cloud(0, S.binding_cams(B, rig), leaf), R.rig_ref(rig, leaf), ("rig", rep))
            _check(ctx.voxel_grid_view(1, R.points(rig), leaf), R.rig_ref(rig, leaf), ("view", rep))
            _check(ctx.rig_to_cloud(1, S.binding_cams(B, big), leafb), R.rig_ref(big, leafb), ("rig, larger images", rep))
            _check(ctx.rig_to_cloud(0, S.binding_cams(B, small), leafs), R.rig_ref(small, leafs), ("rig, smaller images", rep))
            _check(ctx.depth_to_cloud(1, one.depth, one.mask, *one.cam, leaf1), w1, ("single again", rep))
        assert ctx.rig_route_counts() == [6, 0, 0] and ctx.cloud_route_counts() == [4, 0] and ctx.view_route_counts() == [2, 0, 0]
    finally:
        ctx.close()


# ---- 10. the tracker ------------------------------------------------------------------------------------------------------------------------------------------------
POSE = S.about(S.rotation(0.35, (0.1, 1.0, 0.05)), (0.0, 0.0, 0.6), (0.02, -0.01, 0.015))     # camera 1 -> rig (= camera 0's frame): [A | b]


def _second_pose(M, config, frame, T):
    """synth.depth_scene's rope seen by a second camera whose frame is taken to the first's by T = [A | b]: the same tube of surface points, brought into the
    second camera's frame (A^T (p - b): A is a rotation), projected with the same intrinsics, z-buffered, depth in millimetres."""
    from trackdlo_amd import synth
    cam = dict(synth.CAMERA)
    rng = np.random.default_rng(synth.BASE_SEED + 1000 * config + frame + 77)
    samples, radius = 400000, 0.006
    s = rng.random(samples)
    c = synth.centreline(s, M) + np.asarray((0.0, 0.005, 0.0))[None, :]
    ang = rng.random(samples) * 2 * np.pi
    rad = radius * np.sqrt(rng.random(samples))
    p = c + np.stack([np.zeros(samples), rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    p = (p - T[:, 3]) @ T[:, :3]                                   # A^T (p - b), row vectors
    u = np.rint(p[:, 0] * cam["fx"] / p[:, 2] + cam["cx"]).astype(np.int64)
    v = np.rint(p[:, 1] * cam["fy"] / p[:, 2] + cam["cy"]).astype(np.int64)
    ok = (u >= 0) & (u < cam["cols"]) & (v >= 0) & (v < cam["rows"]) & (p[:, 2] > 0.1)
    u, v, z = u[ok], v[ok], p[ok, 2]
    zmm = np.clip(np.rint(z * 1000.0), 1, 65535).astype(np.int64)
    depth = np.full(cam["rows"] * cam["cols"], 65535, dtype=np.int64)
    np.minimum.at(depth, v * cam["cols"] + u, zmm)
    mask = (depth != 65535).astype(np.uint8) * 255
    depth[depth == 65535] = 1500
    return depth.astype(np.uint16).reshape(cam["rows"], cam["cols"]), mask.reshape(cam["rows"], cam["cols"])


def test_ten_frames_of_a_two_camera_scene_against_the_calls_by_hand(B):
    """frame_from_rig over 10 frames against a twin tracker fed visibility_prepass + tracking_step by hand on the rig's cloud, bit for bit; and a node hidden
    from camera 0 by an occluder but seen by camera 1 is in the visible set (it is not when camera 0 is alone)."""
    from trackdlo_amd import synth
    from test_cloud_view_gpu import _same_tracker_state
    M, leaf, d_vis = 30, 0.008, 0.06
    Pm = synth.LAUNCH_PARAMS
    thr = Pm["visibility_threshold"]
    args = (M, thr, Pm["beta"], Pm["lambda_"], Pm["alpha"], Pm["k_vis"], Pm["mu"], 30, Pm["tol"], Pm["beta_pre_proc"], Pm["lambda_pre_proc"], Pm["lle_weight"])
    ca, cb = _make(max_frames=1), _make(max_frames=1)
    ta, tb = B.trackdlo(*args, ctx=ca, precision=0), B.trackdlo(*args, ctx=cb, precision=0)
    try:
        _, _, cam, Y0 = synth.depth_scene(M, config=9, frame=0)
        coord = synth.geodesic_coord(Y0)
        for t in (ta, tb):
            t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        intr = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        # the occluder in front of camera 0: the image columns of the nodes 12 .. 17
        u = np.rint(Y0[:, 0] * cam["fx"] / Y0[:, 2] + cam["cx"]).astype(int)
        lo, hi = sorted((int(u[12]), int(u[17])))
        hidden_somewhere = False
        for fr in range(10):
            d0, m0, _, _ = synth.depth_scene(M, config=9, frame=fr)
            m0 = m0.copy(); m0[:, lo - 6:hi + 7] = 0
            d1, m1 = _second_pose(M, 9, fr, POSE)
            cams = [R.Cam(d0, m0, cam=intr), R.Cam(d1, m1, cam=intr, T=POSE)]
            bc = S.binding_cams(B, cams)
            want = R.rig_ref(cams, leaf)
            Yb = tb.get_tracking_result()
            va, vea, na, nrawa = ta.frame_from_rig(bc, leaf, d_vis)
            Xb, nb, nrawb = cb.rig_to_cloud(0, bc, leaf)
            _, vb, veb = cb.visibility_prepass(0, Yb, thr, d_vis, coord)
            tb.tracking_step(None, vb, veb)
            assert (na, nrawa) == (nb, nrawb) == (want[0].shape[0], want[1]) and 0 < na < nrawa
            _same_bits(ca.get_cloud(0), want[0], fr); _same_bits(Xb, want[0], fr)
            assert np.array_equal(va, vb) and np.array_equal(vea, veb) and len(va) > 0
            _same_tracker_state(ta, tb)
            # camera 0 alone does not see the nodes behind the occluder; the rig does
            X0, _, _ = cb.rig_to_cloud(0, bc[:1], leaf)
            _, v0, _ = cb.visibility_prepass(0, Yb, thr, d_vis, coord)
            behind = [k for k in range(13, 17) if k not in v0]
            hidden_somewhere = hidden_somewhere or bool(behind)
            assert all(k in va for k in behind), (fr, behind, va)
        assert hidden_somewhere
        assert ca.rig_route_counts() == [10, 0, 10] and cb.rig_route_counts() == [20, 0, 0]
        # a rig that keeps nothing: TDLO_E_EMPTY, the nodes as they were
        before = ta.get_tracking_result().copy()
        with pytest.raises(B.TdloError) as e:
            ta.frame_from_rig(S.binding_cams(B, [c.replaced(mask=np.zeros_like(c.mask)) for c in cams]), leaf, d_vis)
        assert e.value.code == -4                                 # TDLO_E_EMPTY
        _same_bits(ta.get_tracking_result(), before)
        _same_tracker_state(ta, tb)
    finally:
        del ta, tb
        ca.close(); cb.close()
