"""CPU suite of the rig calls (tdlo_rig_to_cloud, include/trackdlo_hip.h), no GPU:
1. tests/rig_ref.py, the numpy statement of the rig's point list R, against the single camera's back-projection; the constructed scenes of
   tests/rig_scenes.py hold their stated properties on the reference's own structure; camera order and three wrong readings of the statement are told from it.
2. The host half (csrc/tdlo_rig_host.cpp) and through it the lane of phase A (csrc/tdlo_rig_point.h, the very code the GPU runs) built into
   tests/cpp/rig_host_test.cpp with -fsanitize=address,undefined (the runtimes linked into the program) and run as a child process on planes allocated at exactly their extents: R bit for bit
   against rig_ref.points on every scene.  The only sanitizer run; nothing sanitized is loaded into python.
3. The binding's names and marshalling against a stand-in library, as the other *_cpu.py files do."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import colour_ref
import rig_ref as R
import rig_scenes as S
import voxel_ref as V
from conftest import ROOT
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B

NEW = ["tdlo_rig_to_cloud", "tdlo_rig_to_cloud_visibility", "tdlo_tracker_frame_from_rig", "tdlo_rig_check", "tdlo_rig_points_host"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _differs(a, b):
    return a.shape != b.shape or not np.array_equal(_bits(a), _bits(b))


# ---- 1. the statement -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(64, 64), (65, 64), (1, 1), (3, 5)])
def test_one_camera_without_a_transform_is_the_single_back_projection(rows, cols):
    """Consequence (a) on the statement: points() of one camera with no transform is voxel_ref.backproject + to_float, bit for bit."""
    (cam, ), leaf = S.sized(rows, cols, 1)
    want = V.to_float(V.backproject(cam.depth, cam.mask, *cam.cam))
    got = R.points([cam])
    assert got.dtype == np.float32 and got.shape == want.shape and want.shape[0] > 0
    assert np.array_equal(_bits32(got), _bits32(want))
    Xa, na = R.rig_ref([cam], leaf)
    Xb, nb = V.voxel_ref(want, None, leaf)
    assert na == nb and np.array_equal(_bits(Xa), _bits(Xb))
    # ... the sign of a zero included, under pass-through
    (z, ), tiny = S.minus_zero()
    X, n_raw = R.rig_ref([z], tiny)
    st = V.structure(R.points([z]), None, tiny)
    assert st["nodown"] and X.shape[0] == n_raw
    row = np.nonzero((_bits(X)[:, 0] == 1 << 63) & (_bits(X)[:, 1] == 1 << 63) & (_bits(X)[:, 2] == 0))[0]
    assert len(row) == 1                                           # (-0.0, -0.0, +0.0): the masked pixel with depth 0 left of and above the centre


def test_the_order_of_two_sets_in_one_cell_shows_in_the_centroid():
    """Two sets of 40 float32 points uniform in one 8 mm cell at (0.1, 0.2, 0.6): the cell's centroid differs in bits when the sets are swapped."""
    rng = np.random.default_rng(0)
    lo = np.floor(np.array([0.1, 0.2, 0.6]) / 0.008) * 0.008
    a = (lo + 0.0004 + 0.0072 * rng.random((40, 3))).astype(np.float32)
    b = (lo + 0.0004 + 0.0072 * rng.random((40, 3))).astype(np.float32)
    Xab, _ = V.voxel_ref(np.concatenate([a, b]), None, 0.008)
    Xba, _ = V.voxel_ref(np.concatenate([b, a]), None, 0.008)
    assert Xab.shape == Xba.shape == (1, 3)
    assert not np.array_equal(_bits(Xab), _bits(Xba))


def test_camera_order_changes_the_reference():
    """The two-camera scene whose cameras contribute tens of points each to shared cells: swapping the cameras changes the cloud's bits (not its cells)."""
    cams, leaf = S.shared_cells()
    pa, pb = R.camera_points(cams[0]), R.camera_points(cams[1])
    ka = V.group(np.concatenate([pa, pb]), leaf)[3]
    both = np.intersect1d(ka[:len(pa)], ka[len(pa):])
    assert len(both) >= 20                                          # cells with points of both cameras
    cnt_a, cnt_b = np.bincount(ka[:len(pa)], minlength=int(ka.max()) + 1), np.bincount(ka[len(pa):], minlength=int(ka.max()) + 1)
    assert ((cnt_a[both] >= 20) & (cnt_b[both] >= 20)).sum() >= 20  # ... twenty of them with twenty points or more of each
    Xab, nab = R.rig_ref(cams, leaf)
    Xba, nba = R.rig_ref(cams[::-1], leaf)
    assert nab == nba and Xab.shape == Xba.shape
    differing = (_bits(Xab) != _bits(Xba)).any(axis=1).sum()
    assert differing >= 10 and np.abs(Xab - Xba).max() < 1e-6       # the same cells, other float sums


@pytest.mark.parametrize("wrong", [R.points_reversed, R.points_rounded_first, R.points_float_transform], ids=lambda f: f.__name__)
def test_three_wrong_readings_are_told_from_the_statement(wrong):
    """Cameras reversed; the camera point rounded to float before the transform; the transform evaluated in float32 -- on the scene with a rotation of
    0.3 rad about an oblique axis and a translation each gives another cloud."""
    cams, leaf = S.irrational()
    assert not np.array_equal(cams[1].T, np.round(cams[1].T, 6))    # (no short expansion)
    good = R.points(cams)
    bad = wrong(cams)
    assert good.shape == bad.shape
    if wrong is not R.points_reversed:
        assert (_bits32(good) != _bits32(bad)).any(axis=1).sum() >= 50                # R itself differs ...
    Xg, _ = V.voxel_ref(good, None, leaf)
    Xw, _ = V.voxel_ref(bad, None, leaf)
    assert Xg.shape == Xw.shape and (_bits(Xg) != _bits(Xw)).any(axis=1).sum() >= 5   # ... and so does the cloud


@pytest.mark.parametrize("wrong", [R.points_fused, R.points_fused_source_order], ids=lambda f: f.__name__)
def test_a_fused_transform_is_told_from_the_statement(wrong):
    """The fourth wrong reading: fused multiply-adds in the transform.  On the ordinary scenes it changes the double now and then and never the float; on the
    scene built for it tens of pixels land on the other side of a float rounding boundary, and the cloud differs."""
    cams, leaf = S.fused_boundary()
    good, bad = R.points(cams), wrong(cams)
    assert good.shape == bad.shape and good.shape[0] > 3000
    assert (_bits32(good) != _bits32(bad)).any(axis=1).sum() >= 20
    Xg, _ = V.voxel_ref(good, None, leaf)
    Xw, _ = V.voxel_ref(bad, None, leaf)
    assert Xg.shape == Xw.shape and (_bits(Xg) != _bits(Xw)).any(axis=1).sum() >= 20
    assert S.route(cams, leaf) == "taken"
    # ... where the rotation scene cannot tell them apart (which is why this scene exists)
    rc, _ = S.transform("rotation")
    small = [c.replaced(depth=c.depth[:12, :12], mask=c.mask[:12, :12]) for c in rc]
    assert np.array_equal(_bits32(R.points(small)), _bits32(wrong(small)))


ALL_SCENES = ([("sized", (r, c, K)) for r, c in ((64, 64), (65, 64), (1, 1), (3, 5)) for K in (1, 2, 3)] +
              [("shared_cells", ()), ("irrational", ()), ("fused_boundary", ()), ("overflow", ()), ("minus_zero", ()), ("minus_zero", (True, )), ("colour_rig", ())] +
              [("transform", (k, )) for k in S.TRANSFORMS] + [("empties", (w, )) for w in (0, 1, 2, "all")] + [("border", (n, )) for n in (32704, 32705)])


def _scene(name, args):
    return getattr(S, name)(*args)


def test_the_scenes_have_their_stated_properties():
    for K in (1, 2, 3):
        assert S.tiles(S.sized(64, 64, K)[0]) == K and S.tiles(S.sized(65, 64, K)[0]) == 2 * K      # one tile exactly; a second tile with a tail of 64 pixels
        for rows, cols in ((64, 64), (65, 64), (1, 1), (3, 5)):
            cams, leaf = S.sized(rows, cols, K)
            assert all(c.mask[-1, -1] != 0 for c in cams) and S.route(cams, leaf) == "taken"
    # empties: the camera in question contributes nothing, the others do; none at all: R is empty
    for w in (0, 1, 2):
        cams, leaf = S.empties(w)
        n = [R.camera_points(c).shape[0] for c in cams]
        assert n[w] == 0 and all(v > 1000 for k, v in enumerate(n) if k != w)
    assert R.points(S.empties("all")[0]).shape == (0, 3) and R.rig_ref(*S.empties("all"))[0].shape == (0, 3)
    # overflow: the second camera's masked pixels are dropped except one column; n_raw says so
    cams, leaf = S.overflow()
    masked = [int((c.mask != 0).sum()) for c in cams]
    kept = [R.camera_points(c).shape[0] for c in cams]
    assert kept[0] == masked[0] and kept[1] == cams[1].depth.shape[0] < masked[1]
    assert R.rig_ref(cams, leaf)[1] == sum(kept) and S.route(cams, leaf) == "taken"
    # transforms: the identity given as a matrix is the point itself
    cams, leaf = S.transform("identity")
    assert np.array_equal(_bits32(R.camera_points(cams[1])), _bits32(R.camera_points(cams[1].replaced(T=None))))
    for k in ("translation", "rotation", "scale"):
        cams, leaf = S.transform(k)
        assert not np.array_equal(_bits32(R.camera_points(cams[1])), _bits32(R.camera_points(cams[1].replaced(T=None)))) and S.route(cams, leaf) == "taken"
    # the point border
    assert R.rig_ref(*S.border(32704))[1] == 32704 and S.route(*S.border(32704)) == "taken"
    assert R.rig_ref(*S.border(32705))[1] == 32705 and S.route(*S.border(32705)) == "passed"
    # pass-through
    assert S.route(*S.minus_zero()) == "passed" and S.route(*S.minus_zero(True)) == "passed"
    # the tile border: 63 x 65 = 4095 tiles are served, 64 x 64 = 4096 are not
    assert 63 * ((262145 + 4095) // 4096) == S.kFTmax and 64 * (262144 // 4096) == S.kFTmax + 1
    # the colour rig: both cameras segment something, the occluder hides some of the second's
    cams, leaf = S.colour_rig()
    k0, k1 = cams[0].kept(), cams[1].kept()
    free = cams[1].replaced(occluder=None).kept()
    assert k0.sum() > 300 and 300 < k1.sum() < free.sum() and not k1[:, 20:30].any() and S.route(cams, leaf) == "taken"


# ---- 2. the host half under a sanitizer -----------------------------------------------------------------------------------------------------------------------
def _case_bytes(cams):
    rows, cols = cams[0].depth.shape
    blob = [np.array([len(cams), rows, cols], dtype=np.int64).tobytes()]
    for c in cams:
        blob.append(np.array([c.mask is not None, c.colour is not None, c.occluder is not None, c.T is not None], dtype=np.int64).tobytes())
        blob.append(np.array(c.cam, dtype=np.float64).tobytes())
        blob.append((np.zeros(12) if c.T is None else c.T.reshape(12)).astype(np.float64).tobytes())
        cp = np.zeros(26, dtype=np.int32)
        if c.ranges is not None:
            lower, upper, rgb = c.ranges
            n = len(lower)
            cp[0] = n; cp[1:1 + 3 * n] = np.asarray(lower).reshape(-1); cp[13:13 + 3 * n] = np.asarray(upper).reshape(-1); cp[25] = rgb
        blob.append(cp.tobytes())
        blob.append(c.depth.tobytes())
        for plane in (c.mask, c.colour, c.occluder):
            if plane is not None:
                blob.append(plane.tobytes())
    return b"".join(blob)


def test_the_host_half_compiled_under_a_sanitizer(tmp_path):
    exe = str(tmp_path / "rig_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "rig_host_test.cpp"), os.path.join(ROOT, "trackdlo_amd", "csrc", "tdlo_rig_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    scenes = [_scene(n, a)[0] for n, a in ALL_SCENES]
    # the colour cube's hard corners for the host segmentation: a camera whose colour image walks through random colours under the four ranges, RGB order
    rng = np.random.default_rng(7)
    d, m = S.surface(33, 47, 5)
    img = rng.integers(0, 256, (33, 47, 3)).astype(np.uint8)
    occ = ((rng.random((33, 47)) < 0.8) * 255).astype(np.uint8)
    scenes.append((R.Cam(d, colour=img, ranges=(*colour_ref.MULTI_RANGES, 1), occluder=occ, cam=S.CAM, T=S.IRRATIONAL),
                   R.Cam(d, colour=img[::-1].copy(), ranges=([[0, 0, 0], [200, 0, 0]], [[180, 255, 90], [100, 255, 255]], 0), cam=S.CAM)))
    refused = [(R.Cam(d, m, cam=(0.0, 600.0, 1.0, 1.0)), ), (R.Cam(d, m, cam=S.CAM), R.Cam(d, colour=img, ranges=(*colour_ref.LAUNCH_RANGE, 0), cam=S.CAM))]
    (tmp_path / "cases.bin").write_bytes(np.array([len(scenes) + len(refused)], dtype=np.int64).tobytes() + b"".join(_case_bytes(c) for c in scenes + refused))
    # (the runtimes are linked into the program: it starts in the environment as it is)
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(scenes) + len(refused)} cases run" in r.stdout, r.stdout
    got = (tmp_path / "out.bin").read_bytes()
    at = 0
    for k, cams in enumerate(scenes):
        rc, n = np.frombuffer(got, dtype=np.int64, count=2, offset=at)
        want = R.points(cams)
        assert rc == 0 and n == want.shape[0], (k, rc, n, want.shape)
        Rg = np.frombuffer(got, dtype=np.float32, count=3 * int(n), offset=at + 16).reshape(-1, 3)
        assert np.array_equal(_bits32(Rg), _bits32(want)), (k, int((_bits32(Rg) != _bits32(want)).any(axis=1).sum()))
        at += 16 + 12 * int(n)
    for cams in refused:
        rc, n = np.frombuffer(got, dtype=np.int64, count=2, offset=at)
        assert rc == B.TDLO_E_INVALID and n == 0
        at += 16
    assert at == len(got)
    assert 200 < R.points(scenes[-1]).shape[0] < 2 * 33 * 47        # (the random colour images pass some pixels and not others)


# ---- 3. names and marshalling -----------------------------------------------------------------------------------------------------------------------------------
def test_the_new_names_are_declared_required_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_rig_camera;" in hdr
    assert "#define TDLO_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    for name in ("rig_to_cloud", "rig_to_cloud_visibility", "rig_points_host", "rig_route_counts"):
        assert callable(getattr(B.Context, name))
    assert callable(B.trackdlo.frame_from_rig) and callable(B.rig_points_host) and callable(B.rig_check)
    assert [f[0] for f in B.RigCameraC._fields_] == ["depth", "mask", "colour", "occluder", "colour_params", "fx", "fy", "cx", "cy", "cam_to_rig"]
    assert C.sizeof(B.RigCameraC) == 80
    assert lib.tdlo_debug_route_count(None, 45) == -1
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    assert " * 45 / 46 / 47: rigs (tdlo_rig_to_cloud" in text


def test_the_host_half_through_the_binding():
    """tdlo_rig_check and tdlo_rig_points_host as the library exports them (no context, no GPU): the refusals of the contract, and R of two scenes."""
    for name, args in (("irrational", ()), ("colour_rig", ()), ("sized", (65, 64, 3))):
        cams, _ = _scene(name, args)
        bc = S.binding_cams(B, cams)
        assert B.rig_check(bc) == 0
        assert np.array_equal(_bits32(B.rig_points_host(bc)), _bits32(R.points(cams))), name
    cams, _ = S.irrational()
    a, b = cams
    d, m = a.depth, a.mask
    img = S.paint(m, 3)
    blue = (*colour_ref.LAUNCH_RANGE, 0)
    E = B.TDLO_E_INVALID
    bad = {
        "65 cameras": [a] * 65,
        "too many pixels": [R.Cam(np.zeros((4096, 4096), np.uint16), np.zeros((4096, 4096), np.uint8), cam=S.CAM)] * 5,
        "neither mask nor colour": [a, R.Cam(d, cam=S.CAM)],
        "mixed kinds": [a, R.Cam(d, colour=img, ranges=blue, cam=S.CAM)],
        "fx = 0": [a.replaced(cam=(0.0, 600.0, 1.0, 1.0))],
        "fy = 0": [a, b.replaced(cam=(600.0, 0.0, 1.0, 1.0))],
        "nan in cam_to_rig": [a, b.replaced(T=np.where(np.arange(12).reshape(3, 4) == 7, np.nan, b.T))],
        "inf in cam_to_rig": [a.replaced(T=np.where(np.arange(12).reshape(3, 4) == 0, np.inf, b.T))],
    }
    for what, cams in bad.items():
        assert B.rig_check(S.binding_cams(B, cams)) == E, what
    # colour without ranges, bad ranges
    cc = S.binding_cams(B, [R.Cam(d, colour=img, ranges=blue, cam=S.CAM)])
    assert B.rig_check(cc) == 0
    cc[0].params = None
    assert B.rig_check(cc) == E
    p = B.make_colour_params(); p.n_ranges = 5
    cc[0].params = p
    assert B.rig_check(cc) == E
    # leaf
    good = S.binding_cams(B, [a, b])
    for leaf in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        assert B.rig_check(good, leaf) == E, leaf
    assert B.rig_check(good, 0.008) == 0
    with pytest.raises(ValueError):
        B.rig_check([])


class StubLib:
    """Records what the binding hands to the three entry points and fills the outputs like the library would."""
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    def tdlo_get_cloud(self, h, slot, X, cap, n):
        return 0

    @staticmethod
    def _cams(cams, K, rows, cols):
        out = []
        for cm in (B.RigCameraC * K).from_address(addr(cams)):
            d = dict(cam=(cm.fx, cm.fy, cm.cx, cm.cy), T=None if not cm.cam_to_rig else arr(cm.cam_to_rig, 12, C.c_double), params=None)
            for name, ct, n in (("depth", C.c_uint16, rows * cols), ("mask", C.c_uint8, rows * cols), ("colour", C.c_uint8, 3 * rows * cols), ("occluder", C.c_uint8, rows * cols)):
                p = getattr(cm, name)
                d[name] = None if not p else arr(p, n, ct)
            if cm.colour_params:
                cp = B.ColourParams.from_address(cm.colour_params)
                d["params"] = (cp.n_ranges, [list(cp.lower[k]) for k in range(cp.n_ranges)], [list(cp.upper[k]) for k in range(cp.n_ranges)], cp.rgb_order)
            out.append(d)
        return out

    def tdlo_rig_to_cloud(self, h, slot, cams, K, rows, cols, leaf, X, cap, n, nraw):
        self.calls.append(dict(fn="cloud", h=h, slot=slot, K=K, rows=rows, cols=cols, leaf=leaf, cams=self._cams(cams, K, rows, cols), X=addr(X), cap=cap))
        n._obj.value = 11; nraw._obj.value = 111
        return self.rc

    def tdlo_rig_to_cloud_visibility(self, h, slot, cams, K, rows, cols, leaf, Y, M, thr, d_vis, coord, dist, vis, nv, ext, ne, n, nraw):
        self.calls.append(dict(fn="vis", h=h, slot=slot, K=K, rows=rows, cols=cols, leaf=leaf, cams=self._cams(cams, K, rows, cols), Y=arr(Y, 3 * M, C.c_double), M=M,
                               thr=thr, d_vis=d_vis, coord=arr(coord, M, C.c_double)))
        (C.c_double * M).from_address(addr(dist))[0] = 0.25
        (C.c_int * M).from_address(addr(vis))[0] = 2
        e = (C.c_int * M).from_address(addr(ext)); e[0] = 2; e[1] = 3
        nv._obj.value = 1; ne._obj.value = 2; n._obj.value = 12; nraw._obj.value = 112
        return self.rc

    def tdlo_tracker_frame_from_rig(self, t, cams, K, rows, cols, leaf, d_vis, vis, nv, ext, ne, n, nraw, stats):
        self.calls.append(dict(fn="frame", t=t, K=K, rows=rows, cols=cols, leaf=leaf, d_vis=d_vis, cams=self._cams(cams, K, rows, cols)))
        M = 4
        (C.c_int * M).from_address(addr(vis))[0] = 1
        e = (C.c_int * M).from_address(addr(ext)); e[0] = 1; e[1] = 2
        nv._obj.value = 1; ne._obj.value = 2; n._obj.value = 13; nraw._obj.value = 113
        st = (B.Stats * 2).from_address(addr(stats))
        st[0].iters = 5; st[1].iters = 6
        return self.rc


def test_rig_marshalling():
    lib = StubLib()
    ctx = stub_context(lib)
    rows, cols = 3, 5
    rng = np.random.default_rng(1)
    d0 = rng.integers(0, 65536, (rows, cols)).astype(np.uint16); m0 = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    d1 = rng.integers(0, 65536, (rows, cols)).astype(np.uint16); m1 = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    T = np.arange(12, dtype=np.float64).reshape(3, 4) + 0.5
    cams = [B.RigCamera(d0, mask=m0, cam=(600.0, 601.0, 2.5, 1.5)), B.RigCamera(d1.astype(np.int64), mask=m1, cam=(1, 2, 3, 4), cam_to_rig=T)]
    X, n, nraw = ctx.rig_to_cloud(3, cams, 0.008, fetch=False)
    c = lib.calls[-1]
    assert (c["fn"], c["h"], c["slot"], c["K"], c["rows"], c["cols"], c["leaf"], c["X"], c["cap"]) == ("cloud", 0x1234, 3, 2, rows, cols, 0.008, 0, 0)
    c0, c1 = c["cams"]
    assert c0["cam"] == (600.0, 601.0, 2.5, 1.5) and c0["T"] is None and c0["depth"] == d0.reshape(-1).tolist() and c0["mask"] == m0.reshape(-1).tolist()
    assert c0["colour"] is None and c0["occluder"] is None and c0["params"] is None
    assert c1["cam"] == (1.0, 2.0, 3.0, 4.0) and c1["T"] == T.reshape(-1).tolist() and c1["depth"] == d1.reshape(-1).tolist() and c1["mask"] == m1.reshape(-1).tolist()
    assert (X, n, nraw) == (None, 11, 111)
    # a colour rig: ranges per camera, an occluder
    img = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8); occ = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    two = B.make_colour_params([[0, 60, 50], [15, 100, 80]], [[10, 255, 255], [40, 255, 255]], rgb_order=1)
    cc = [B.RigCamera(d0, colour=img, params=B.make_colour_params(), cam=(5, 6, 7, 8)), B.RigCamera(d1, colour=img, params=two, occluder=occ, cam=(5, 6, 7, 8), cam_to_rig=T)]
    Y = rng.standard_normal((4, 3)); coord = np.arange(4) * 0.01
    dist, vis, ext, n, nraw = ctx.rig_to_cloud_visibility(1, cc, 0.01, Y, 0.008, 0.06, coord)
    c = lib.calls[-1]
    assert (c["fn"], c["slot"], c["K"], c["leaf"], c["M"], c["thr"], c["d_vis"]) == ("vis", 1, 2, 0.01, 4, 0.008, 0.06)
    assert c["cams"][0]["params"] == (1, [[90, 90, 30]], [[130, 255, 255]], 0) and c["cams"][0]["mask"] is None and c["cams"][0]["colour"] == img.reshape(-1).tolist()
    assert c["cams"][1]["params"] == (2, [[0, 60, 50], [15, 100, 80]], [[10, 255, 255], [40, 255, 255]], 1) and c["cams"][1]["occluder"] == occ.reshape(-1).tolist()
    assert c["coord"] == coord.tolist() and sorted(c["Y"]) == sorted(Y.reshape(-1).tolist())
    assert dist[0] == 0.25 and vis.tolist() == [2] and ext.tolist() == [2, 3] and (n, nraw) == (12, 112)
    # the tracker call
    trk = stub_tracker(ctx, 0x3000)
    patched_handles([trk])
    v, e, n, nraw = trk.frame_from_rig(cams, 0.009, 0.05)
    c = lib.calls[-1]
    assert (c["fn"], c["t"], c["K"], c["rows"], c["cols"], c["leaf"], c["d_vis"]) == ("frame", 0x3000, 2, rows, cols, 0.009, 0.05)
    assert c["cams"][1]["T"] == T.reshape(-1).tolist()
    assert v.tolist() == [1] and e.tolist() == [1, 2] and (n, nraw) == (13, 113) and [s["iters"] for s in trk.last_stats] == [5, 6]
    # a code is raised; a plane of the wrong shape never reaches the library
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.rig_to_cloud(0, cams, 0.008, fetch=False)
    ncalls = len(lib.calls)
    with pytest.raises(ValueError):
        ctx.rig_to_cloud(0, [B.RigCamera(d0, mask=m0[:, :4])], 0.008, fetch=False)
    assert len(lib.calls) == ncalls
    trk.h = None
    # cam_to_rig: 3 x 4 or its 12 entries; a 4 x 4 matrix is not cut down silently
    assert B.RigCamera(d0, mask=m0, cam_to_rig=T.reshape(12)).cam_to_rig.tolist() == T.reshape(-1).tolist()
    for bad in (np.eye(4), np.zeros((4, 3)), np.zeros(11), np.zeros((2, 6))):
        with pytest.raises(ValueError):
            B.RigCamera(d0, mask=m0, cam_to_rig=bad)
