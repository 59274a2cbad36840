"""Depth aligned to the colour camera without a GPU: the vectorised numpy statement (tests/align_ref.py) equals its literal per-pixel restatement; the host
call tdlo_align_depth_host equals the statement bit for bit, counts included, on every scene and through pitched and bottom-up views; every scene has the
property it is there for; tdlo_align_check refuses what the header says; the wrong readings of the statement are each told from it on a named scene; the
lanes run over their whole grids in a sanitized stand-alone program; the new names are declared, exported and marshalled as the header lays them out."""
import ctypes as C
from fractions import Fraction
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tracker_batch_cpu import addr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B
import align_ref as AR

NEW = ["tdlo_align_check", "tdlo_align_depth_host", "tdlo_align_depth", "tdlo_frame_to_cloud_view_aligning", "tdlo_tracker_frame_view_aligning"]
SCENES = AR.all_scenes()
_REF = {}


def ref(name):
    """the statement's (plane, counts) of a scene, computed once"""
    if name not in _REF:
        A, n = AR.align(SCENES[name]["D"], SCENES[name]["p"])
        A.setflags(write=False)
        _REF[name] = (A, n)
    return _REF[name]


def host(s, kind="packed", **over):
    D = s["D"]
    buf, off, stride = AR.as_view_array(D, kind)
    v = B.ImageView(buf.ctypes.data + off, B.IMG_F32C1 if D.dtype == np.float32 else B.IMG_U16C1, B.MEM_HOST, stride, None)
    v.rows, v.cols = D.shape
    out = B.align_depth_host(v, B.make_align_params(**dict(s["p"], **over)))
    del buf
    return out


def test_the_new_names_are_declared_exported_and_documented():
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_align_params;" in hdr and lib.tdlo_abi_version() == 3
    f = B.AlignParams
    assert C.sizeof(f) == 96 and (f.rows_d.offset, f.fx_d.offset, f.rows_c.offset, f.fx_c.offset, f.depth_to_colour.offset, f.max_footprint.offset) == (0, 8, 40, 48, 80, 88)
    assert lib.tdlo_debug_route_count(None, 59) == -1 and lib.tdlo_debug_route_count(None, 60) == -1
    assert re.search(r"\* 59 / 60: aligned planes", text)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "tdlo_align_depth" in open(os.path.join(ROOT, doc)).read(), doc
    mk = open(os.path.join(ROOT, "trackdlo_amd", "csrc", "Makefile")).read()
    for unit in ("tdlo_align.hip", "tdlo_align_host.cpp"):
        line = [ln for ln in mk.splitlines() if f"-c {unit}" in ln]
        assert len(line) == 1 and "-ffp-contract=off" in line[0] and "fast-math" not in line[0].split("#")[0], unit


@pytest.mark.parametrize("name", [n for n, s in SCENES.items() if s["D"].size <= 3100])
def test_the_vectorised_statement_equals_the_literal_loop(name):
    A, n = ref(name)
    L, ln = AR.align_literal(SCENES[name]["D"], SCENES[name]["p"])
    assert np.array_equal(A, L) and n == ln


@pytest.mark.parametrize("name", list(SCENES))
def test_the_host_call_equals_the_statement(name):
    A, n = ref(name)
    for kind in ("packed", "pitched", "bottom_up"):
        H, hn = host(SCENES[name], kind)
        assert np.array_equal(A, H) and n == hn, (name, kind, n, hn)


def test_the_full_size_case_on_the_host():
    s = AR.scene_rope()
    A, n = AR.align(s["D"], s["p"])
    H, hn = host(s)
    assert np.array_equal(A, H) and n == hn and n[1] > 5000 and n[0] < 0.1 * s["D"].size


def footprints(name):
    s = SCENES[name]
    ver, (x0, y0, x1, y1) = AR.verdicts(s["D"], s["p"])
    return s, ver, x0, y0, x1, y1


def bad_corners(s):
    K = AR.to_mm(s["D"])
    return (AR._corners(K, s["p"], -0.5)[2] | AR._corners(K, s["p"], 0.5)[2]) & (K != 0)


def test_every_scene_has_the_property_it_is_there_for():
    for name in ("1x1", "1x63", "1x64", "1x65", "3x257", "5x7"):                       # the wave and block borders: used pixels up to the last lane
        s, ver, *_ = footprints(name)
        assert ver.reshape(-1)[-1] == 1 and ref(name)[1][1] >= 0.7 * s["D"].size, name
    s, ver, x0, y0, x1, y1 = footprints("upscale")
    u = ver == 1
    assert set(np.unique((x1 - x0 + 1)[u])) == {2, 3} == set(np.unique((y1 - y0 + 1)[u]))
    assert ref("upscale_mf1")[1][1] == 0 and ref("upscale_mf1")[1][3] == ref("upscale")[1][1] and not ref("upscale_mf1")[0].any()
    s, ver, x0, y0, x1, y1 = footprints("downscale")
    offers = np.zeros((s["p"]["rows_c"], s["p"]["cols_c"]), int)
    for a, b, c, d in zip(x0[ver == 1], y0[ver == 1], x1[ver == 1], y1[ver == 1]):
        offers[b:d + 1, a:c + 1] += 1
    assert offers.min() >= 4                                                           # contention for the minimum at every output pixel
    A, n = ref("one_pixel")
    assert n[1] == n[0] > 600 and (A != 0).sum() == 1 and A.max() == SCENES["one_pixel"]["D"][SCENES["one_pixel"]["D"] > 0].min()
    assert np.array_equal(ref("identical_null")[0], ref("identical_eye")[0]) and ref("identical_null")[1] == ref("identical_eye")[1]
    assert (ref("identical_null")[0] != SCENES["identical_null"]["D"]).sum() > 0.5 * SCENES["identical_null"]["D"].size       # the result is not D
    s, ver, x0, y0, x1, y1 = footprints("border")
    K, R, Cc = s["D"] != 0, s["p"]["rows_c"], s["p"]["cols_c"]
    for straddles in (K & (x0 < 0) & (x1 >= 0), K & (y0 < 0) & (y1 >= 0), K & (x0 < Cc) & (x1 >= Cc), K & (y0 < R) & (y1 >= R)):
        assert straddles.sum() > 10 and (ver[straddles] == 2).all()                    # dropped whole at every one of the four borders
    _, _, _, px, py = AR._corners(AR.to_mm(s["D"]), s["p"], -0.5)
    assert (K & (px > -1.5) & (px < -0.5)).sum() > 5 and (K & (py > -1.5) & (py < -0.5)).sum() > 5 and ref("border")[1][1] > 1000
    s, ver, x0, y0, x1, y1 = footprints("rot180")
    assert (x1 < x0)[s["D"] != 0].all() and not bad_corners(s).any() and ref("rot180")[1][2] == ref("rot180")[1][0] > 0
    s, ver, *_ = footprints("looking_away")
    assert bad_corners(s)[s["D"] != 0].all() and ref("looking_away")[1][2] == ref("looking_away")[1][0] > 0
    s, ver, *_ = footprints("rot80")
    bad = bad_corners(s) & (s["D"] != 0)
    assert bad.sum() > 100 and ((ver == 2) & ~bad).sum() > 100 and (ver == 1).sum() > 100      # q_z crosses 0 inside the image
    assert ref("ratio20")[1][3] == ref("ratio20")[1][0] > 0 and ref("ratio20_mf64")[1][1] == ref("ratio20")[1][0] and ref("ratio20_mf64")[0].any()
    assert ref("ratio20_border")[1][2] > 50 and ref("ratio20_border")[1][3] > 20
    D = SCENES["f32"]["D"].reshape(-1)
    exact = [int(np.floor(Fraction(float(d)) * 1000 + Fraction(1, 2))) if np.isfinite(d) else -1 for d in D]      # the rule in exact arithmetic
    assert AR.to_mm(D).tolist() == [e if 0 <= e < 65536 else 0 for e in exact]
    assert not AR.to_mm(D[:5]).any() and AR.to_mm(D[7:8])[0] == 0 and not np.isfinite(D[:3]).any() and (D[3:5] < 0).all() and D[7] > 65.536
    near = [abs(Fraction(float(d)) * 1000 % 1 - Fraction(1, 2)) for d in D[14:40]]
    assert max(near) < Fraction(1, 10000) and len({AR.to_mm(D[14 + i:15 + i])[0] - int(float(D[14 + i]) * 1000) for i in range(26)}) == 2      # both sides of .5 mm
    assert not ref("all_zero")[0].any() and ref("all_zero")[1] == [0, 0, 0, 0]


def test_refusals_of_tdlo_align_check():
    p = SCENES["upscale"]["p"]
    assert B.align_check(B.make_align_params(**p)) == 0 and B.align_check(None) == B.TDLO_E_INVALID
    nanT = p["T"].copy(); nanT[1, 2] = np.nan
    infT = p["T"].copy(); infT[2, 3] = np.inf
    bads = [dict(rows_d=0), dict(cols_d=-1), dict(rows_c=0), dict(cols_c=0), dict(rows_d=8193, cols_d=8193), dict(rows_c=1 << 14, cols_c=(1 << 12) + 1),
            dict(fx_d=0.0), dict(fy_d=-1.0), dict(fx_c=np.nan), dict(fy_c=np.inf), dict(fx_d=np.nan), dict(fy_d=np.inf), dict(fx_c=-2.0), dict(fy_c=0.0),
            dict(cx_d=np.nan), dict(cy_c=np.inf), dict(T=nanT), dict(T=infT), dict(max_footprint=-1), dict(max_footprint=65)]
    for bad in bads:
        assert B.align_check(B.make_align_params(**dict(p, **bad))) == B.TDLO_E_INVALID, bad
        with pytest.raises(B.TdloError):
            host(SCENES["upscale"], **bad)
    for ok in (dict(max_footprint=1), dict(max_footprint=64), dict(rows_c=1 << 13, cols_c=1 << 13)):
        assert B.align_check(B.make_align_params(**dict(p, **ok))) == 0, ok
    # the host call refuses a view that is no depth view of the depth camera's size
    D = SCENES["upscale"]["D"]
    with pytest.raises(B.TdloError):
        B.align_depth_host(B.image_view(np.zeros(D.shape, np.uint8)), B.make_align_params(**p))
    v = B.image_view(D)
    v.row_stride = 2 * D.shape[1] - 2                                                  # rows overlap
    with pytest.raises(B.TdloError):
        B.align_depth_host(v, B.make_align_params(**p))


WRONG = [("trunc", "identical_null", dict(rounding="trunc")), ("float32", "identical_null", dict(dtype=np.float32)), ("last writer", "downscale", dict(reduce="last")),
         ("maximum", "downscale", dict(reduce="max")), ("centre only", "upscale", dict(footprint=False)), ("clipped", "border", dict(clip=True)),
         ("fused transform", "fused", dict(fused=True))]


@pytest.mark.parametrize("what,name,kw", WRONG, ids=[w[0] for w in WRONG])
def test_a_wrong_reading_is_told_from_the_statement(what, name, kw):
    A, n = ref(name)
    W, wn = AR.align_literal(SCENES[name]["D"], SCENES[name]["p"], **kw)
    assert (A != W).sum() >= 1, what                                                   # a scene that fails to separate fails here
    H, hn = host(SCENES[name])
    assert np.array_equal(H, A) and not np.array_equal(H, W)                           # ... and the library stands on the statement's side


def test_the_fused_transform_is_not_told_by_a_generic_scene():
    """why the fused scene is constructed: neither identical cameras under T = identity nor the generic T of the upscale scene moves a corner over a border"""
    for name in ("identical_eye", "upscale"):
        W, wn = AR.align_literal(SCENES[name]["D"], SCENES[name]["p"], fused=True)
        assert np.array_equal(W, ref(name)[0]) and wn == ref(name)[1]


def test_the_wide_test_in_front_of_the_border_test_is_told_by_the_counts():
    """A footprint that is wide AND over the border is used by neither reading, so the planes of the two cannot differ on any scene; the counts do: the
    statement counts it as dropped."""
    name = "ratio20_border"
    A, n = ref(name)
    W, wn = AR.align_literal(SCENES[name]["D"], SCENES[name]["p"], wide_first=True)
    assert np.array_equal(A, W) and n != wn and n[2] > 0 and wn[2] == 0 and wn[3] == n[2] + n[3]
    assert host(SCENES[name])[1] == n


def test_lanes_over_their_grids_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/align_lane_host_test.cpp with csrc/tdlo_align_host.cpp and csrc/tdlo_image_host.cpp: no HIP, built with -fsanitize=address,undefined (the
    runtime linked into the program) and run as a child process of its own.  Nothing sanitized is loaded into python."""
    cases = [("border", 0), ("border", 1), ("border", 2), ("ratio20", 0), ("ratio20_mf64", 2), ("ratio20_border", 1), ("rot180", 0), ("rot80", 1), ("rot80", 2),
             ("looking_away", 0), ("f32", 1), ("f32", 2), ("3x257", 2), ("1x65", 0), ("5x7", 1), ("upscale", 0), ("one_pixel", 0), ("all_zero", 0)]
    blob = [struct.pack("<i", len(cases))]
    for name, layout in cases:
        s = SCENES[name]
        p, D = s["p"], np.ascontiguousarray(s["D"])
        A, n = ref(name)
        blob.append(struct.pack("<8i", p["rows_d"], p["cols_d"], p["rows_c"], p["cols_c"], B.IMG_F32C1 if D.dtype == np.float32 else B.IMG_U16C1,
                                int(p["T"] is not None), p["max_footprint"], layout))
        T = np.zeros(12) if p["T"] is None else p["T"].reshape(12)
        blob.append(struct.pack("<20d", *[p[k] for k in ("fx_d", "fy_d", "cx_d", "cy_d", "fx_c", "fy_c", "cx_c", "cy_c")], *T))
        blob += [D.tobytes(), np.ascontiguousarray(A).tobytes(), struct.pack("<4q", *n)]
    path = tmp_path / "scenes.bin"
    path.write_bytes(b"".join(blob))
    exe = str(tmp_path / "align_lane_host_test")
    csrc = os.path.join(ROOT, "trackdlo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "align_lane_host_test.cpp"), os.path.join(csrc, "tdlo_align_host.cpp"),
                        os.path.join(csrc, "tdlo_image_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"(\d+) scenes, (\d+) lanes, (\d+) words, 0 differing\n", r.stdout)
    words = sum(SCENES[name]["p"]["rows_c"] * SCENES[name]["p"]["cols_c"] for name, _ in cases)
    assert m and int(m.group(1)) == len(cases) and int(m.group(3)) == words and int(m.group(2)) % 256 == 0, r.stdout


# ---- marshalling against a stand-in library ----------------------------------------------------------------------------------------------------------
class StubLib:
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    @staticmethod
    def _params(p):
        q = B.AlignParams.from_address(addr(p))
        d = {k: getattr(q, k) for k, _ in B.AlignParams._fields_}
        d["T"] = list((C.c_double * 12).from_address(q.depth_to_colour)) if q.depth_to_colour else None
        return d

    @staticmethod
    def _view(v):
        return dict(data=v.data, format=v.format, location=v.location, row_stride=v.row_stride, ready_stream=v.ready_stream)

    @staticmethod
    def _counts(cnt, base):
        a = (C.c_longlong * 4).from_address(addr(cnt))
        for i in range(4):
            a[i] = base + i

    def tdlo_align_depth(self, h, depth, p, out, plane, cnt):                          # (the header's order)
        self.calls.append(dict(h=h, depth=self._view(B.ImageView.from_address(addr(depth))), p=self._params(p), out=addr(out)))
        plane._obj.value = 0xABC000
        self._counts(cnt, 10)
        return self.rc

    def tdlo_frame_to_cloud_view_aligning(self, h, slot, fv, p, cp, leaf, X, cap, n, nraw, cnt):
        f = B.FrameView.from_address(addr(fv))
        self.calls.append(dict(h=h, slot=slot, fv={k: self._view(getattr(f, k)) for k in ("depth", "colour", "occluder", "mask")}, p=self._params(p), cp=addr(cp), leaf=leaf, cap=cap))
        n._obj.value = 2; nraw._obj.value = 5
        if addr(X):
            (C.c_double * 6).from_address(addr(X))[:] = [1, 2, 3, 4, 5, 6]
        self._counts(cnt, 20)
        return self.rc

    def tdlo_tracker_frame_view_aligning(self, t, fv, p, cp, leaf, d_vis, vis, nv, ext, ne, n, nraw, st, cnt):
        f = B.FrameView.from_address(addr(fv))
        self.calls.append(dict(t=t, fv={k: self._view(getattr(f, k)) for k in ("depth", "colour", "occluder", "mask")}, p=self._params(p), cp=addr(cp), leaf=leaf, d_vis=d_vis))
        nv._obj.value = 1; ne._obj.value = 2; n._obj.value = 7; nraw._obj.value = 9
        (C.c_int * 1).from_address(addr(vis))[0] = 3
        (C.c_int * 2).from_address(addr(ext))[:] = [2, 3]
        self._counts(cnt, 30)
        return self.rc


def test_argtypes_are_the_header_s():
    L = B.load_library()
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    assert len(L.tdlo_align_check.argtypes) == 1 and len(L.tdlo_align_depth_host.argtypes) == 4 and len(L.tdlo_align_depth.argtypes) == 6
    a = L.tdlo_frame_to_cloud_view_aligning.argtypes
    assert len(a) == 11 and (a[0], a[1], a[5], a[6], a[7]) == (vp, ci, cd, vp, ci)
    a = L.tdlo_tracker_frame_view_aligning.argtypes
    assert len(a) == 14 and (a[0], a[4], a[5], a[6], a[12]) == (vp, cd, cd, vp, vp)


def test_marshalling_against_a_stand_in_library():
    lib = StubLib()
    ctx = stub_context(lib)
    s = SCENES["upscale"]
    p = B.make_align_params(**s["p"])
    D = s["D"]
    A, cnt, plane = ctx.align_depth(D, p)
    k = lib.calls[-1]
    assert k["h"] == 0x1234 and k["depth"] == dict(data=D.ctypes.data, format=B.IMG_U16C1, location=B.MEM_HOST, row_stride=2 * D.shape[1], ready_stream=None)
    assert k["out"] == A.ctypes.data and A.shape == (72, 96) and cnt == [10, 11, 12, 13] and plane == 0xABC000
    assert {q: k["p"][q] for q in s["p"] if q != "T"} == {q: s["p"][q] for q in s["p"] if q != "T"} and k["p"]["T"] == s["p"]["T"].reshape(-1).tolist()
    assert ctx.align_depth(D, B.make_align_params(**dict(s["p"], T=None)), out=None)[0] is None and lib.calls[-1]["out"] == 0 and lib.calls[-1]["p"]["T"] is None
    assert ctx.align_depth(D, p, out=0x7002)[0] is None and lib.calls[-1]["out"] == 0x7002
    mask = np.ones((72, 96), np.uint8)
    X, n, nraw, cnt = ctx.frame_to_cloud_view_aligning(3, dict(depth=D, mask=mask), p, None, 0.008)
    k = lib.calls[-1]
    assert (k["slot"], k["cp"], k["leaf"], k["cap"]) == (3, 0, 0.008, 72 * 96) and k["fv"]["depth"]["data"] == D.ctypes.data and k["fv"]["mask"]["data"] == mask.ctypes.data
    assert k["fv"]["colour"]["data"] is None and k["fv"]["mask"]["row_stride"] == 96 and k["fv"]["depth"]["row_stride"] == 128
    assert X.tolist() == [[1, 3, 5], [2, 4, 6]] and (n, nraw, cnt) == (2, 5, [20, 21, 22, 23])
    with pytest.raises(ValueError):
        B.aligning_frame_view(D, colour=np.zeros((72, 96, 3), np.uint8), occluder=np.zeros((48, 64), np.uint8))
    trk = stub_tracker(ctx, 0x3000)
    patched_handles([trk])
    cp = B.make_colour_params()
    col = np.zeros((72, 96, 4), np.uint8)
    v, e, n, nraw, cnt = trk.frame_view_aligning(dict(depth=D.astype(np.float32), colour=col), p, cp, 0.01, 0.05)
    k = lib.calls[-1]
    assert k["t"] == 0x3000 and k["cp"] == C.addressof(cp) and (k["leaf"], k["d_vis"]) == (0.01, 0.05)
    assert k["fv"]["depth"]["format"] == B.IMG_F32C1 and k["fv"]["colour"]["format"] == B.IMG_U8C4 and k["fv"]["colour"]["row_stride"] == 4 * 96
    assert v.tolist() == [3] and e.tolist() == [2, 3] and (n, nraw, cnt) == (7, 9, [30, 31, 32, 33])
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.align_depth(D, p)
    with pytest.raises(B.TdloError):
        trk.frame_view_aligning(dict(depth=D, colour=col), p, cp)
    trk.h = None
