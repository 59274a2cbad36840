"""The self-occlusion test under a rig without a GPU: the scenes of tests/rig_painter_scenes.py assert their own properties on the numpy / integer statement
(tests/rig_painter_ref.py); the host call tdlo_rig_self_occlusion_visible equals that statement on every scene and on 300 random self-crossing ropes under
random rigs, in sets and per-camera words; the K = 1 consequence holds against tdlo_self_occlusion_visible; five wrong readings of the statement are each told
from it by a scene; the lane runs over a whole (camera, frame) grid in a sanitized stand-alone program; the binding's marshalling is what the header lays down."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B
import rig_painter_ref as PR
import rig_painter_scenes as PS

NEW = ["tdlo_rig_self_occlusion_visible", "tdlo_rig_self_occlusion_batch", "tdlo_tracker_set_rig_self_occlusion"]


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def host(s):
    return B.rig_self_occlusion_visible(s.Y, s.cams, s.mats, s.rows, s.cols, s.w, s.dist, s.thr, words=True)


def test_the_new_names_are_declared_required_and_exported():
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_rig_painter_frame;" in hdr
    assert callable(B.rig_self_occlusion_visible) and callable(B.Context.rig_self_occlusion_batch) and callable(B.Context.rig_painter_route_counts)
    assert callable(B.trackdlo.set_rig_self_occlusion)
    # the struct as the C ABI lays it out
    f = B.RigPainterFrameC
    assert C.sizeof(f) == 56 and (f.M.offset, f.cams.offset, f.rig_to_cam.offset, f.K.offset, f.dlo_pixel_width.offset, f.node_dist.offset,
                                  f.visibility_threshold.offset) == (8, 16, 24, 32, 36, 40, 48)
    assert lib.tdlo_debug_route_count(None, 51) == -1 and lib.tdlo_debug_route_count(None, 52) == -1
    assert re.search(r"\* 51 / 52: \(camera, frame\) jobs of the self-occlusion test under a rig", text)
    # parity against OpenCV's rasteriser stays unpinned, and every document says so
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        t = open(os.path.join(ROOT, doc)).read()
        assert "tdlo_rig_self_occlusion" in t and re.search(r"under a rig[^\n]*unpinned|unpinned[^\n]*under a rig", t, flags=re.I), doc


@pytest.mark.parametrize("i", range(len(PS.scenes())), ids=[s[0].name for s in PS.scenes()])
def test_scene_property_and_host_call(i):
    s, vis, seen, hidden, per = PS.scenes()[i]
    if s.check:
        s.check(s, vis, seen, hidden, per)
    assert list(vis) == sorted(vis) and seen.shape == hidden.shape == (s.K, (s.M + 31) // 32)
    assert same(host(s), (vis, seen, hidden)), s.name


def test_batches_are_what_the_issue_asks_for():
    b = PS.batches()
    assert [len(v) for v in b.values()] == [1, 2, 33]
    many = [s for s, *_ in b["F=33"]]
    assert many[0].K == many[-1].K == 1 == min(s.K for s in many) and len({s.K for s in many}) > 2 and len({s.M for s in many}) > 10
    two = [s for s, *_ in b["F=2"]]
    assert two[0].K < two[1].K and two[0].M != two[1].M
    for group in b.values():
        for s, vis, seen, hidden, per in group:
            assert same(host(s), (vis, seen, hidden)), s.name


def test_host_call_on_300_random_ropes_under_random_rigs():
    rng = np.random.default_rng(5)
    hid = multi = 0
    for trial in range(300):
        s = PS.random_scene(rng)
        vis, seen, hidden, per = s.ref()
        assert same(host(s), (vis, seen, hidden)), trial
        near = int((s.dist <= s.thr).sum())
        hid += len(vis) < near
        alone = [set(PR.rig_verdict(s.Y, [s.cams[k]], None if s.mats is None else [s.mats[k]], s.rows, s.cols, s.w, s.dist, s.thr)[0]) for k in range(s.K)]
        assert set(vis) == set().union(*alone)                            # the rig sees what some camera alone sees
        multi += s.K > 1 and any(set(vis) != a for a in alone)
    assert hid > 100 and multi > 50


def test_one_camera_without_a_matrix_is_the_single_test():
    """K = 1, NULL matrix, every pixel inside the image: tdlo_self_occlusion_visible's set with the matrix built from the intrinsics."""
    rng = np.random.default_rng(6)
    cam = (400.0, 410.0, 320.0, 240.0)
    hid = 0
    for trial in range(300):
        M = int(rng.integers(1, 60))
        Y = PS.rope(rng, M); nd = rng.uniform(0, 0.016, M); w = int(rng.integers(1, 40))
        vis, seen, hidden = B.rig_self_occlusion_visible(Y, [cam], None, 480, 640, w, nd, 0.008, words=True)
        assert all((seen[0, m >> 5] >> (m & 31)) & 1 for m in range(M))
        single = B.self_occlusion_visible(Y, PR.proj_of(cam), w, nd, 0.008)
        assert np.array_equal(vis, single), trial
        hid += len(vis) < int((nd <= 0.008).sum())
    assert hid > 60


WRONG = {"no_image": "c third camera, one column out", "any": "a crossing, opposite sides", "rig_keys": "a crossing, opposite sides",
         "all_edges": "d z_c zero and negative", "fused": "k fused boundary"}


@pytest.mark.parametrize("variant", list(WRONG))
def test_a_wrong_reading_is_told_from_the_statement(variant):
    s, vis, seen, hidden, per = next(e for e in PS.scenes() if e[0].name == WRONG[variant])
    wrong = s.ref(variant)[:3]
    assert not same(wrong, (vis, seen, hidden))
    assert same(host(s), (vis, seen, hidden)) and not same(host(s), wrong)


def test_refusals_of_the_host_call():
    Y = np.array([[0.0, 0.0, 1.0], [0.1, 0.0, 1.0]]); d = np.zeros(2)
    ok = lambda **k: B.rig_self_occlusion_visible(**{**dict(Y=Y, cams=[PS.CAM], rig_to_cam=None, rows=480, cols=640, dlo_pixel_width=5, node_dist=d,
                                                            visibility_threshold=0.008), **k})
    assert list(ok()) == [0, 1]
    bad = [dict(dlo_pixel_width=0), dict(dlo_pixel_width=256), dict(rows=0), dict(rows=8193), dict(cols=0), dict(cols=8193), dict(cams=[]), dict(cams=[PS.CAM] * 65),
           dict(cams=[(0.0, 500.0, 1.0, 1.0)]), dict(cams=[(500.0, 0.0, 1.0, 1.0)]), dict(cams=[(np.inf, 500.0, 1.0, 1.0)]), dict(cams=[(500.0, 500.0, np.nan, 1.0)]),
           dict(rig_to_cam=[np.where(np.arange(12).reshape(3, 4) == 7, np.inf, PS.IDENT)]), dict(rig_to_cam=[np.where(np.arange(12).reshape(3, 4) == 0, np.nan, PS.IDENT)]),
           dict(Y=np.zeros((1025, 3)), node_dist=np.zeros(1025)), dict(Y=np.zeros((0, 3)), node_dist=np.zeros(0))]
    for k in bad:
        with pytest.raises(B.TdloError):
            ok(**k)
    assert list(ok(rig_to_cam=[None])) == [0, 1] and list(ok(cams=[PS.CAM] * 64)) == [0, 1] and list(ok(dlo_pixel_width=255, rows=8192, cols=8192)) == [0, 1]


def test_lane_over_a_job_grid_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/rig_painter_test.cpp with csrc/tdlo_painter_host.cpp: no HIP, built with -fsanitize=address,undefined (the runtime linked into the program) and
    run as a child process of its own.  Nothing sanitized is loaded into python."""
    exe = str(tmp_path / "rig_painter_test")
    csrc = os.path.join(ROOT, "trackdlo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "rig_painter_test.cpp"), os.path.join(csrc, "tdlo_painter_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"(\d+) jobs, 0 with a differing word, (\d+) hidden bits\n", r.stdout)
    assert m and int(m.group(1)) == 93 and int(m.group(2)) > 50, r.stdout


# ---- the binding's marshalling ----------------------------------------------------------------------------------------------------------------------
class StubLib:
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    def tdlo_rig_self_occlusion_batch(self, h, F, frames, rows, cols, vis, nv, seen, hidden):      # (the header's order)
        out = []
        Mmax = 0
        assert isinstance(F, int) and list(B.load_library().tdlo_rig_self_occlusion_batch.argtypes[:3]) == [C.c_void_p, C.c_int, C.c_void_p]
        tab =(B.RigPainterFrameC * F).from_address(addr(frames))
        for f in tab:
            cams = [(c.fx, c.fy, c.cx, c.cy, c.depth) for c in (B.RigCameraC * f.K).from_address(f.cams)]
            out.append(dict(M=f.M, K=f.K, w=f.dlo_pixel_width, thr=f.visibility_threshold, Y=arr(f.Y, 3 * f.M, C.c_double), cams=cams,
                            T=None if not f.rig_to_cam else arr(f.rig_to_cam, 12 * f.K, C.c_double), dist=arr(f.node_dist, f.M, C.c_double)))
            Mmax = max(Mmax, f.M)
        self.calls.append(dict(h=h, F=F, rows=rows, cols=cols, frames=out, words=bool(addr(seen)) and bool(addr(hidden))))
        iw = 0
        for i, f in enumerate(out):
            (C.c_int * 1).from_address(addr(nv) + 4 * i)[0] = 1
            (C.c_int * 1).from_address(addr(vis) + 4 * Mmax * i)[0] = f["M"] - 1
            n = f["K"] * ((f["M"] + 31) // 32)
            if addr(seen):
                for q in range(n):
                    (C.c_uint * 1).from_address(addr(seen) + 4 * (iw + q))[0] = 100 * i + q
                    (C.c_uint * 1).from_address(addr(hidden) + 4 * (iw + q))[0] = 1000 * i + q
            iw += n
        return self.rc

    def tdlo_tracker_set_rig_self_occlusion(self, t, T, K, w):
        self.calls.append(dict(t=addr(t), T=None if not addr(T) else arr(T, 12 * K, C.c_double), K=K, w=w))
        return self.rc

    def tdlo_debug_route_count(self, h, which):
        return 10 * which


def test_batch_marshalling():
    lib = StubLib()
    ctx = stub_context(lib)
    Y0 = np.arange(6.0).reshape(2, 3); Y1 = np.arange(120.0).reshape(40, 3)
    T = np.arange(12.0).reshape(3, 4)
    frames = [(Y0, [(1.0, 2.0, 3.0, 4.0)], None, 7, [0.5, 0.25], 0.3),
              (Y1, [(5.0, 6.0, 7.0, 8.0), B.RigCamera(np.zeros((2, 2), np.uint16), cam=(9.0, 10.0, 11.0, 12.0))], [None, T], 9, np.arange(40.0), 0.4)]
    vis, seen, hidden = ctx.rig_self_occlusion_batch(frames, 480, 640, words=True)
    k = lib.calls[-1]
    assert (k["h"], k["F"], k["rows"], k["cols"], k["words"]) == (0x1234, 2, 480, 640, True)
    f0, f1 = k["frames"]
    assert (f0["M"], f0["K"], f0["w"], f0["thr"]) == (2, 1, 7, 0.3) and (f1["M"], f1["K"], f1["w"], f1["thr"]) == (40, 2, 9, 0.4)
    assert f0["Y"] == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0]                          # column-major, as every call takes nodes
    assert f1["Y"][:40] == Y1[:, 0].tolist() and f1["Y"][80:] == Y1[:, 2].tolist()
    assert f0["cams"] == [(1.0, 2.0, 3.0, 4.0, None)] and f1["cams"] == [(5.0, 6.0, 7.0, 8.0, None), (9.0, 10.0, 11.0, 12.0, None)]      # the intrinsics alone
    assert f0["T"] is None and np.isnan(f1["T"][:12]).all() and f1["T"][12:] == T.reshape(-1).tolist()
    assert f0["dist"] == [0.5, 0.25] and f1["dist"] == list(np.arange(40.0))
    assert [v.tolist() for v in vis] == [[1], [39]]
    assert seen[0].tolist() == [[0]] and seen[1].tolist() == [[100, 101], [102, 103]] and hidden[1].tolist() == [[1000, 1001], [1002, 1003]]
    assert [v.tolist() for v in ctx.rig_self_occlusion_batch(frames, 8, 9)] == [[1], [39]] and lib.calls[-1]["words"] is False
    assert ctx.rig_painter_route_counts() == [510, 520]
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.rig_self_occlusion_batch(frames, 480, 640)
    with pytest.raises(ValueError):
        ctx.rig_self_occlusion_batch([(Y0, [(1.0, 2.0, 3.0, 4.0)], [None, None], 7, [0.5, 0.25], 0.3)], 480, 640)


def test_tracker_switch_marshalling():
    lib = StubLib()
    ctx = stub_context(lib)
    t = stub_tracker(ctx, 0x3000)
    patched_handles([t])
    T = np.arange(12.0).reshape(3, 4)
    t.set_rig_self_occlusion([None, T, None], 3, 11)
    k = lib.calls[-1]
    assert (k["t"], k["K"], k["w"]) == (0x3000, 3, 11) and np.isnan(k["T"][:12]).all() and k["T"][12:24] == T.reshape(-1).tolist() and np.isnan(k["T"][24:]).all()
    t.set_rig_self_occlusion(None, 2, 5)
    assert lib.calls[-1] == dict(t=0x3000, T=None, K=2, w=5)
    t.set_rig_self_occlusion(None, 0)
    assert lib.calls[-1] == dict(t=0x3000, T=None, K=0, w=0)
    t.h = None
