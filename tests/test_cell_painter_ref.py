"""The painter test over a cell of ropes without a GPU: the scenes of tests/cell_painter_scenes.py assert their own properties on the numpy / integer
statement (tests/cell_painter_ref.py); the host call tdlo_cell_occlusion_visible equals that statement on every scene, on the batches' cells, on the largest
cell and on 150 random cells, in sets and per-camera words; F = 1 gives tdlo_rig_self_occlusion_visible's bits on the scenes of tests/rig_painter_scenes.py;
permuting the ropes permutes the verdict where no keys tie; five wrong readings of the statement are each told from it by a scene; every refusal leaves every
output untouched; the lane runs over a whole (node block, camera, edge tile) grid in a sanitized stand-alone program; the binding's marshalling is what the
header lays down."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B
import cell_painter_scenes as CS
import rig_painter_scenes as PS

NEW = ["tdlo_cell_occlusion_visible", "tdlo_cell_occlusion_batch", "tdlo_tracker_frames_from_shared_cloud_occluded_batch"]


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[0], want[0])) and len(got[0]) == len(want[0]) and np.array_equal(got[1], want[1]) \
        and np.array_equal(got[2], want[2])


def host(s):
    return B.cell_occlusion_visible(s.ropes, s.cams, s.mats, s.rows, s.cols, s.w, words=True)


def test_the_new_names_are_declared_required_and_exported():
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    for t in ("tdlo_cell_rope;", "tdlo_cell;", "tdlo_cell_view;"):
        assert t in hdr
    assert callable(B.cell_occlusion_visible) and callable(B.Context.cell_occlusion_batch) and callable(B.Context.cell_painter_route_counts)
    assert callable(B.frames_from_shared_cloud_occluded_batch)
    # the structs as the C ABI lays them out
    r, c, v = B.CellRopeC, B.CellC, B.CellViewC
    assert C.sizeof(r) == 32 and (r.M.offset, r.node_dist.offset, r.visibility_threshold.offset) == (8, 16, 24)
    assert C.sizeof(c) == 40 and (c.F.offset, c.cams.offset, c.rig_to_cam.offset, c.K.offset, c.dlo_pixel_width.offset) == (8, 16, 24, 32, 36)
    assert C.sizeof(v) == 32 and (v.rig_to_cam.offset, v.K.offset, v.rows.offset, v.cols.offset, v.dlo_pixel_width.offset) == (8, 16, 20, 24, 28)
    assert lib.tdlo_debug_route_count(None, 57) == -1 and lib.tdlo_debug_route_count(None, 58) == -1
    assert re.search(r"\* 57 / 58: \(camera, cell\) jobs of the painter test over a cell of ropes", text)
    assert "one rope hiding ANOTHER" not in text
    for doc in ("README.md", "DESIGN.md"):
        assert "tdlo_cell_occlusion" in open(os.path.join(ROOT, doc)).read(), doc


@pytest.mark.parametrize("i", range(len(CS.scenes())), ids=[s[0].name for s in CS.scenes()])
def test_scene_property_and_host_call(i):
    s, vis, seen, hidden, per = CS.scenes()[i]
    s.check(s, vis, seen, hidden, per)
    assert all(list(v) == sorted(v) for v in vis) and seen.shape == hidden.shape == (s.K, (s.N + 31) // 32)
    assert same(host(s), (vis, seen, hidden)), s.name


def test_largest_cell_property_and_host_call():
    s, vis, seen, hidden, per = CS.largest()
    s.check(s, vis, seen, hidden, per)
    assert same(host(s), (vis, seen, hidden))


def test_batches_are_what_the_issue_asks_for():
    b = CS.batches()
    assert [len(v) for v in b.values()] == [1, 2, 33]
    many = [s for s, *_ in b["C=33"]]
    assert len({s.K for s in many}) > 2 and len({s.N for s in many}) > 10 and len({s.F for s in many}) > 2
    two = [s for s, *_ in b["C=2"]]
    assert two[0].K != two[1].K and two[0].N != two[1].N and two[0].F != two[1].F
    for group in b.values():
        for s, vis, seen, hidden, per in group:
            assert same(host(s), (vis, seen, hidden)), s.name


def test_host_call_on_150_random_cells():
    rng = np.random.default_rng(15)
    other = 0
    for trial in range(150):
        s = CS.random_cell(rng)
        vis, seen, hidden, per = s.ref()
        assert same(host(s), (vis, seen, hidden)), trial
        other += not same(s.ref("own_only")[:3], (vis, seen, hidden))
    assert other > 60                                   # in most cells a rope hides a node of another


def test_one_rope_is_the_test_under_a_rig():
    """Consequence (a): F = 1 gives the set and the words of tdlo_rig_self_occlusion_visible, bit for bit."""
    for s, vis, seen, hidden, per in PS.scenes():
        got = B.cell_occlusion_visible([(s.Y, s.dist, s.thr)], s.cams, s.mats, s.rows, s.cols, s.w, words=True)
        rig = B.rig_self_occlusion_visible(s.Y, s.cams, s.mats, s.rows, s.cols, s.w, s.dist, s.thr, words=True)
        assert np.array_equal(got[0][0], rig[0]) and np.array_equal(got[1], rig[1]) and np.array_equal(got[2], rig[2]), s.name
        assert np.array_equal(got[0][0], vis) and np.array_equal(got[1], seen) and np.array_equal(got[2], hidden), s.name


def test_permuting_the_ropes_changes_a_verdict_only_through_ties():
    """Consequence (b)."""
    rng = np.random.default_rng(16)
    for trial in range(40):
        s = CS.random_cell(rng, F=4)
        order = list(rng.permutation(4))
        a, b = host(s)[0], host(s.permuted(order))[0]
        assert all(np.array_equal(b[i], a[f]) for i, f in enumerate(order)), trial      # (random keys do not tie)
    tie = next(e for e in CS.scenes() if e[0].name == "mirror tie")
    flip = next(e for e in CS.scenes() if e[0].name == "mirror tie, permuted")
    (A1, B1), (B2, A2) = tie[1], flip[1]                                                     # (A's node 0 lies outside the image in both)
    assert list(A1) == [1, 2, 3, 4, 5] and list(B1) == [0, 2] and list(B2) == [0, 1, 2] and list(A2) == [1, 2, 3, 5]


WRONG = {"phantom_edge": "no phantom edge", "own_only": "crossing", "local_tie": "mirror tie", "any_first": "crossing, depths swapped", "no_order": "tiny ropes"}


@pytest.mark.parametrize("variant", list(WRONG))
def test_a_wrong_reading_is_told_from_the_statement(variant):
    s, vis, seen, hidden, per = next(e for e in CS.scenes() if e[0].name == WRONG[variant])
    wrong = s.ref(variant)[:3]
    assert not same(wrong, (vis, seen, hidden))
    assert same(host(s), (vis, seen, hidden)) and not same(host(s), wrong)


def raw_host(ropes, cams, mats, rows, cols, w, null=()):
    """tdlo_cell_occlusion_visible on outputs filled with a pattern: (code, whether every output is as it was)."""
    lib = B.load_library()
    rt, F, N, Ms, keep = B._cell_ropes(ropes)
    tab, K = B._painter_cams(cams)
    T = B._painter_matrices(mats, K)
    v = [np.full(max(M, 1), -7, dtype=np.int32) for M in Ms]
    pv = (C.c_void_p * max(F, 1))(*[x.ctypes.data for x in v])
    nv = np.full(max(F, 1), -7, dtype=np.int32)
    W = (max(N, 1) + 31) // 32
    seen = np.full((max(K, 1), W), 0xABCD, dtype=np.uint32); hidden = np.full_like(seen, 0xABCD)
    if "Y" in null:
        rt[F - 1].Y = None
    if "dist" in null:
        rt[F - 1].node_dist = None
    rc = lib.tdlo_cell_occlusion_visible(None if "ropes" in null else C.cast(rt, C.c_void_p), F, None if "cams" in null else C.cast(tab, C.c_void_p), B._ptr(T), K,
                                         int(rows), int(cols), int(w), None if "vis" in null else C.cast(pv, C.c_void_p), None if "nv" in null else B._ptr(nv),
                                         B._ptr(seen), B._ptr(hidden))
    return rc, all((x == -7).all() for x in v) and (nv == -7).all() and (seen == 0xABCD).all() and (hidden == 0xABCD).all()


def test_refusals_leave_every_output_untouched():
    Y = np.array([[0.0, 0.0, 1.0], [0.1, 0.0, 1.0]]); d = np.zeros(2)
    base = dict(ropes=[(Y, d, 0.008), (Y + 0.01, d, 0.008)], cams=[PS.CAM], mats=None, rows=480, cols=640, w=5)
    assert raw_host(**base) == (0, False)
    big = np.zeros((1024, 3)); big[:, 2] = 1.0
    bad = [dict(w=0), dict(w=256), dict(rows=0), dict(rows=8193), dict(cols=0), dict(cols=8193), dict(cams=[]), dict(cams=[PS.CAM] * 65),
           dict(cams=[(0.0, 500.0, 1.0, 1.0)]), dict(cams=[(500.0, 0.0, 1.0, 1.0)]), dict(cams=[(np.inf, 500.0, 1.0, 1.0)]), dict(cams=[(500.0, 500.0, np.nan, 1.0)]),
           dict(mats=[np.where(np.arange(12).reshape(3, 4) == 7, np.inf, PS.IDENT)]), dict(mats=[np.where(np.arange(12).reshape(3, 4) == 0, np.nan, PS.IDENT)]),
           dict(ropes=[]), dict(ropes=[(Y, d, 0.008), (np.zeros((1025, 3)), np.zeros(1025), 0.008)]), dict(ropes=[(Y, d, 0.008), (np.zeros((0, 3)), np.zeros(0), 0.008)]),
           dict(ropes=[(big, np.zeros(1024), 0.008)] * 16 + [(Y[:1], d[:1], 0.008)]),      # N = 16 385
           dict(null=("Y", )), dict(null=("dist", )), dict(null=("ropes", )), dict(null=("cams", )), dict(null=("vis", )), dict(null=("nv", ))]
    for k in bad:
        assert raw_host(**{**base, **k}) == (B.TDLO_E_INVALID, True), k
    ok = [dict(mats=[None]), dict(cams=[PS.CAM] * 64), dict(w=255, rows=8192, cols=8192), dict(ropes=[(Y[:1], d[:1], 0.008)])]
    for k in ok:
        assert raw_host(**{**base, **k}) == (0, False), k


def cells_file(path, cells):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cells)))
        for s in cells:
            f.write(struct.pack("<5i", s.F, s.K, s.rows, s.cols, s.w))
            f.write(np.array(s.Ms, dtype="<i4").tobytes())
            f.write(np.array(s.cams, dtype="<f8").tobytes())
            T = np.full((s.K, 12), np.nan) if s.mats is None else B._painter_matrices(s.mats, s.K)
            f.write(T.astype("<f8").tobytes())
            for Y, _, _ in s.ropes:
                f.write(np.asfortranarray(Y).astype("<f8").tobytes(order="F"))


def fnv(h, a):
    for b in np.ascontiguousarray(a, dtype="<u4").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_lane_over_a_job_grid_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/cell_painter_lane_host_test.cpp with csrc/tdlo_cell_painter_host.cpp and csrc/tdlo_painter_host.cpp: no HIP, built with
    -fsanitize=address,undefined (the runtime linked into the program) and run as a child process of its own.  Nothing sanitized is loaded into python.
    The program's hash over all words is the reference's."""
    exe = str(tmp_path / "cell_painter_lane_host_test")
    csrc = os.path.join(ROOT, "trackdlo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "cell_painter_lane_host_test.cpp"),
                        os.path.join(csrc, "tdlo_cell_painter_host.cpp"), os.path.join(csrc, "tdlo_painter_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    group = [e for e in CS.scenes() if e[0].name != "many cameras"] + CS.batches()["C=33"][:12]      # block boundaries: 557 nodes, three node blocks, two edge tiles
    cells_file(str(tmp_path / "cells.bin"), [e[0] for e in group])
    r = subprocess.run([exe, str(tmp_path / "cells.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"(\d+) jobs, 0 with a differing word, (\d+) hidden bits, hash ([0-9a-f]{16})\n", r.stdout)
    assert m, r.stdout
    h = 1469598103934665603
    bits = 0
    for s, vis, seen, hidden, per in group:
        h = fnv(fnv(h, seen), hidden)
        bits += sum(len(CS.hidden_set(c)) for c in per)
    assert int(m.group(1)) == sum(e[0].K for e in group) and int(m.group(2)) == bits > 400 and int(m.group(3), 16) == h


# ---- the binding's marshalling ----------------------------------------------------------------------------------------------------------------------
class StubLib:
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    def tdlo_cell_occlusion_batch(self, h, Cn, cells, rows, cols, vis, nv, seen, hidden):      # (the header's order)
        assert isinstance(Cn, int) and list(B.load_library().tdlo_cell_occlusion_batch.argtypes[:3]) == [C.c_void_p, C.c_int, C.c_void_p]
        out = []
        for q in (B.CellC * Cn).from_address(addr(cells)):
            ropes = [dict(M=r.M, thr=r.visibility_threshold, Y=arr(r.Y, 3 * r.M, C.c_double), dist=arr(r.node_dist, r.M, C.c_double))
                     for r in (B.CellRopeC * q.F).from_address(q.ropes)]
            cams = [(c.fx, c.fy, c.cx, c.cy, c.depth) for c in (B.RigCameraC * q.K).from_address(q.cams)]
            out.append(dict(F=q.F, K=q.K, w=q.dlo_pixel_width, ropes=ropes, cams=cams, T=None if not q.rig_to_cam else arr(q.rig_to_cam, 12 * q.K, C.c_double)))
        self.calls.append(dict(h=h, C=Cn, rows=rows, cols=cols, cells=out, words=bool(addr(seen)) and bool(addr(hidden))))
        Mmax = max(r["M"] for q in out for r in q["ropes"])
        row = iw = 0
        for i, q in enumerate(out):
            for r in q["ropes"]:
                (C.c_int * 1).from_address(addr(nv) + 4 * row)[0] = 1
                (C.c_int * 1).from_address(addr(vis) + 4 * Mmax * row)[0] = r["M"] - 1
                row += 1
            n = q["K"] * ((sum(r["M"] for r in q["ropes"]) + 31) // 32)
            if addr(seen):
                for j in range(n):
                    (C.c_uint * 1).from_address(addr(seen) + 4 * (iw + j))[0] = 100 * i + j
                    (C.c_uint * 1).from_address(addr(hidden) + 4 * (iw + j))[0] = 1000 * i + j
            iw += n
        return self.rc

    def tdlo_tracker_frames_from_shared_cloud_occluded_batch(self, tr, F, src, d_max, d_vis, view, vis, nv, ext, ne, n_each, st, rcs):
        v = B.CellViewC.from_address(addr(view))
        cams = [(c.fx, c.fy, c.cx, c.cy) for c in (B.RigCameraC * v.K).from_address(v.cams)]
        self.calls.append(dict(trackers=arr(tr, F, C.c_void_p), F=F, src=src, d_max=d_max, d_vis=d_vis, K=v.K, rows=v.rows, cols=v.cols, w=v.dlo_pixel_width, cams=cams,
                               T=None if not v.rig_to_cam else arr(v.rig_to_cam, 12 * v.K, C.c_double)))
        M = 4
        for i in range(F):
            (C.c_int * 1).from_address(addr(nv) + 4 * i)[0] = 1
            (C.c_int * 1).from_address(addr(ne) + 4 * i)[0] = 2
            (C.c_int * 1).from_address(addr(vis) + 4 * M * i)[0] = i
            (C.c_int * 2).from_address(addr(ext) + 4 * M * i)[:] = [i, i + 1]
            (C.c_int * 1).from_address(addr(n_each) + 4 * i)[0] = 10 + i
        return self.rc

    def tdlo_debug_route_count(self, h, which):
        return 10 * which


def test_batch_marshalling():
    lib = StubLib()
    ctx = stub_context(lib)
    Y0 = np.arange(6.0).reshape(2, 3); Y1 = np.arange(120.0).reshape(40, 3); Y2 = np.arange(9.0).reshape(3, 3)
    T = np.arange(12.0).reshape(3, 4)
    cells = [([(Y0, [0.5, 0.25], 0.3)], [(1.0, 2.0, 3.0, 4.0)], None, 7),
             ([(Y1, np.arange(40.0), 0.4), (Y2, [1.0, 2.0, 3.0], 0.5)], [(5.0, 6.0, 7.0, 8.0), B.RigCamera(np.zeros((2, 2), np.uint16), cam=(9.0, 10.0, 11.0, 12.0))], [None, T], 9)]
    vis, seen, hidden = ctx.cell_occlusion_batch(cells, 480, 640, words=True)
    k = lib.calls[-1]
    assert (k["h"], k["C"], k["rows"], k["cols"], k["words"]) == (0x1234, 2, 480, 640, True)
    c0, c1 = k["cells"]
    assert (c0["F"], c0["K"], c0["w"]) == (1, 1, 7) and (c1["F"], c1["K"], c1["w"]) == (2, 2, 9)
    assert c0["ropes"][0]["Y"] == [0.0, 3.0, 1.0, 4.0, 2.0, 5.0] and c0["ropes"][0]["dist"] == [0.5, 0.25] and c0["ropes"][0]["thr"] == 0.3      # column-major
    assert c1["ropes"][0]["Y"][:40] == Y1[:, 0].tolist() and c1["ropes"][0]["Y"][80:] == Y1[:, 2].tolist() and [r["M"] for r in c1["ropes"]] == [40, 3]
    assert c1["ropes"][1]["dist"] == [1.0, 2.0, 3.0] and c1["ropes"][1]["thr"] == 0.5
    assert c0["cams"] == [(1.0, 2.0, 3.0, 4.0, None)] and c1["cams"] == [(5.0, 6.0, 7.0, 8.0, None), (9.0, 10.0, 11.0, 12.0, None)]
    assert c0["T"] is None and np.isnan(c1["T"][:12]).all() and c1["T"][12:] == T.reshape(-1).tolist()
    assert [[v.tolist() for v in c] for c in vis] == [[[1]], [[39], [2]]]
    assert seen[0].tolist() == [[0]] and seen[1].tolist() == [[100, 101], [102, 103]] and hidden[1].tolist() == [[1000, 1001], [1002, 1003]]
    assert [[v.tolist() for v in c] for c in ctx.cell_occlusion_batch(cells, 8, 9)] == [[[1]], [[39], [2]]] and lib.calls[-1]["words"] is False
    assert ctx.cell_painter_route_counts() == [570, 580]
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.cell_occlusion_batch(cells, 480, 640)
    with pytest.raises(ValueError):
        ctx.cell_occlusion_batch([([(Y0, [0.5, 0.25], 0.3)], [(1.0, 2.0, 3.0, 4.0)], [None, None], 7)], 480, 640)


def test_tracker_call_marshalling():
    lib = StubLib()
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x2000 + i) for i in range(3)]
    patched_handles(trk)
    T = np.arange(12.0).reshape(3, 4)
    codes, vis, ext, n_each = B.frames_from_shared_cloud_occluded_batch(trk, 5, 0.05, 0.03, [(1.0, 2.0, 3.0, 4.0), (5.0, 6.0, 7.0, 8.0)], [T, None], 480, 640, 11)
    k = lib.calls[-1]
    assert k["trackers"] == [0x2000, 0x2001, 0x2002] and (k["F"], k["src"], k["d_max"], k["d_vis"]) == (3, 5, 0.05, 0.03)
    assert (k["K"], k["rows"], k["cols"], k["w"]) == (2, 480, 640, 11) and k["cams"] == [(1.0, 2.0, 3.0, 4.0), (5.0, 6.0, 7.0, 8.0)]
    assert k["T"][:12] == T.reshape(-1).tolist() and np.isnan(k["T"][12:]).all()
    assert codes == [0, 0, 0] and [v.tolist() for v in vis] == [[0], [1], [2]] and [v.tolist() for v in ext] == [[0, 1], [1, 2], [2, 3]] and n_each == [10, 11, 12]
    B.frames_from_shared_cloud_occluded_batch(trk, 5, 0.05, 0.03, [(1.0, 2.0, 3.0, 4.0)], None, 8, 9, 3)
    assert lib.calls[-1]["T"] is None and lib.calls[-1]["K"] == 1
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        B.frames_from_shared_cloud_occluded_batch(trk, 5, 0.05, 0.03, [(1.0, 2.0, 3.0, 4.0)], None, 8, 9, 3)
    for t in trk:
        t.h = None
