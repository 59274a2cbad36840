"""Result images for many ropes, the part that needs no GPU: the declared interface, the host half (tdlo_render_batch_table) record for record against
tests/render_batch_ref.py, the statement itself told from three wrong readings of it, the kernel's per-lane code compiled for the host in a sanitized
stand-alone program, and the binding's marshalling against a stand-in library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_batch_cases as BC
import render_batch_ref as RB
import render_ref as R
from conftest import ROOT
from test_tracker_batch_cpu import StubLib, addr, arr, patched_handles, stub_context, stub_tracker
from trackdlo_amd import binding as B

NEW = ["tdlo_render_batch_table", "tdlo_render_result_batch", "tdlo_tracker_render_result_batch"]


def _lib_ropes(ropes):
    return [dict(r, params=B.make_render_params(**r["params"]) if r.get("params") else None) for r in ropes]


# ---- the interface ------------------------------------------------------------------------------------------------------------------------------------
def test_the_three_names_are_declared_listed_and_exported():
    lib = B.load_library()
    hdr = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    for name in NEW:
        assert name + "(" in hdr and name in B.SYMBOLS and hasattr(lib, name), name
    assert [f[0] for f in B.RenderImage._fields_] == ["colour", "occluder", "image_out"] and C.sizeof(B.RenderImage) == 24
    assert [f[0] for f in B.RenderRope._fields_] == ["image", "M", "Y", "proj", "vis", "n_vis", "params"] and C.sizeof(B.RenderRope) == 48
    assert lib.tdlo_debug_route_count(None, 34) == -1 and lib.tdlo_debug_route_count(None, 35) == -1
    assert lib.tdlo_abi_version() == 3


# ---- the host half ------------------------------------------------------------------------------------------------------------------------------------
def _random_list(rng):
    K = int(rng.integers(1, 5))
    n = int(rng.integers(1, 13))
    ropes = []
    for i in range(n):
        M = 1 if rng.random() < 0.15 else int(rng.integers(2, 41))
        prm = None if rng.random() < 0.5 else dict(line_width=int(rng.integers(1, 12)), node_radius=int(rng.integers(1, 12)), edge_visible=(1, i + 1, 3))
        ropes.append(BC.random_rope(rng, 60, 80, M, int(rng.integers(0, K)), prm))
    if K > 1 and rng.random() < 0.5:                    # an image without a rope
        skip = int(rng.integers(0, K))
        for r in ropes:
            if r["image"] == skip:
                r["image"] = (skip + 1) % K
    return ropes, K


def test_the_table_record_for_record():
    rng = np.random.default_rng(20240)
    seen_one_node = seen_empty_image = seen_unsorted = 0
    for trial in range(200):
        ropes, K = _random_list(rng)
        heads, prims, first = B.render_batch_table(_lib_ropes(ropes), K)
        wh, wp, wf = RB.table(ropes, K)
        assert np.array_equal(first, wf) and np.array_equal(prims, wp) and np.array_equal(heads, wh), trial
        # the head boxes once more, from the library's own primitive ranges
        order = sorted(range(len(ropes)), key=lambda i: (ropes[i]["image"], i))
        for j, i in enumerate(order):
            lo, n = int(heads[j, 4]), int(heads[j, 5])
            assert n == 3 * (len(ropes[i]["Y"]) - 1) and lo == sum(3 * (len(ropes[q]["Y"]) - 1) for q in order[:j])
            assert np.array_equal(prims[lo:lo + n], R.primitives(ropes[i]["Y"], ropes[i]["proj"], ropes[i]["vis"], ropes[i]["params"]))
            if n == 0:
                assert heads[j, :4].tolist() == [0, 0, -1, -1]; seen_one_node += 1
            else:
                b = np.array([RB.box(rec) for rec in prims[lo:lo + n]])
                assert heads[j, :4].tolist() == [b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()]
            assert heads[j, 6:].tolist() == [0, 0]
        for k in range(K):
            assert [ropes[i]["image"] for i in order[first[k]:first[k + 1]]] == [k] * (first[k + 1] - first[k])
            seen_empty_image += first[k] == first[k + 1]
        seen_unsorted += order != list(range(len(ropes)))
    assert seen_one_node > 20 and seen_empty_image > 20 and seen_unsorted > 100


def _raw_table(ropes, K, cap=None, R_=None):
    """tdlo_render_batch_table on poisoned outputs: (rc, outputs untouched?)."""
    tab, Rn, keep = B._render_ropes(_lib_ropes(ropes))
    Rn = Rn if R_ is None else R_
    heads = np.full((max(Rn, 1), 8), -77, dtype=np.int32); prims = np.full((4096, 8), -77, dtype=np.int32); first = np.full(300, -77, dtype=np.int32)
    n = C.c_int(-77)
    rc = B.load_library().tdlo_render_batch_table(C.cast(tab, C.c_void_p), Rn, K, heads.ctypes.data, prims.ctypes.data, 4096 if cap is None else cap,
                                                  C.byref(n), first.ctypes.data)
    return rc, bool(np.all(heads == -77) and np.all(prims == -77) and np.all(first == -77) and n.value == -77)


def test_the_table_refuses_with_its_outputs_untouched():
    good = [BC.rope([(5, 5), (20, 9), (30, 30)], 0), BC.rope([(7, 40), (50, 12)], 1)]
    assert _raw_table(good, 2) == (0, False)
    bad = {
        "image below 0": [good[0], dict(good[1], image=-1)],
        "image beyond K - 1": [good[0], dict(good[1], image=2)],
        "vis out of range": [good[0], dict(good[1], vis=np.array([2], dtype=np.int32))],
        "width 0": [dict(good[0], params=dict(line_width=0)), good[1]],
        "radius 256": [good[0], dict(good[1], params=dict(node_radius=256))],
        "a node behind the camera": [good[0], dict(good[1], Y=np.asfortranarray(good[1]["Y"] * np.array([1.0, 1.0, -1.0])))],
        "a pixel beyond 8192": [dict(good[0], Y=np.asfortranarray(R.nodes_from_pixels([(5, 5), (9000, 9)], BC.K.FX))), good[1]],
    }
    for name, ropes in bad.items():
        assert _raw_table(ropes, 2) == (B.TDLO_E_INVALID, True), name
        with pytest.raises(ValueError):
            RB.render_batch(BC.images(2, 48, 64, 1), ropes, 48, 64)
    assert _raw_table(good, 0) == (B.TDLO_E_INVALID, True) and _raw_table(good, 257) == (B.TDLO_E_INVALID, True)
    assert _raw_table(good, 2, cap=8) == (B.TDLO_E_INVALID, True)                 # 9 records do not fit
    assert _raw_table(good, 2, R_=1025) == (B.TDLO_E_INVALID, True) and _raw_table(good, 2, R_=-1) == (B.TDLO_E_INVALID, True)
    assert _raw_table([], 3)[0] == 0                                               # no rope at all is a table
    with pytest.raises(B.TdloError):
        B.render_batch_table(_lib_ropes(bad["vis out of range"]), 2)


# ---- the statement ------------------------------------------------------------------------------------------------------------------------------------
def _crossing_pair():
    """Two ropes that cross each other (and the second itself) on a 64 x 72 image with an occluder of mixed bytes; the rope listed FIRST is nearer."""
    a = BC.rope([(6, 10), (60, 50), (64, 8)], 0, [0, 1], [0.80, 0.85, 0.90], dict(edge_visible=(10, 20, 30), node_visible=(40, 50, 60)))
    b = BC.rope([(8, 52), (56, 12), (30, 30), (8, 8), (66, 58)], 0, [1, 2], [1.40, 1.30, 1.50, 1.20, 1.60], dict(edge_visible=(200, 210, 220), node_hidden=(90, 91, 92)))
    return BC.images(1, 64, 72, 3, [True]), [a, b]


def test_list_order_decides_and_one_rope_is_the_single_statement():
    imgs, (a, b) = _crossing_pair()
    ab, cor = RB.render_batch(imgs, [a, b], 64, 72)
    ba, _ = RB.render_batch(imgs, [b, a], 64, 72)
    assert not np.array_equal(ab[0], ba[0])
    for first, second, got in ((a, b, ab[0]), (b, a, ba[0])):
        want = R.blend(imgs[0]["colour"], imgs[0]["occluder"])
        R.paint(want, R.primitives(first["Y"], first["proj"], first["vis"], first["params"]))
        R.paint(want, R.primitives(second["Y"], second["proj"], second["vis"], second["params"]))
        assert np.array_equal(got, want)
    assert cor == [R.corners(imgs[0]["occluder"])]
    # one rope per image, shuffled image fields, an image without a rope
    imgs3 = BC.images(3, 64, 72, 9)
    out, cors = RB.render_batch(imgs3, [dict(b, image=2), dict(a, image=0)], 64, 72)
    for k, r in ((0, a), (2, b)):
        w, wc = R.render(imgs3[k]["colour"], imgs3[k]["occluder"], r["Y"], r["proj"], r["vis"], r["params"])
        assert np.array_equal(out[k], w) and cors[k] == wc
    assert np.array_equal(out[1], R.blend(imgs3[1]["colour"], imgs3[1]["occluder"])) and cors[1] == [-1] * 4


def test_three_wrong_readings_are_told_from_the_statement():
    imgs, ropes = _crossing_pair()
    colour, occ = imgs[0]["colour"], imgs[0]["occluder"]
    want = RB.render_batch(imgs, ropes, 64, 72)[0][0]
    prims = [R.primitives(r["Y"], r["proj"], r["vis"], r["params"]) for r in ropes]
    # 1. the blend once per rope (what successive single calls over their own output give)
    img = colour.copy()
    for p in prims:
        img = R.paint(R.blend(img, occ), p)
    assert not np.array_equal(img, want)
    # 2. every rope's edges merged into one global farthest-first order
    keyed = []
    for r, p in zip(ropes, prims):
        Y = np.asarray(r["Y"]); m = (Y[:-1] + Y[1:]) / 2
        key = np.sqrt((m * m).sum(axis=1))
        for slot, e in enumerate(R.edge_order(Y)):
            keyed.append((key[e], p[3 * slot:3 * slot + 3]))
    merged = np.concatenate([t for _, t in sorted(keyed, key=lambda kt: -kt[0])])
    assert not np.array_equal(R.paint(R.blend(colour, occ), merged), want)
    # 3. the first covering primitive instead of the last
    assert not np.array_equal(R.paint(R.blend(colour, occ), np.concatenate(prims)[::-1]), want)


# ---- the per-lane code of the kernel, on the host -----------------------------------------------------------------------------------------------------
def test_the_search_header_in_a_sanitized_stand_alone_program(tmp_path):
    """csrc/tdlo_render_search.h (the loads, the two-level search, the blend and the stores of k_render_batch) built into tests/cpp/render_batch_host_test.cpp
    with -fsanitize=address,undefined and run as a child process of its own (nothing preloaded): images of 1 x 1, 1 x 3, 7 x 9, 33 x 65 and 64 x 64 and
    tables at exactly their sizes, every byte against a literal blend-then-paint loop."""
    exe = str(tmp_path / "render_batch_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "cpp", "render_batch_host_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "30 pictures, 0 differing bytes" in r.stdout, r.stdout


# ---- the binding's marshalling ------------------------------------------------------------------------------------------------------------------------
class RenderStub(StubLib):
    def _images(self, tab, K):
        return [(x.colour or 0, x.occluder or 0, x.image_out or 0) for x in (B.RenderImage * K).from_address(addr(tab))]

    def tdlo_last_colour_shape(self, h, rows, cols):
        rows._obj.value = 6; cols._obj.value = 8
        return 0

    def tdlo_debug_route_count(self, h, which):
        return 100 + which

    def tdlo_render_result_batch(self, h, images, K, rows, cols, ropes, R_, corners):
        rp = []
        for x in (B.RenderRope * R_).from_address(addr(ropes)) if R_ else []:
            prm = B.RenderParams.from_address(x.params) if x.params else None
            rp.append(dict(image=x.image, M=x.M, Y=arr(x.Y, 3 * x.M, C.c_double), proj=arr(x.proj, 12, C.c_double), vis=arr(x.vis, x.n_vis, C.c_int), n_vis=x.n_vis,
                           params=None if prm is None else (prm.line_width, prm.node_radius, list(prm.edge_visible))))
        self.calls.append(dict(h=h, K=K, rows=rows, cols=cols, R=R_, images=self._images(images, K), ropes=rp, corners=addr(corners)))
        if addr(corners):
            (C.c_int * (4 * K)).from_address(addr(corners))[:] = list(range(4 * K))
        return self.rc

    def tdlo_tracker_render_result_batch(self, tab, F, images, K, rows, cols, image_of, proj, params, corners):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, K=K, rows=rows, cols=cols, images=self._images(images, K), image_of=arr(image_of, F, C.c_int),
                               proj=None if not addr(proj) else [None if not p else arr(p, 12, C.c_double) for p in arr(proj, F, C.c_void_p)],
                               params=None if not addr(params) else [None if not p else B.RenderParams.from_address(p).line_width for p in arr(params, F, C.c_void_p)],
                               corners=addr(corners)))
        return self.rc


def test_render_result_batch_marshalling():
    lib = RenderStub()
    ctx = stub_context(lib)
    rows, cols = 6, 8
    colour = [np.full((rows, cols, 3), 10 + k, dtype=np.uint8) for k in range(2)]
    occ = np.zeros((rows, cols), dtype=np.uint8)
    out1 = np.zeros((rows, cols, 3), dtype=np.uint8)
    prm = B.RenderParams(); prm.line_width = 9; prm.node_radius = 4; prm.edge_visible[:] = [1, 2, 3]
    Y = np.arange(12, dtype=np.float64).reshape(4, 3)
    ropes = [dict(image=1, Y=Y, proj=np.arange(12.0), vis=[0, 3], params=prm), dict(image=0, Y=Y[:1], proj=np.ones(12), vis=[], params=None)]
    outs, cor = ctx.render_result_batch([dict(colour=colour[0], occluder=occ), dict(colour=colour[1], out=out1)], ropes)
    c = lib.calls[-1]
    assert (c["h"], c["K"], c["rows"], c["cols"], c["R"]) == (0x1234, 2, rows, cols, 2)
    assert c["images"][0][:2] == (colour[0].ctypes.data, occ.ctypes.data) and c["images"][0][2] == outs[0].ctypes.data
    assert c["images"][1] == (colour[1].ctypes.data, 0, out1.ctypes.data) and outs[1] is out1
    assert c["ropes"][0] == dict(image=1, M=4, Y=Y.T.reshape(-1).tolist(), proj=list(np.arange(12.0)), vis=[0, 3], n_vis=2, params=(9, 4, [1, 2, 3]))
    assert c["ropes"][1]["M"] == 1 and c["ropes"][1]["n_vis"] == 0 and c["ropes"][1]["params"] is None
    assert cor == [[0, 1, 2, 3], [4, 5, 6, 7]]
    # colour None: the context's last colour frame, its shape asked of the library; no ropes; no corners
    outs, cor = ctx.render_result_batch([dict()], [], corners=False)
    c = lib.calls[-1]
    assert c["images"][0][:2] == (0, 0) and (c["rows"], c["cols"], c["R"], c["corners"]) == (6, 8, 0, 0) and cor is None and outs[0].shape == (6, 8, 3)
    assert ctx.render_batch_route_counts() == [134, 135]
    # a plane or an output of the wrong shape never reaches the library
    n = len(lib.calls)
    for im in (dict(colour=colour[0][:, :7]), dict(colour=colour[0], occluder=occ[:5]), dict(colour=colour[0], out=np.zeros((rows, cols, 4), dtype=np.uint8)),
               dict(colour=colour[0], out=np.zeros((rows, cols, 3), dtype=np.float32))):
        with pytest.raises(ValueError):
            ctx.render_result_batch([dict(colour=colour[0]), im], ropes, shape=(rows, cols))
    with pytest.raises(ValueError):
        ctx.render_result_batch([dict(colour=colour[0])], [dict(ropes[0], Y=np.zeros((4, 2)))])
    assert len(lib.calls) == n
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.render_result_batch([dict(colour=colour[0])], ropes[1:])


def test_tracker_render_result_batch_marshalling():
    lib = RenderStub()
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    try:
        rows, cols = 5, 7
        colour = np.zeros((rows, cols, 3), dtype=np.uint8)
        imgs = [dict(colour=colour), dict(colour=colour.copy())]
        outs, cor = B.render_result_batch(trk, imgs, [1, 0, 1])
        c = lib.calls[-1]
        assert c["trackers"] == [0x3000, 0x3001, 0x3002] and (c["F"], c["K"], c["rows"], c["cols"]) == (3, 2, rows, cols)
        assert c["image_of"] == [1, 0, 1] and c["proj"] is None and c["params"] is None and c["corners"] != 0
        assert [i[2] for i in c["images"]] == [o.ctypes.data for o in outs] and cor == [[0] * 4, [0] * 4]
        prm = B.RenderParams(); prm.line_width = 3
        B.render_result_batch(trk, imgs, [0, 0, 0], proj=[None, np.arange(12.0), None], params=[prm, None, None], corners=False)
        c = lib.calls[-1]
        assert c["proj"] == [None, list(np.arange(12.0)), None] and c["params"] == [3, None, None] and c["corners"] == 0
        n = len(lib.calls)
        with pytest.raises(ValueError):
            B.render_result_batch(trk, [dict(colour=colour), dict(colour=colour[:4])], [0, 1, 0])
        assert len(lib.calls) == n
        lib.rc = B.TDLO_E_INVALID
        assert B.render_result_batch(trk, imgs, [1, 0, 1], check=False)[2] == B.TDLO_E_INVALID
        with pytest.raises(B.TdloError):
            B.render_result_batch(trk, imgs, [1, 0, 1])
    finally:
        for t in trk:
            t.h = None
