"""tdlo_depth_to_cloud_batch / tdlo_tracker_frames_batch without a GPU: the names are declared, required and exported, and the binding's marshalling of
images, frames, image_of and per-frame colour ranges is what the header lays down -- checked against a stand-in library, as tests/test_tracker_batch_cpu.py
does for the tracker batch calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B

NEW = ["tdlo_depth_to_cloud_batch", "tdlo_tracker_frames_batch"]


def test_the_new_names_are_declared_required_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_batch_image;" in hdr and "tdlo_batch_frame;" in hdr
    assert "#define TDLO_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    for name in ("depth_to_cloud_batch", "cloud_batch_route_counts"):
        assert callable(getattr(B.Context, name))
    assert callable(B.frames_batch)
    # the two structs as the C ABI lays them out: four pointers + four doubles; {int, int, pointer}
    assert [f[0] for f in B.BatchImage._fields_] == ["depth", "mask", "colour", "occluder", "fx", "fy", "cx", "cy"] and C.sizeof(B.BatchImage) == 64
    assert [f[0] for f in B.BatchFrame._fields_] == ["slot", "image", "colour_params"] and C.sizeof(B.BatchFrame) == 16
    # the route counters exist on any context: -1 only for an unknown counter (no GPU: a null context answers -1 for all of them)
    assert lib.tdlo_debug_route_count(None, 32) == -1


class StubLib:
    """Records what the binding hands to the two entry points and fills the outputs like the library would."""
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    @staticmethod
    def _images(images, K, rows, cols):
        out = []
        for im in (B.BatchImage * K).from_address(addr(images)):
            d = dict(cam=(im.fx, im.fy, im.cx, im.cy))
            for name, ct, n in (("depth", C.c_uint16, rows * cols), ("mask", C.c_uint8, rows * cols), ("colour", C.c_uint8, 3 * rows * cols),
                                ("occluder", C.c_uint8, rows * cols)):
                p = getattr(im, name)
                d[name] = None if not p else arr(p, n, ct)
            out.append(d)
        return out

    @staticmethod
    def _params(p):
        if not p:
            return None
        cp = B.ColourParams.from_address(p)
        return (cp.n_ranges, [list(cp.lower[k]) for k in range(cp.n_ranges)], [list(cp.upper[k]) for k in range(cp.n_ranges)], cp.rgb_order)

    def tdlo_depth_to_cloud_batch(self, h, images, K, rows, cols, frames, F, leaf, n, nraw, rcs):
        fr = [(f.slot, f.image, self._params(f.colour_params)) for f in (B.BatchFrame * F).from_address(addr(frames))] if F else []
        self.calls.append(dict(h=h, K=K, rows=rows, cols=cols, F=F, leaf=leaf, images=self._images(images, K, rows, cols), frames=fr))
        for i in range(F):
            (C.c_int * 1).from_address(addr(n) + 4 * i)[0] = 10 + i
            (C.c_int * 1).from_address(addr(nraw) + 4 * i)[0] = 100 + i
        if F:
            (C.c_int * 1).from_address(addr(rcs) + 4 * (F - 1))[0] = self.rc
        return self.rc

    def tdlo_tracker_frames_batch(self, tab, F, images, K, rows, cols, image_of, cps, leaf, d_vis, vis, nv, ext, ne, n, nraw, stats, rcs):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, K=K, rows=rows, cols=cols, leaf=leaf, d_vis=d_vis, images=self._images(images, K, rows, cols),
                               image_of=arr(image_of, F, C.c_int), params=None if not addr(cps) else [self._params(p) for p in arr(cps, F, C.c_void_p)]))
        M = 4
        for i in range(F):
            (C.c_int * 1).from_address(addr(nv) + 4 * i)[0] = 1
            (C.c_int * 1).from_address(addr(ne) + 4 * i)[0] = 2
            (C.c_int * M).from_address(addr(vis) + 4 * M * i)[0] = i
            e = (C.c_int * M).from_address(addr(ext) + 4 * M * i); e[0] = i; e[1] = i + 1
            (C.c_int * 1).from_address(addr(n) + 4 * i)[0] = 50 + i
            (C.c_int * 1).from_address(addr(nraw) + 4 * i)[0] = 500 + i
        st = (B.Stats * (2 * F)).from_address(addr(stats))
        for i in range(2 * F):
            st[i].iters = 300 + i
        (C.c_int * F).from_address(addr(rcs))[F - 1] = self.rc
        return self.rc


@pytest.fixture
def lib():
    return StubLib()


def planes(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 65536, (rows, cols)).astype(np.uint16), rng.integers(0, 256, (rows, cols)).astype(np.uint8),
            rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8), rng.integers(0, 256, (rows, cols)).astype(np.uint8))


def test_depth_to_cloud_batch_marshalling(lib):
    ctx = stub_context(lib)
    rows, cols = 3, 5
    d0, m0, c0, o0 = planes(rows, cols, 1)
    d1, m1, c1, _ = planes(rows, cols, 2)
    images = [dict(depth=d0, mask=m0, colour=c0, occluder=o0, cam=(600.0, 601.0, 2.5, 1.5)), dict(depth=d1, colour=c1, cam=(1.0, 2.0, 3.0, 4.0)),
              dict(depth=d1.astype(np.int64), mask=m1, cam=(5.0, 6.0, 7.0, 8.0))]           # (another dtype: converted to uint16)
    blue = B.make_colour_params()
    two = B.make_colour_params([[0, 60, 50], [15, 100, 80]], [[10, 255, 255], [40, 255, 255]], rgb_order=1)
    n, nraw, codes = ctx.depth_to_cloud_batch(images, [(5, 0, None), (0, 0, blue), (3, 1, two), (2, 2, None)], 0.008)
    c = lib.calls[-1]
    assert (c["h"], c["K"], c["rows"], c["cols"], c["F"], c["leaf"]) == (0x1234, 3, rows, cols, 4, 0.008)
    i0, i1, i2 = c["images"]
    assert i0["cam"] == (600.0, 601.0, 2.5, 1.5) and i0["depth"] == d0.reshape(-1).tolist() and i0["mask"] == m0.reshape(-1).tolist()
    assert i0["colour"] == c0.reshape(-1).tolist() and i0["occluder"] == o0.reshape(-1).tolist()
    assert i1["mask"] is None and i1["occluder"] is None and i1["colour"] == c1.reshape(-1).tolist() and i1["cam"] == (1.0, 2.0, 3.0, 4.0)
    assert i2["colour"] is None and i2["depth"] == d1.reshape(-1).tolist() and i2["mask"] == m1.reshape(-1).tolist()
    f = c["frames"]
    assert [(s, i) for s, i, _ in f] == [(5, 0), (0, 0), (3, 1), (2, 2)]
    assert f[0][2] is None and f[3][2] is None
    assert f[1][2] == (1, [[90, 90, 30]], [[130, 255, 255]], 0)
    assert f[2][2] == (2, [[0, 60, 50], [15, 100, 80]], [[10, 255, 255], [40, 255, 255]], 1)
    assert (n, nraw, codes) == ([10, 11, 12, 13], [100, 101, 102, 103], [0, 0, 0, 0])
    # a per-frame code: returned with check=False, raised otherwise
    lib.rc = B.TDLO_E_INVALID
    assert ctx.depth_to_cloud_batch(images, [(0, 0, None)], 0.008, check=False)[2] == [B.TDLO_E_INVALID]
    with pytest.raises(B.TdloError):
        ctx.depth_to_cloud_batch(images, [(0, 0, None)], 0.008)
    # a plane of the wrong shape never reaches the library
    ncalls = len(lib.calls)
    with pytest.raises(ValueError):
        ctx.depth_to_cloud_batch([dict(depth=d0, mask=m0[:, :4], cam=(1, 1, 0, 0))], [(0, 0, None)], 0.008)
    assert len(lib.calls) == ncalls


def test_frames_batch_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    rows, cols = 2, 4
    d0, m0, c0, o0 = planes(rows, cols, 3)
    images = [dict(depth=d0, mask=m0, colour=c0, occluder=o0, cam=(615.0, 615.0, 2.0, 1.0))]
    red = B.make_colour_params([[0, 60, 50]], [[10, 255, 255]])
    codes, vis, ext, n, nraw = B.frames_batch(trk, images, [0, 0, 0], [None, red, None], 0.008, 0.06)
    c = lib.calls[-1]
    assert c["trackers"] == [0x3000, 0x3001, 0x3002] and (c["F"], c["K"], c["rows"], c["cols"], c["leaf"], c["d_vis"]) == (3, 1, rows, cols, 0.008, 0.06)
    assert c["image_of"] == [0, 0, 0] and c["params"] == [None, (1, [[0, 60, 50]], [[10, 255, 255]], 0), None]
    assert c["images"][0]["depth"] == d0.reshape(-1).tolist() and c["images"][0]["occluder"] == o0.reshape(-1).tolist()
    assert codes == [0, 0, 0] and [v.tolist() for v in vis] == [[0], [1], [2]] and [e.tolist() for e in ext] == [[0, 1], [1, 2], [2, 3]]
    assert n == [50, 51, 52] and nraw == [500, 501, 502]
    assert [s["iters"] for s in trk[2].last_stats] == [304, 305]
    # no colour ranges at all: NULL for the table
    B.frames_batch(trk, images, [0, 0, 0], None, 0.008, 0.06)
    assert lib.calls[-1]["params"] is None
    lib.rc = B.TDLO_E_EMPTY
    assert B.frames_batch(trk, images, [0, 0, 0], None, 0.008, 0.06, check=False)[0] == [0, 0, B.TDLO_E_EMPTY]
    with pytest.raises(B.TdloError):
        B.frames_batch(trk, images, [0, 0, 0], None, 0.008, 0.06)
    for t in trk:
        t.h = None           # (nothing for __del__ to destroy)
