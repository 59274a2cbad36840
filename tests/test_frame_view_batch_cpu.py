"""tdlo_frame_views_to_cloud_batch / tdlo_tracker_frame_views_batch / tdlo_view_batch_images without a GPU: the names are declared, required and exported,
the binding marshals images (views where they lie, host or device), frames, image_of and per-frame colour ranges as the header lays them down -- checked
against a stand-in library, as tests/test_cloud_batch_cpu.py does for the packed batch -- the calls refuse a null context and bad arguments, and the lane
under k_image_import_batch's table (csrc/tdlo_image_lane.h, the code the GPU runs) is run over a whole grid in a stand-alone program built with
-fsanitize=address,undefined (tests/cpp/image_batch_lane_host_test.cpp).  No sanitizer on code loaded into python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import image_view_ref as R
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B

NEW = ["tdlo_frame_views_to_cloud_batch", "tdlo_tracker_frame_views_batch", "tdlo_view_batch_images"]


def test_the_new_names_are_declared_required_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_view_image;" in hdr
    assert "#define TDLO_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr)
    for name in ("frame_views_to_cloud_batch", "view_batch_images", "frame_view_batch_route_counts"):
        assert callable(getattr(B.Context, name))
    assert callable(B.frame_views_batch)
    # tdlo_view_image as the C ABI lays it out: a tdlo_frame_view (four views of 32 bytes) and four doubles
    assert [f[0] for f in B.ViewImage._fields_] == ["fv", "fx", "fy", "cx", "cy"]
    assert C.sizeof(B.ViewImage) == C.sizeof(B.FrameView) + 32 == 160 and B.ViewImage.fx.offset == 128
    # the route counters: -1 for a null context, whatever the index
    assert all(lib.tdlo_debug_route_count(None, k) == -1 for k in (42, 43, 44, 45))


def test_the_struct_layout_against_a_compiler(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "trackdlo_hip.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tdlo_view_image), offsetof(tdlo_view_image, fv), offsetof(tdlo_view_image, fx), '
                   'offsetof(tdlo_view_image, fy), offsetof(tdlo_view_image, cx), offsetof(tdlo_view_image, cy)); return 0; }\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    V = B.ViewImage
    assert got == [C.sizeof(V), V.fv.offset, V.fx.offset, V.fy.offset, V.cx.offset, V.cy.offset]


def test_null_context_and_bad_arguments_without_a_device():
    lib = B.load_library()
    d = np.zeros((2, 4), np.uint16); m = np.ones((2, 4), np.uint8)
    tab, K, rows, cols, keep = B._view_images([dict(depth=d, mask=m, cam=(1.0, 1.0, 0.0, 0.0))])
    fr = (B.BatchFrame * 1)(); fr[0].slot, fr[0].image = 0, 0
    n = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert (K, rows, cols) == (1, 2, 4)
    assert lib.tdlo_frame_views_to_cloud_batch(None, C.cast(tab, C.c_void_p), K, rows, cols, C.cast(fr, C.c_void_p), 1, 0.008, p(n), p(n), None) == B.TDLO_E_INVALID
    assert lib.tdlo_tracker_frame_views_batch(None, 1, C.cast(tab, C.c_void_p), K, rows, cols, p(n), None, 0.008, 0.06, None, None, None, None, None, None, None, None) \
        == B.TDLO_E_INVALID
    assert lib.tdlo_tracker_frame_views_batch(None, 0, None, 0, 0, 0, None, None, 0.008, 0.06, None, None, None, None, None, None, None, None) == B.TDLO_E_INVALID
    q = [C.c_void_p(7) for _ in range(4)]
    assert lib.tdlo_view_batch_images(None, 0, C.byref(q[0]), C.byref(q[1]), C.byref(q[2]), C.byref(q[3])) == B.TDLO_E_INVALID
    assert lib.tdlo_view_batch_images(None, -1, None, None, None, None) == B.TDLO_E_INVALID
    assert [v.value for v in q] == [7, 7, 7, 7]                  # (a refused call writes nothing)


class StubLib:
    """Records what the binding hands to the three entry points and fills the outputs like the library would."""
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    @staticmethod
    def _images(images, K):
        out = []
        for im in (B.ViewImage * K).from_address(addr(images)):
            d = dict(cam=(im.fx, im.fy, im.cx, im.cy))
            for name in ("depth", "colour", "occluder", "mask"):
                v = getattr(im.fv, name)
                d[name] = None if not v.data else (v.data, v.format, v.location, v.row_stride, v.ready_stream)
            out.append(d)
        return out

    @staticmethod
    def _params(p):
        if not p:
            return None
        cp = B.ColourParams.from_address(p)
        return (cp.n_ranges, [list(cp.lower[k]) for k in range(cp.n_ranges)], [list(cp.upper[k]) for k in range(cp.n_ranges)], cp.rgb_order)

    def tdlo_frame_views_to_cloud_batch(self, h, images, K, rows, cols, frames, F, leaf, n, nraw, rcs):
        fr = [(f.slot, f.image, self._params(f.colour_params)) for f in (B.BatchFrame * F).from_address(addr(frames))] if F else []
        self.calls.append(dict(h=h, K=K, rows=rows, cols=cols, F=F, leaf=leaf, images=self._images(images, K), frames=fr))
        for i in range(F):
            (C.c_int * 1).from_address(addr(n) + 4 * i)[0] = 10 + i
            (C.c_int * 1).from_address(addr(nraw) + 4 * i)[0] = 100 + i
        if F:
            (C.c_int * 1).from_address(addr(rcs) + 4 * (F - 1))[0] = self.rc
        return self.rc

    def tdlo_tracker_frame_views_batch(self, tab, F, images, K, rows, cols, image_of, cps, leaf, d_vis, vis, nv, ext, ne, n, nraw, stats, rcs):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, K=K, rows=rows, cols=cols, leaf=leaf, d_vis=d_vis, images=self._images(images, K),
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

    def tdlo_view_batch_images(self, h, k, depth, colour, occluder, mask):
        self.calls.append(dict(h=h, k=k))
        if self.rc:
            return self.rc
        for p, v in ((depth, 0x1000 + k), (colour, 0x2000 + k), (occluder, None), (mask, 0x4000 + k)):
            C.cast(p, C.POINTER(C.c_void_p))[0] = v
        return 0


@pytest.fixture
def lib():
    return StubLib()


class FakeDeviceImage:
    """An object with __cuda_array_interface__ (what image_view() takes for device memory): RGBA8 rows behind a pitch, at a made-up address."""
    def __init__(self, address, rows, cols, channels, typestr, pitch):
        es = int(typestr[2:])
        shape = (rows, cols, channels) if channels > 1 else (rows, cols)
        strides = (pitch, channels * es, es)[:len(shape)]
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(address, False), strides=strides, version=3)


def test_frame_views_to_cloud_batch_marshalling(lib):
    ctx = stub_context(lib)
    rows, cols = 3, 8
    rng = np.random.default_rng(4)
    d16 = rng.integers(0, 65536, (rows, cols + 2)).astype(np.uint16)[:, 1:1 + cols]          # pitched host depth, data 2 bytes into the buffer
    bgr = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)[::-1]                        # bottom-up host colour
    occ = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    mask = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    rgba = FakeDeviceImage(0x7f0000001000, rows, cols, 4, "|u1", 4 * cols + 16)
    metres = FakeDeviceImage(0x7f0000002000, rows, cols, 1, "<f4", 4 * cols)
    images = [dict(depth=d16, colour=bgr, occluder=occ, mask=mask, cam=(600.0, 601.0, 2.5, 1.5)),
              dict(depth=B.image_view(metres, ready_stream=0xbeef), colour=rgba, cam=(1.0, 2.0, 3.0, 4.0)),
              dict(depth=d16, mask=mask, cam=(5.0, 6.0, 7.0, 8.0))]
    blue = B.make_colour_params()
    two = B.make_colour_params([[0, 60, 50], [15, 100, 80]], [[10, 255, 255], [40, 255, 255]], rgb_order=1)
    n, nraw, codes = ctx.frame_views_to_cloud_batch(images, [(5, 0, None), (0, 0, blue), (3, 1, two), (2, 2, None)], 0.008)
    c = lib.calls[-1]
    assert (c["h"], c["K"], c["rows"], c["cols"], c["F"], c["leaf"]) == (0x1234, 3, rows, cols, 4, 0.008)
    i0, i1, i2 = c["images"]
    assert i0["cam"] == (600.0, 601.0, 2.5, 1.5) and i1["cam"] == (1.0, 2.0, 3.0, 4.0) and i2["cam"] == (5.0, 6.0, 7.0, 8.0)
    assert i0["depth"] == (d16.ctypes.data, B.IMG_U16C1, B.MEM_HOST, 2 * (cols + 2), None)
    assert i0["colour"] == (bgr.ctypes.data, B.IMG_U8C3, B.MEM_HOST, -3 * cols, None)
    assert i0["occluder"] == (occ.ctypes.data, B.IMG_U8C1, B.MEM_HOST, cols, None) and i0["mask"] == (mask.ctypes.data, B.IMG_U8C1, B.MEM_HOST, cols, None)
    assert i1["depth"] == (0x7f0000002000, B.IMG_F32C1, B.MEM_DEVICE, 4 * cols, 0xbeef)
    assert i1["colour"] == (0x7f0000001000, B.IMG_U8C4, B.MEM_DEVICE, 4 * cols + 16, None) and i1["mask"] is None and i1["occluder"] is None
    assert i2["colour"] is None and i2["depth"] == i0["depth"] and i2["mask"] == i0["mask"]
    f = c["frames"]
    assert [(s, i) for s, i, _ in f] == [(5, 0), (0, 0), (3, 1), (2, 2)]
    assert f[0][2] is None and f[3][2] is None
    assert f[1][2] == (1, [[90, 90, 30]], [[130, 255, 255]], 0)
    assert f[2][2] == (2, [[0, 60, 50], [15, 100, 80]], [[10, 255, 255], [40, 255, 255]], 1)
    assert (n, nraw, codes) == ([10, 11, 12, 13], [100, 101, 102, 103], [0, 0, 0, 0])
    # a ready-made FrameView is taken as it is
    fv = B.frame_view(d16, mask=mask)
    ctx.frame_views_to_cloud_batch([dict(fv=fv, cam=(1, 1, 0, 0))], [(0, 0, None)], 0.008)
    assert lib.calls[-1]["images"][0]["depth"] == i0["depth"] and lib.calls[-1]["images"][0]["colour"] is None
    # a per-frame code: returned with check=False, raised otherwise
    lib.rc = B.TDLO_E_INVALID
    assert ctx.frame_views_to_cloud_batch(images, [(0, 0, None)], 0.008, check=False)[2] == [B.TDLO_E_INVALID]
    with pytest.raises(B.TdloError):
        ctx.frame_views_to_cloud_batch(images, [(0, 0, None)], 0.008)
    # images of two shapes never reach the library
    ncalls = len(lib.calls)
    with pytest.raises(ValueError):
        ctx.frame_views_to_cloud_batch([images[0], dict(depth=np.zeros((rows, cols + 1), np.uint16), mask=np.zeros((rows, cols + 1), np.uint8), cam=(1, 1, 0, 0))],
                                       [(0, 0, None)], 0.008)
    assert len(lib.calls) == ncalls


def test_view_batch_images_marshalling(lib):
    ctx = stub_context(lib)
    assert ctx.view_batch_images(3) == dict(depth=0x1003, colour=0x2003, occluder=None, mask=0x4003)
    assert lib.calls[-1] == dict(h=0x1234, k=3)
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.view_batch_images(0)
    # a canonical plane in the shape the render batch takes a tensor
    pl = B.DevicePlane(0x2003, (4, 6, 3))
    assert B._batch_plane(pl, np.uint8, (4, 6, 3), "colour") == (0x2003, pl)
    with pytest.raises(ValueError):
        B._batch_plane(pl, np.uint8, (4, 6), "occluder")


def test_frame_views_batch_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    rows, cols = 2, 4
    rng = np.random.default_rng(6)
    d = rng.integers(0, 65536, (rows, cols)).astype(np.uint16); m = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    rgba = rng.integers(0, 256, (rows, cols, 4)).astype(np.uint8)
    images = [dict(depth=d, mask=m, colour=rgba, cam=(615.0, 615.0, 2.0, 1.0))]
    red = B.make_colour_params([[0, 60, 50]], [[10, 255, 255]])
    codes, vis, ext, n, nraw = B.frame_views_batch(trk, images, [0, 0, 0], [None, red, None], 0.008, 0.06)
    c = lib.calls[-1]
    assert c["trackers"] == [0x3000, 0x3001, 0x3002] and (c["F"], c["K"], c["rows"], c["cols"], c["leaf"], c["d_vis"]) == (3, 1, rows, cols, 0.008, 0.06)
    assert c["image_of"] == [0, 0, 0] and c["params"] == [None, (1, [[0, 60, 50]], [[10, 255, 255]], 0), None]
    assert c["images"][0]["depth"] == (d.ctypes.data, B.IMG_U16C1, B.MEM_HOST, 2 * cols, None)
    assert c["images"][0]["colour"] == (rgba.ctypes.data, B.IMG_U8C4, B.MEM_HOST, 4 * cols, None) and c["images"][0]["occluder"] is None
    assert codes == [0, 0, 0] and [v.tolist() for v in vis] == [[0], [1], [2]] and [e.tolist() for e in ext] == [[0, 1], [1, 2], [2, 3]]
    assert n == [50, 51, 52] and nraw == [500, 501, 502]
    assert [s["iters"] for s in trk[2].last_stats] == [304, 305]
    B.frame_views_batch(trk, images, [0, 0, 0], None, 0.008, 0.06)
    assert lib.calls[-1]["params"] is None
    lib.rc = B.TDLO_E_EMPTY
    assert B.frame_views_batch(trk, images, [0, 0, 0], None, 0.008, 0.06, check=False)[0] == [0, 0, B.TDLO_E_EMPTY]
    with pytest.raises(B.TdloError):
        B.frame_views_batch(trk, images, [0, 0, 0], None, 0.008, 0.06)
    for t in trk:
        t.h = None           # (nothing for __del__ to destroy)


# ---- the lane under the table, on the host ---------------------------------------------------------------------------------------------------------
def _pick(lays, name):
    return next(l for l in lays if l[0] == name)


def _table(rows, cols, rng):
    """A K = 3 table whose images differ in their forms: [(format, role, layout)] per job.  At a width that is a multiple of 4 job 0 is all wide loads, job 1
    dword loads (data offset 4), job 2 element by element (data offset 1 / 2, odd pitches, bottom-up rows); at any other width every view is element by
    element and the pitched and bottom-up layouts are what differs."""
    L = {f: R.layouts(rows, cols, f, rng) for f in (R.U8C1, R.U8C3, R.U8C4, R.U16C1, R.F32C1)}
    return [
        [(R.F32C1, R.DEPTH, _pick(L[R.F32C1], "pitch+16")), (R.U8C4, R.COLOUR, _pick(L[R.U8C4], "off0")), (R.U8C1, R.OCCLUDER, _pick(L[R.U8C1], "pitch+4")),
         (R.U8C1, R.MASK, _pick(L[R.U8C1], "off8"))],
        [(R.U16C1, R.DEPTH, _pick(L[R.U16C1], "off4")), (R.U8C4, R.COLOUR, _pick(L[R.U8C4], "off4")), (R.U8C1, R.MASK, _pick(L[R.U8C1], "bottom-up-pitch+16"))],
        [(R.U16C1, R.DEPTH, _pick(L[R.U16C1], "off-and-pitch")), (R.U8C3, R.COLOUR, _pick(L[R.U8C3], "pitch+1")), (R.U8C1, R.OCCLUDER, _pick(L[R.U8C1], "off1")),
         (R.U8C1, R.MASK, _pick(L[R.U8C1], "bottom-up"))],
    ]


@pytest.fixture(scope="module")
def lane_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lane") / "image_batch_lane_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "image_batch_lane_host_test.cpp"), os.path.join(ROOT, "trackdlo_amd", "csrc", "tdlo_image_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (5, 7), (32, 32), (2, 514), (6, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_workgroup_and_lane_of_a_table_of_three_images(tmp_path, lane_program, shape):
    """Every (workgroup y, lane) of a K = 3 table, sources allocated at exactly their extents, destinations between canary bytes: no report from the
    sanitizers, the bytes of image_pack_host (compared in the program) and of the numpy statement (compared here).  Shapes: image tails of 1, 3 and 3 pixels;
    1 024 pixels = exactly one workgroup of lanes; 1 028 = one lane into a second; 6 x 8 for the vector forms at a small size."""
    rows, cols = shape
    table = _table(rows, cols, np.random.default_rng(100 * rows + cols))
    blob = [np.array([len(table), rows, cols], dtype=np.int64).tobytes()]
    want = []
    forms = [0, 0, 0]
    for job in table:
        blob.append(np.array([len(job)], dtype=np.int64).tobytes())
        for fmt, role, (name, buf, off, stride) in job:
            lo, hi = R.extent(fmt, stride, rows, cols)
            lead = off + lo
            assert lead in (0, 1, 2, 4, 8) and buf.size == off + hi
            forms[R.form(lead - lo, stride, cols, fmt)] += 1           # (the program's source blocks are 16-byte aligned: data = block + lead - lo)
            blob.append(np.array([fmt, role, stride, lead, lo, hi, 0, 0], dtype=np.int64).tobytes())
            blob.append(buf[lead:].tobytes())
            want.append((name, R.canonical(buf, off, fmt, stride, rows, cols).tobytes()))
    (tmp_path / "table.bin").write_bytes(b"".join(blob))
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([lane_program, str(tmp_path / "table.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    groups = ((rows * cols + 3) // 4 + 255) // 256
    assert f"3 jobs imported over a grid of {groups} x 3 workgroups" in r.stdout, r.stdout
    said = [int(x) for x in r.stdout.split(":")[-1].split()]
    assert said == forms, (said, forms)
    if cols % 4 == 0:
        assert min(said) >= 2, said                               # all three forms in one table
    else:
        assert said[1:] == [0, 0]
    got = (tmp_path / "out.bin").read_bytes()
    assert len(got) == sum(len(w) for _, w in want)
    at = 0
    for name, w in want:
        assert got[at:at + len(w)] == w, name
        at += len(w)
