"""Cloud views without a GPU: the exported symbols, tdlo_cloud_view_check / _extent against tests/cloud_view_ref.py, binding.cloud_view on numpy arrays
and on a __cuda_array_interface__ stub, and the ctypes structure against the header's layout as a C++ compiler sees it (tests/cpp/view_test)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import cloud_view_ref as R

NEW = ["tdlo_cloud_view_check", "tdlo_cloud_view_extent", "tdlo_set_cloud_view", "tdlo_get_cloud", "tdlo_tracker_tracking_step_view"]


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    binding.load_library()
    return binding


def _view(B, data, dtype=0, location=0, sp=3, sc=1, stream=None, flags=0):
    return B.CloudView(data, dtype, location, sp, sc, stream, flags)


def test_the_library_exports_the_view_calls_without_a_gpu(B):
    lib = B.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in B.SYMBOLS, name


def test_view_check_accepts_and_refuses(B):
    lib = B.load_library()
    buf = np.zeros(64, dtype=np.float64)
    a = buf.ctypes.data
    ok = lambda v, N: lib.tdlo_cloud_view_check(C.byref(v), N)
    assert lib.tdlo_cloud_view_check(None, 4) == B.TDLO_E_INVALID                          # a null view
    assert ok(_view(B, None), 4) == B.TDLO_E_INVALID                                      # null data
    assert ok(_view(B, a), 0) == B.TDLO_E_INVALID and ok(_view(B, a), -3) == B.TDLO_E_INVALID
    assert ok(_view(B, a, dtype=2), 4) == B.TDLO_E_INVALID and ok(_view(B, a, dtype=-1), 4) == B.TDLO_E_INVALID
    assert ok(_view(B, a, location=3), 4) == B.TDLO_E_INVALID and ok(_view(B, a, location=-1), 4) == B.TDLO_E_INVALID
    assert ok(_view(B, a, flags=2), 4) == B.TDLO_E_INVALID and ok(_view(B, a, flags=3), 4) == B.TDLO_E_INVALID
    assert ok(_view(B, a, sp=0), 2) == B.TDLO_E_INVALID
    assert ok(_view(B, a, sp=0), 1) == 0                                                   # (one point: its stride addresses nothing)
    assert ok(_view(B, a, sc=0), 4) == B.TDLO_E_INVALID
    assert ok(_view(B, a + 2), 4) == B.TDLO_E_INVALID                                     # float32 at an odd half-word
    assert ok(_view(B, a + 4, dtype=B.F64), 4) == B.TDLO_E_INVALID and ok(_view(B, a + 4), 4) == 0
    for loc in (B.MEM_AUTO, B.MEM_HOST, B.MEM_DEVICE):
        for dt in (B.F32, B.F64):
            assert ok(_view(B, a, dtype=dt, location=loc, flags=B.VIEW_ASYNC, stream=0x1000), 5) == 0
    # negative strides are legal: a reversed numpy view is a cloud
    assert ok(_view(B, a + 64, sp=-3, sc=1), 4) == 0 and ok(_view(B, a + 64, sp=1, sc=-4), 4) == 0
    lo = C.c_longlong(0); hi = C.c_longlong(0)
    assert lib.tdlo_cloud_view_extent(C.byref(_view(B, a, sc=0)), 4, C.byref(lo), C.byref(hi)) == B.TDLO_E_INVALID
    assert lib.tdlo_cloud_view_extent(C.byref(_view(B, a)), 4, None, C.byref(hi)) == B.TDLO_E_INVALID


EXTENTS = [("packed", "f4", 3, 1, 1000), ("packed-f64", "f8", 3, 1, 257), ("xyz_", "f4", 4, 1, 77), ("xyzrgb", "f4", 8, 1, 77),
           ("columns-ld>N", "f4", 1, 1005, 1000), ("columns-f64", "f8", 1, 300, 257), ("reversed", "f4", -3, 1, 64), ("reversed-columns", "f8", 1, -70, 64),
           ("both-reversed", "f4", -8, -1, 5), ("one-point", "f4", 3, 1, 1), ("2^28", "f4", 1 << 28, 1, 3), ("-2^28", "f4", -(1 << 28), 1, 3)]


@pytest.mark.parametrize("name,dt,sp,sc,N", EXTENTS, ids=[e[0] for e in EXTENTS])
def test_view_extent_equals_the_numpy_statement(B, name, dt, sp, sc, N):
    base = 1 << 40                                     # (never dereferenced; an element-offset view is base + 4 * offset: data itself carries the offset)
    for off in (0, 7):
        v = _view(B, base + off * np.dtype(dt).itemsize, dtype=B.F32 if dt == "f4" else B.F64, sp=sp, sc=sc)
        v.N = N
        assert B.cloud_view_extent(v) == R.extent(dt, sp, sc, N)
    if name == "2^28":
        assert B.cloud_view_extent(v)[1] > 1 << 31     # 2 * 2^28 elements * 4 bytes and a point: past 2^31 bytes


def test_cloud_view_of_numpy_arrays(B):
    rng = np.random.default_rng(5)
    N = 37
    C32 = rng.standard_normal((N, 3)).astype(np.float32)
    wide = rng.standard_normal((N, 8)).astype(np.float32)
    cases = [C32, np.asfortranarray(C32), C32[::-1], wide[:, :3], wide, C32.astype(np.float64), np.asfortranarray(C32.astype(np.float64))[::-1], C32[3:N:2]]
    for X in cases:
        v = B.cloud_view(X)
        es = X.itemsize
        assert v.data == X.__array_interface__["data"][0] and v.N == X.shape[0] and v.owner is X
        assert (v.stride_point * es, v.stride_comp * es) == X.strides and v.dtype == (B.F32 if es == 4 else B.F64)
        assert v.location == B.MEM_HOST and v.flags == 0 and not v.ready_stream
        assert B.load_library().tdlo_cloud_view_check(C.byref(v), v.N) == 0
        # ... and the view addresses the array's own elements: the numpy statement over the underlying bytes gives the array back
        base = X if X.base is None else X.base
        while base.base is not None:
            base = base.base
        off = (v.data - base.__array_interface__["data"][0]) // es
        got = R.widen(np.lib.stride_tricks.as_strided(base.reshape(-1, order="A"), shape=(base.size,), strides=(es,)), X.dtype, off, v.stride_point, v.stride_comp, v.N)
        np.testing.assert_array_equal(got.view(np.uint64), np.asfortranarray(X[:, :3].astype(np.float64)).view(np.uint64))


def test_cloud_view_of_a_device_array_stub_and_refusals(B):
    class Dev:
        def __init__(self, shape, typestr, ptr, strides=None):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), strides=strides, version=3)

    v = B.cloud_view(Dev((100, 3), "<f4", 0x7f0000001000), ready_stream=0xabc0, asynchronous=True)
    assert (v.data, v.N, v.dtype, v.location, v.stride_point, v.stride_comp, v.ready_stream, v.flags) == (0x7f0000001000, 100, B.F32, B.MEM_DEVICE, 3, 1, 0xabc0, B.VIEW_ASYNC)
    v = B.cloud_view(Dev((100, 8), "<f8", 0x7f0000001000, strides=(8, 1600)))
    assert (v.dtype, v.stride_point, v.stride_comp, v.flags, v.ready_stream) == (B.F64, 1, 200, 0, None)
    for bad in (np.zeros((5, 3), dtype=np.float16), np.zeros((5, 3), dtype=np.int32), np.zeros((5, 2), dtype=np.float32), np.zeros(6, dtype=np.float32),
                np.zeros((5, 3), dtype=np.complex64), Dev((5, 3), "<f2", 0x1000), Dev((5, 3), "<i4", 0x1000), Dev((5, 2), "<f4", 0x1000), [[1.0, 2.0, 3.0]]):
        with pytest.raises(TypeError):
            B.cloud_view(bad)


def test_the_ctypes_structure_has_the_headers_layout(B):
    """tests/cpp/view_test --layout prints sizeof(tdlo_cloud_view) and offsetof of every field as the C++ compiler lays the header's struct out."""
    exe = os.path.join(ROOT, "tests", "cpp", "view_test")
    assert os.path.exists(exe), "tests/cpp/view_test is missing: run __graft_entry__.build() first"
    r = subprocess.run([exe, "--layout"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    want = dict(tok.split("=") for tok in r.stdout.split() if "=" in tok)
    assert int(want.pop("sizeof")) == C.sizeof(B.CloudView)
    assert set(want) == {n for n, _ in B.CloudView._fields_}
    for name, _ in B.CloudView._fields_:
        assert int(want[name]) == getattr(B.CloudView, name).offset, name
