"""The binding's marshalling for the calls of "starting ropes of one colour", checked without a GPU against a stand-in library (as tests/test_assign_cpu.py
does): the destination table, NULL for outputs nobody asked for, the argument order of the header, the counts handed back."""
import ctypes as C

import numpy as np
import pytest

from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B


class StubLib:
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    def tdlo_get_cloud(self, h, slot, X, cap, n):
        n._obj.value = 5
        return 0

    def tdlo_debug_route_count(self, h, which):
        return 100 + which

    def tdlo_cloud_cluster(self, h, src, dst, F, tol, min_size, n_clusters, n_each, n_un, owner):      # (the header's order)
        self.calls.append(dict(h=h, src=src, F=F, tol=tol, min_size=min_size, dst=arr(dst, F, C.c_int), owner=addr(owner)))
        n_clusters._obj.value = 7
        for f in range(F):
            (C.c_int * 1).from_address(addr(n_each) + 4 * f)[0] = 2 + f
        n_un._obj.value = 1
        if addr(owner):
            (C.c_int * 5).from_address(addr(owner))[4] = -1
        return self.rc

    def tdlo_cloud_cluster_host(self, X, n, F, tol, min_size, owner, n_clusters, n_each, n_un):
        self.calls.append(dict(X=arr(X, 3 * n, C.c_double), n=n, F=F, tol=tol, min_size=min_size))
        (C.c_int * n).from_address(addr(owner))[n - 1] = 1
        n_clusters._obj.value = 2
        (C.c_int * F).from_address(addr(n_each))[F - 1] = 9
        n_un._obj.value = 3
        return self.rc

    def tdlo_tracker_initialize_from_shared_cloud_batch(self, tab, F, src, tol, min_size, mu, max_iter, s2, n_clusters, n_each, rcs):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, src=src, tol=tol, min_size=min_size, mu=mu, max_iter=max_iter))
        n_clusters._obj.value = F + (1 if self.rc else 0)
        for i in range(F):
            (C.c_double * 1).from_address(addr(s2) + 8 * i)[0] = 0.5 + i
            (C.c_int * 1).from_address(addr(n_each) + 4 * i)[0] = 70 + i
        (C.c_int * F).from_address(addr(rcs))[F - 1] = self.rc
        return self.rc


@pytest.fixture
def lib():
    return StubLib()


def test_argtypes_are_the_header_s():
    L = B.load_library()
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    assert list(L.tdlo_cloud_cluster.argtypes[:6]) == [vp, ci, vp, ci, cd, ci] and len(L.tdlo_cloud_cluster.argtypes) == 10
    assert list(L.tdlo_cloud_cluster_host.argtypes[:5]) == [vp, ci, ci, cd, ci] and len(L.tdlo_cloud_cluster_host.argtypes) == 9
    assert list(L.tdlo_tracker_initialize_from_shared_cloud_batch.argtypes[:7]) == [vp, ci, ci, cd, ci, cd, ci]
    assert len(L.tdlo_tracker_initialize_from_shared_cloud_batch.argtypes) == 11


def test_cloud_cluster_marshalling(lib):
    ctx = stub_context(lib)
    assert ctx.cloud_cluster(3, [2, 0, 1], 0.015, 4) == (7, [2, 3, 4], 1)
    k = lib.calls[-1]
    assert (k["h"], k["src"], k["F"], k["tol"], k["min_size"], k["dst"], k["owner"]) == (0x1234, 3, 3, 0.015, 4, [2, 0, 1], 0)
    nc, n_each, un, own = ctx.cloud_cluster(3, [1], 0.02, 1, owners=True)
    assert lib.calls[-1]["owner"] != 0 and own.shape == (5,) and own.dtype == np.int32 and own[4] == -1 and n_each == [2]
    assert ctx.cluster_route_counts() == [155, 156]
    lib.rc = B.TDLO_E_INVALID
    assert ctx.cloud_cluster(3, [1], 0.02, 1, check=False)[0] == B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.cloud_cluster(3, [1], 0.02, 1)


def test_cloud_cluster_host_marshalling(lib):
    X = np.arange(12.0).reshape(4, 3)
    own, nc, n_each, un = B.cloud_cluster_host(X, 2, 0.03, 5, lib=lib)
    k = lib.calls[-1]
    assert (k["n"], k["F"], k["tol"], k["min_size"]) == (4, 2, 0.03, 5) and k["X"] == X.T.reshape(-1).tolist()      # column-major n x 3
    assert own.tolist() == [0, 0, 0, 1] and nc == 2 and n_each == [0, 9] and un == 3
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        B.cloud_cluster_host(X, 2, 0.03, 5, lib=lib)


def test_tracker_entrance_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    codes, s2, nc, n_each = B.initialize_from_shared_cloud_batch(trk, 3, 0.02, 10, mu=0.1, max_iter=50)
    k = lib.calls[-1]
    assert k["trackers"] == [0x3000, 0x3001, 0x3002] and (k["F"], k["src"], k["tol"], k["min_size"], k["mu"], k["max_iter"]) == (3, 3, 0.02, 10, 0.1, 50)
    assert codes == [0, 0, 0] and s2.tolist() == [0.5, 1.5, 2.5] and nc == 3 and n_each == [70, 71, 72]
    lib.rc = B.TDLO_E_INVALID
    out = B.initialize_from_shared_cloud_batch(trk, 3, 0.02, 10, check=False)
    assert out[0] == B.TDLO_E_INVALID and out[3] == 4 and out[4] == [70, 71, 72]
    with pytest.raises(B.TdloError):
        B.initialize_from_shared_cloud_batch(trk, 3, 0.02, 10)
    for t in trk:
        t.h = None
