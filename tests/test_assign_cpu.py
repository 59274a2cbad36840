"""The binding's marshalling for the calls of "ropes of one colour", checked without a GPU against a stand-in library (as tests/test_rig_batch_cpu.py does):
the rope table as the header lays it out, the per-rope pointer tables, NULL for outputs nobody asked for, the argument order."""
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

    @staticmethod
    def _ropes(ropes, F):
        return [dict(slot=r.slot, M=r.M, Y=arr(r.Y, 3 * r.M, C.c_double)) for r in (B.AssignRopeC * F).from_address(addr(ropes))]

    def tdlo_get_cloud(self, h, slot, X, cap, n):
        n._obj.value = 5
        return 0

    def tdlo_cloud_assign(self, h, src, ropes, F, d_max, n_each, n_un, owner, d2):      # (the header's order)
        self.calls.append(dict(h=h, src=src, F=F, d_max=d_max, ropes=self._ropes(ropes, F), owner=addr(owner), d2=addr(d2)))
        for f in range(F):
            (C.c_int * 1).from_address(addr(n_each) + 4 * f)[0] = 2 + f
        n_un._obj.value = 1
        if addr(owner):
            (C.c_int * 5).from_address(addr(owner))[4] = 7
            (C.c_double * 5).from_address(addr(d2))[4] = 0.25
        return self.rc

    def tdlo_cloud_assign_visibility(self, h, src, ropes, F, d_max, thr, d_vis, coords, n_each, n_un, dist, vis, nv, ext, ne):
        rp = self._ropes(ropes, F)
        pc, pd, pv, pe = (arr(p, F, C.c_void_p) for p in (coords, dist, vis, ext))
        self.calls.append(dict(src=src, F=F, d_max=d_max, thr=thr, d_vis=d_vis, ropes=rp, coords=[arr(pc[f], rp[f]["M"], C.c_double) for f in range(F)]))
        for f in range(F):
            (C.c_int * 1).from_address(addr(n_each) + 4 * f)[0] = 3 + f
            (C.c_int * 1).from_address(addr(nv) + 4 * f)[0] = 1
            (C.c_int * 1).from_address(addr(ne) + 4 * f)[0] = rp[f]["M"]
            (C.c_int * 1).from_address(pv[f])[0] = f
            (C.c_double * 1).from_address(pd[f])[0] = 0.5 + f
            e = (C.c_int * rp[f]["M"]).from_address(pe[f])
            for k in range(rp[f]["M"]):
                e[k] = k
        n_un._obj.value = 9
        return self.rc

    def tdlo_tracker_frames_from_shared_cloud_batch(self, tab, F, src, d_max, d_vis, vis, nv, ext, ne, n_each, stats, rcs):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, src=src, d_max=d_max, d_vis=d_vis))
        M = 4
        for i in range(F):
            (C.c_int * 1).from_address(addr(nv) + 4 * i)[0] = 1
            (C.c_int * 1).from_address(addr(ne) + 4 * i)[0] = 2
            (C.c_int * M).from_address(addr(vis) + 4 * M * i)[0] = i
            e = (C.c_int * M).from_address(addr(ext) + 4 * M * i); e[0] = i; e[1] = i + 1
            (C.c_int * 1).from_address(addr(n_each) + 4 * i)[0] = 70 + i
        st = (B.Stats * (2 * F)).from_address(addr(stats))
        for i in range(2 * F):
            st[i].iters = 300 + i
        (C.c_int * F).from_address(addr(rcs))[F - 1] = self.rc
        return self.rc


@pytest.fixture
def lib():
    return StubLib()


def ropes2():
    return np.arange(6.0).reshape(2, 3), 10.0 + np.arange(9.0).reshape(3, 3)


def test_argtypes_are_the_header_s():
    L = B.load_library()
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    assert list(L.tdlo_cloud_assign.argtypes[:5]) == [vp, ci, vp, ci, cd] and len(L.tdlo_cloud_assign.argtypes) == 9
    assert list(L.tdlo_cloud_assign_visibility.argtypes[:7]) == [vp, ci, vp, ci, cd, cd, cd] and len(L.tdlo_cloud_assign_visibility.argtypes) == 15
    assert list(L.tdlo_cloud_assign_host.argtypes[:5]) == [vp, ci, vp, ci, cd] and len(L.tdlo_cloud_assign_host.argtypes) == 9
    assert list(L.tdlo_tracker_frames_from_shared_cloud_batch.argtypes[:5]) == [vp, ci, ci, cd, cd] and len(L.tdlo_tracker_frames_from_shared_cloud_batch.argtypes) == 12


def test_cloud_assign_marshalling(lib):
    ctx = stub_context(lib)
    Ya, Yb = ropes2()
    assert ctx.cloud_assign(3, [(1, Ya), (0, Yb)], 0.01) == ([2, 3], 1)
    k = lib.calls[-1]
    assert (k["h"], k["src"], k["F"], k["d_max"], k["owner"], k["d2"]) == (0x1234, 3, 2, 0.01, 0, 0)
    assert [(r["slot"], r["M"]) for r in k["ropes"]] == [(1, 2), (0, 3)]
    assert k["ropes"][0]["Y"] == Ya.T.reshape(-1).tolist() and k["ropes"][1]["Y"] == Yb.T.reshape(-1).tolist()      # column-major M x 3
    n_each, un, own, d2 = ctx.cloud_assign(3, [(1, Ya), (0, Yb)], np.inf, owners=True)
    assert lib.calls[-1]["d_max"] == np.inf and own.shape == d2.shape == (5,) and own[4] == 7 and d2[4] == 0.25
    lib.rc = B.TDLO_E_INVALID
    assert ctx.cloud_assign(3, [(1, Ya)], 0.01, check=False)[0] == B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.cloud_assign(3, [(1, Ya)], 0.01)


def test_cloud_assign_visibility_marshalling(lib):
    ctx = stub_context(lib)
    Ya, Yb = ropes2()
    n_each, un, dist, vis, ext = ctx.cloud_assign_visibility(2, [(0, Ya), (1, Yb)], 0.02, 0.008, 0.06, [[0.0, 0.1], [0.0, 0.2, 0.4]])
    k = lib.calls[-1]
    assert (k["src"], k["F"], k["d_max"], k["thr"], k["d_vis"]) == (2, 2, 0.02, 0.008, 0.06) and k["coords"] == [[0.0, 0.1], [0.0, 0.2, 0.4]]
    assert n_each == [3, 4] and un == 9 and [d[0] for d in dist] == [0.5, 1.5] and [len(d) for d in dist] == [2, 3]
    assert [v.tolist() for v in vis] == [[0], [1]] and [e.tolist() for e in ext] == [[0, 1], [0, 1, 2]]


def test_tracker_entrance_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    codes, vis, ext, n_each = B.frames_from_shared_cloud_batch(trk, 3, 0.02, 0.06)
    k = lib.calls[-1]
    assert k["trackers"] == [0x3000, 0x3001, 0x3002] and (k["F"], k["src"], k["d_max"], k["d_vis"]) == (3, 3, 0.02, 0.06)
    assert codes == [0, 0, 0] and [v.tolist() for v in vis] == [[0], [1], [2]] and [e.tolist() for e in ext] == [[0, 1], [1, 2], [2, 3]]
    assert n_each == [70, 71, 72] and [s["iters"] for s in trk[2].last_stats] == [304, 305]
    lib.rc = B.TDLO_E_EMPTY
    assert B.frames_from_shared_cloud_batch(trk, 3, 0.02, 0.06, check=False)[0] == [0, 0, B.TDLO_E_EMPTY]
    with pytest.raises(B.TdloError):
        B.frames_from_shared_cloud_batch(trk, 3, 0.02, 0.06)
    for t in trk:
        t.h = None
