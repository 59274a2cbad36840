"""The binding's marshalling for the four batch calls, checked without a GPU against a stand-in library (as tests/bench_stub.py stands in for the
context under the bench): the shapes, the per-frame pointer tables, NULL for absent lists -- and that the binding requires the new symbols."""
import ctypes as C

import numpy as np
import pytest

from trackdlo_amd import binding as B

NEW = ["tdlo_visibility_prepass_batch", "tdlo_cpd_lle_batch_each", "tdlo_tracker_tracking_step_batch", "tdlo_tracker_frame_batch"]


def addr(p):
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    return C.cast(p, C.c_void_p).value or 0


def arr(p, n, ct):
    """n elements of ctypes type ct at pointer p, as a list."""
    return list((ct * n).from_address(addr(p))) if n else []


class StubLib:
    """Records what the binding hands to the four entry points and fills the outputs like the library would."""
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    def tdlo_visibility_prepass_batch(self, h, F, slots, Y, M, thr, d_vis, coord, dist, vis, nv, ext, ne):
        self.calls.append(dict(h=h, F=F, slots=arr(slots, F, C.c_int), Y=arr(Y, 3 * F * M, C.c_double), M=M, thr=thr, d_vis=d_vis, coord=arr(coord, F * M, C.c_double)))
        for i in range(F):
            (C.c_int * 1).from_address(addr(nv) + 4 * i)[0] = i + 1
            (C.c_int * 1).from_address(addr(ne) + 4 * i)[0] = i + 2
            row = (C.c_int * M).from_address(addr(ext) + 4 * M * i)
            for k in range(M):
                row[k] = 10 * i + k
            (C.c_double * M).from_address(addr(dist) + 8 * M * i)[0] = 0.5 + i
        return self.rc

    def tdlo_cpd_lle_batch_each(self, h, F, slots, Y, M, sigma2, params, args, stats):
        a = None
        if addr(args):
            a = [dict(priors=arr(x.priors, 4 * x.K, C.c_double), K=x.K, vis=arr(x.visible_nodes, x.n_vis, C.c_int), n_vis=x.n_vis,
                      H=arr(x.H_override, M * M, C.c_double) if x.H_override else None) for x in (B.FrameArgs * F).from_address(addr(args))]
        self.calls.append(dict(h=h, F=F, slots=arr(slots, F, C.c_int) if addr(slots) else None, Y=arr(Y, 3 * F * M, C.c_double), M=M,
                               sigma2=arr(sigma2, F, C.c_double), args=a))
        st = (B.Stats * F).from_address(addr(stats))
        for i in range(F):
            st[i].iters = 7 + i
        return self.rc

    def _trackers(self, tab, F):
        return arr(tab, F, C.c_void_p)

    def tdlo_tracker_tracking_step_batch(self, tab, F, vis, nv, ext, ne, H, stats, rcs):
        nvl, nel = arr(nv, F, C.c_int), arr(ne, F, C.c_int)
        pv, pe = arr(vis, F, C.c_void_p), arr(ext, F, C.c_void_p)
        self.calls.append(dict(trackers=self._trackers(tab, F), F=F, n_vis=nvl, n_ext=nel, vis=[arr(pv[i], nvl[i], C.c_int) for i in range(F)],
                               ext=[arr(pe[i], nel[i], C.c_int) for i in range(F)],
                               H=None if not addr(H) else [None if not p else arr(p, nel[i] ** 2, C.c_double) for i, p in enumerate(arr(H, F, C.c_void_p))]))
        st = (B.Stats * (2 * F)).from_address(addr(stats))
        for i in range(2 * F):
            st[i].iters = 100 + i
        (C.c_int * F).from_address(addr(rcs))[F - 1] = self.rc
        return self.rc

    def tdlo_tracker_frame_batch(self, tab, F, d_vis, vis, nv, ext, ne, stats, rcs):
        self.calls.append(dict(trackers=self._trackers(tab, F), F=F, d_vis=d_vis))
        M = 4
        for i in range(F):
            (C.c_int * 1).from_address(addr(nv) + 4 * i)[0] = 1
            (C.c_int * 1).from_address(addr(ne) + 4 * i)[0] = 2
            (C.c_int * M).from_address(addr(vis) + 4 * M * i)[0] = i
            e = (C.c_int * M).from_address(addr(ext) + 4 * M * i); e[0] = i; e[1] = i + 1
        st = (B.Stats * (2 * F)).from_address(addr(stats))
        for i in range(2 * F):
            st[i].iters = 200 + i
        return 0


def stub_context(lib):
    ctx = object.__new__(B.Context)
    ctx.lib = lib; ctx.h = 0x1234
    ctx.close = lambda: None
    return ctx


def stub_tracker(ctx, handle, M=4):
    t = object.__new__(B.trackdlo)
    t.ctx = ctx; t.h = None; t.M = M
    t._stats_raw = None; t._st = (B.Stats * 2)(); t._fv = None
    t._st_ptr = C.cast(t._st, C.c_void_p)
    t._handle = handle
    return t


@pytest.fixture
def lib():
    return StubLib()


def test_the_new_symbols_are_required():
    assert all(s in B.SYMBOLS for s in NEW)
    assert [f[0] for f in B.FrameArgs._fields_] == ["priors", "K", "visible_nodes", "n_vis", "H_override"]
    assert C.sizeof(B.FrameArgs) == 40           # {ptr, int, ptr, int, ptr} with the C ABI's padding


def test_visibility_prepass_batch_marshalling(lib):
    ctx = stub_context(lib)
    F, M = 3, 5
    Ys = np.arange(F * M * 3, dtype=np.float64).reshape(F, M, 3)
    coords = np.arange(F * M, dtype=np.float64).reshape(F, M) / 8
    dist, vis, ext = ctx.visibility_prepass_batch([5, 0, 3], Ys, 0.008, 0.06, coords)
    c = lib.calls[0]
    assert (c["h"], c["F"], c["M"], c["slots"], c["thr"], c["d_vis"]) == (0x1234, 3, 5, [5, 0, 3], 0.008, 0.06)
    for i in range(F):           # F consecutive column-major M x 3 blocks
        assert c["Y"][15 * i: 15 * (i + 1)] == Ys[i].T.reshape(-1).tolist()
    assert c["coord"] == coords.reshape(-1).tolist()
    assert dist.shape == (F, M) and [d[0] for d in dist] == [0.5, 1.5, 2.5]
    assert [len(v) for v in vis] == [1, 2, 3] and [e.tolist() for e in ext] == [[0, 1], [10, 11, 12], [20, 21, 22, 23]]
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.visibility_prepass_batch([0, 0, 1], Ys, 0.008, 0.06, coords)


def test_cpd_lle_batch_each_marshalling(lib):
    ctx = stub_context(lib)
    F, M = 3, 4
    Ys = np.arange(F * M * 3, dtype=np.float64).reshape(F, M, 3)
    pr = B.make_params(1.0, 2.0, 3.0, 0.1)
    # no lists at all: NULL for slots and args
    out = ctx.cpd_lle_batch_each(None, Ys, [0.0, 1e-4, 2e-4], pr)
    c = lib.calls[-1]
    assert c["slots"] is None and c["args"] is None and c["sigma2"] == [0.0, 1e-4, 2e-4] and (c["F"], c["M"]) == (3, 4)
    assert c["Y"][12:24] == Ys[1].T.reshape(-1).tolist()
    assert [s["iters"] for s in out["stats"]] == [7, 8, 9] and out["Y"].shape == (F, M, 3) and out["rc"] == 0
    # per-frame lists with absent entries
    pri = [np.array([[1.0, 0.1, 0.2, 0.3], [3.0, 0.4, 0.5, 0.6]]), None, None]
    vis = [[0, 1, 2], None, [1, 3]]
    H = [None, np.arange(16, dtype=np.float64).reshape(4, 4), None]
    ctx.cpd_lle_batch_each([2, 0, 1], Ys, [0.0] * 3, pr, priors=pri, visible_nodes=vis, H=H)
    c = lib.calls[-1]
    assert c["slots"] == [2, 0, 1]
    a = c["args"]
    assert (a[0]["K"], a[0]["priors"], a[0]["vis"], a[0]["H"]) == (2, pri[0].reshape(-1).tolist(), [0, 1, 2], None)
    assert (a[1]["K"], a[1]["n_vis"], a[1]["priors"], a[1]["vis"]) == (0, 0, [], []) and a[1]["H"] == H[1].T.reshape(-1).tolist()
    assert (a[2]["K"], a[2]["vis"], a[2]["H"]) == (0, [1, 3], None)
    # only one kind of list
    ctx.cpd_lle_batch_each(None, Ys, [0.0] * 3, pr, visible_nodes=vis)
    a = lib.calls[-1]["args"]
    assert [x["n_vis"] for x in a] == [3, 0, 2] and all(x["K"] == 0 and x["H"] is None for x in a)


def patched_handles(trackers):
    for t in trackers:
        t.h = t._handle


def test_tracking_step_batch_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x1000 + i) for i in range(3)]
    patched_handles(trk)
    vis = [[0, 1, 2, 3], [0, 1], []]
    ext = [[0, 1, 2, 3], [0, 1, 2], [3]]
    codes = B.tracking_step_batch(trk, vis, ext)
    c = lib.calls[-1]
    assert c["trackers"] == [0x1000, 0x1001, 0x1002] and c["F"] == 3 and c["H"] is None
    assert c["n_vis"] == [4, 2, 0] and c["n_ext"] == [4, 3, 1] and c["vis"] == vis and c["ext"] == ext
    assert codes == [0, 0, 0]
    for i, t in enumerate(trk):      # last_stats as the single calls fill them: [pre-processing, main]
        assert [s["iters"] for s in t.last_stats] == [100 + 2 * i, 101 + 2 * i]
    H = [np.arange(16, dtype=np.float64).reshape(4, 4), None, np.array([[2.0]])]
    B.tracking_step_batch(trk, vis, ext, H_pre=H)
    c = lib.calls[-1]
    assert c["H"][0] == H[0].T.reshape(-1).tolist() and c["H"][1] is None and c["H"][2] == [2.0]
    lib.rc = B.TDLO_E_EMPTY
    assert B.tracking_step_batch(trk, vis, ext, check=False) == [0, 0, B.TDLO_E_EMPTY]
    with pytest.raises(B.TdloError):
        B.tracking_step_batch(trk, vis, ext)
    for t in trk:
        t.h = None           # (nothing for __del__ to destroy)


def test_frame_batch_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x2000 + i) for i in range(2)]
    patched_handles(trk)
    codes, vis, ext = B.frame_batch(trk, 0.06)
    c = lib.calls[-1]
    assert c["trackers"] == [0x2000, 0x2001] and c["F"] == 2 and c["d_vis"] == 0.06
    assert codes == [0, 0] and [v.tolist() for v in vis] == [[0], [1]] and [e.tolist() for e in ext] == [[0, 1], [1, 2]]
    assert [s["iters"] for s in trk[1].last_stats] == [202, 203]
    for t in trk:
        t.h = None
