"""tdlo_cloud_view_voxel_grid_batch / tdlo_set_cloud_view_batch / the two tracker entrances without a GPU: the names are declared, required and exported; the
arena plan (csrc/tdlo_view_batch_plan.h) keeps every block apart, on 256 bytes and inside its total, with the state blocks where no N can move them -- through
the library's export and in a stand-alone sanitized program; the binding's marshalling is what the header lays down, checked against a stand-in library as
tests/test_cloud_batch_cpu.py does; and for the scenes of tests/test_view_batch_gpu.py the reference alone says which frames the batch launch serves."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B
import view_batch_scenes as S
import voxel_ref

NEW = ["tdlo_cloud_view_voxel_grid_batch", "tdlo_set_cloud_view_batch", "tdlo_tracker_tracking_step_view_batch", "tdlo_tracker_frames_from_cloud_view_batch",
       "tdlo_debug_view_batch_plan"]
N_SETS = [[1], [4096, 1, 4097], [1 << 20, 5], list(S.SIZES), [4097] * 32]


def test_the_new_names_are_declared_required_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_view_frame;" in hdr
    assert "#define TDLO_ABI_VERSION 3" in re.sub(r"[ \t]+", " ", hdr) and lib.tdlo_abi_version() == 3
    for name in ("set_cloud_view_batch", "voxel_grid_view_batch", "view_batch_route_counts"):
        assert callable(getattr(B.Context, name))
    assert callable(B.tracking_step_view_batch) and callable(B.frames_from_cloud_view_batch)
    # the struct as the C ABI lays it out: {int, pointer, int, pointer}
    assert [f[0] for f in B.ViewFrame._fields_] == ["slot", "view", "N", "select"] and C.sizeof(B.ViewFrame) == 32
    assert (B.ViewFrame.view.offset, B.ViewFrame.N.offset, B.ViewFrame.select.offset) == (8, 16, 24)
    # the route counters: -1 only for an unknown counter or a null context
    assert lib.tdlo_debug_route_count(None, 38) == -1 and lib.tdlo_debug_route_count(None, 41) == -1


def test_a_null_context_is_refused():
    lib = B.load_library()
    P = np.zeros((4, 3), dtype=np.float32)
    v = B.cloud_view(P)
    fr = (B.ViewFrame * 1)(); fr[0].slot = 0; fr[0].view = C.addressof(v); fr[0].N = 4
    n = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tdlo_cloud_view_voxel_grid_batch(None, C.cast(fr, C.c_void_p), 1, 0.008, p(n), p(n), None) == B.TDLO_E_INVALID
    pv = (C.c_void_p * 1)(C.addressof(v))
    assert lib.tdlo_set_cloud_view_batch(None, p(n), C.cast(pv, C.c_void_p), p(np.array([4], dtype=np.int32)), 1, None) == B.TDLO_E_INVALID
    assert lib.tdlo_tracker_tracking_step_view_batch(None, 1, None, None, None, None, None, None, None, None, None) == B.TDLO_E_INVALID
    assert lib.tdlo_tracker_frames_from_cloud_view_batch(None, 1, C.cast(fr, C.c_void_p), 0.008, 0.06, None, None, None, None, None, None, None, None) == B.TDLO_E_INVALID


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
def _blocks(plan, N):
    """(offset, bytes, name) of every block the kernel addresses, the table included (its size from the gap the plan leaves is not used: desc bytes are the
    library's own, so the table is taken up to the first frame block)."""
    out = [(plan["table"], min(plan["tiles"]) - plan["table"], "table")]
    for f, n in enumerate(N):
        T = (n + S.TILE - 1) // S.TILE
        out += [(plan["state"][f], 256, f"state {f}"), (plan["tiles"][f], 12 * n, f"tiles {f}"), (plan["pts"][f], 12 * S.NMAX, f"pts {f}"), (plan["cnt"][f], 4 * T, f"cnt {f}")]
    return out


@pytest.mark.parametrize("N", N_SETS, ids=[str(len(n)) + "x" + str(max(n)) for n in N_SETS])
def test_plan_blocks_are_disjoint_aligned_and_inside_the_total(N):
    Fcap = 32
    plan = B.view_batch_plan(N, Fcap)
    assert plan is not None
    blocks = sorted(_blocks(plan, N))
    for off, size, name in blocks:
        assert off % 256 == 0 and size > 0 and off + size <= plan["total"], name
    for (o0, s0, n0), (o1, _, n1) in zip(blocks, blocks[1:]):
        assert o0 + s0 <= o1, (n0, n1)
    # the state blocks are an array in front of everything else: room for every slot of the context
    assert plan["state"] == [256 * f for f in range(len(N))] and plan["table"] == 256 * Fcap


def test_the_place_of_the_state_blocks_is_independent_of_the_sizes():
    F = 3
    seen = {tuple(B.view_batch_plan(N, 16)["state"]) for N in ([1, 1, 1], [4096, 1, 4097], [1 << 20, 5, 70000], [9, 1 << 20, 1 << 20])}
    assert seen == {tuple(256 * f for f in range(F))}
    # ... nor of F: frame f of a longer call finds its block where a shorter call's frame f had it
    assert B.view_batch_plan([5] * 16, 16)["state"][:3] == B.view_batch_plan([7, 8, 9], 16)["state"]
    # frame blocks are sized by each frame's own N
    small, big = B.view_batch_plan([5, 5], 4), B.view_batch_plan([1 << 20, 5], 4)
    assert big["total"] - small["total"] == (12 * (1 << 20) + 4 * 256) - 2 * 256


def test_plan_refusals():
    assert B.view_batch_plan([], 4) is None and B.view_batch_plan([0], 4) is None and B.view_batch_plan([(1 << 20) + 1], 4) is None
    assert B.view_batch_plan([5] * 5, 4) is None and B.view_batch_plan([5] * 4, 4) is not None
    lib = B.load_library()
    Na = np.array([5, 6], dtype=np.int32); total = C.c_longlong(-1)
    assert lib.tdlo_debug_view_batch_plan(Na.ctypes.data_as(C.c_void_p), 2, 4, None, None, None, None, None, C.byref(total)) == 0 and total.value == B.view_batch_plan([5, 6], 4)["total"]
    assert lib.tdlo_debug_view_batch_plan(None, 2, 4, None, None, None, None, None, C.byref(total)) == B.TDLO_E_INVALID


def test_plan_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/view_batch_plan_host_test.cpp: the plan header alone (no HIP), built with -fsanitize=address,undefined (the runtime linked into the program),
    run as a child process of its own: it fills every block of every frame in a heap arena of exactly `total` bytes.  Nothing sanitized is loaded into python."""
    exe = str(tmp_path / "view_batch_plan_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "trackdlo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "view_batch_plan_host_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for N in N_SETS:
        Fcap = max(len(N), 8)
        plan = B.view_batch_plan(N, Fcap)
        # the program is given the room the library's plan leaves for one descriptor (its size is the library's own)
        room = plan["tiles"][0] - plan["table"]
        r = subprocess.run([exe, str(Fcap), str(room // len(N))] + [str(n) for n in N], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (N, r.stdout + r.stderr)
        lines = r.stdout.split("\n")
        m = re.fullmatch(r"F=(\d+) Fcap=(\d+) table=(\d+) total=(\d+)", lines[0])
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(N), Fcap, plan["table"])
        rows = [[int(x) for x in ln.split()] for ln in lines[1:1 + len(N)]]
        assert [row[0] for row in rows] == plan["state"]
        # the same frame blocks one behind the other, whatever the table's size
        shift = rows[0][1] - plan["tiles"][0]
        assert abs(shift) < 256 * len(N) + 256
        assert [[row[1] - shift, row[2] - shift, row[3] - shift] for row in rows] == [list(t) for t in zip(plan["tiles"], plan["pts"], plan["cnt"])]
        assert int(m.group(4)) - shift == plan["total"]
    r = subprocess.run([exe, "4", "64", "5", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "refused" in r.stdout
    r = subprocess.run([exe, "1", "64", "5", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "refused" in r.stdout


# ---- the routes of the GPU file's scenes, from the reference alone -----------------------------------------------------------------------------------
def test_the_reference_says_which_frames_are_served():
    assert S.counts([(S.rope(N, 40 + k), None) for k, N in enumerate(S.SIZES)]) == [8, 0]
    routes = {name: S.route(P, sel) for name, P, sel in S.borders()}
    assert routes == {"rope-a": "served", "32704 kept": "served", "32705 kept": "passed", "rope-b": "served", "rb + kb = 33": "passed", "pass-through": "passed",
                      "keeps nothing": "served", "non-finite, -0.0f": "served", "rope-c": "served"}
    st = {name: voxel_ref.structure(P, sel, S.LEAF) for name, P, sel in S.borders()}
    assert st["32704 kept"]["n_raw"] == S.NMAX and st["32704 kept"]["rb"] + st["32704 kept"]["kb"] <= 32
    assert st["32705 kept"]["n_raw"] == S.NMAX + 1 and st["32705 kept"]["rb"] + st["32705 kept"]["kb"] <= 32 and not st["32705 kept"]["nodown"]
    assert st["rb + kb = 33"]["rb"] + st["rb + kb = 33"]["kb"] == 33 and not st["rb + kb = 33"]["nodown"]
    assert st["pass-through"]["nodown"] and st["keeps nothing"]["n_raw"] == 0
    assert st["non-finite, -0.0f"]["n_raw"] == len(S.special_cloud()) - 4
    with pytest.raises(voxel_ref.TooFar):
        voxel_ref.structure(S.far_cloud(), None, S.LEAF)
    assert S.route(S.far_cloud(), None) == "passed"
    Pb, sb = S.big_view()
    assert len(Pb) == S.MAX_N + 1 and S.route(Pb, sb) == "passed" and S.route(Pb[:S.MAX_N], sb[:S.MAX_N]) == "served"
    P, sels = S.organized()
    assert [S.route(P, s) for s in sels] == ["served"] * 3 and not ((sels[0] != 0) & (sels[1] != 0)).any() and not ((sels[1] != 0) & (sels[2] != 0)).any()
    # with the one-launch form off every frame is handed to the single call
    assert S.counts([(S.rope(5, 1), None), (S.rope(4097, 2), None)], fused=False) == [0, 2]


# ---- the binding's marshalling ----------------------------------------------------------------------------------------------------------------------
class StubLib:
    """Records what the binding hands to the four entry points and fills the outputs like the library would."""
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    @staticmethod
    def _view(p, N):
        v = B.CloudView.from_address(p)
        ct = C.c_float if v.dtype == B.F32 else C.c_double
        es = C.sizeof(ct)
        pts = [[ct.from_address(v.data + es * (n * v.stride_point + c * v.stride_comp)).value for c in range(3)] for n in range(N)]
        return dict(dtype=v.dtype, location=v.location, sp=v.stride_point, sc=v.stride_comp, ready=v.ready_stream, flags=v.flags, pts=pts)

    def _frames(self, frames, F):
        return [dict(slot=f.slot, N=f.N, view=self._view(f.view, f.N), select=None if not f.select else arr(f.select, f.N, C.c_uint8))
                for f in (B.ViewFrame * F).from_address(addr(frames))] if F else []

    def tdlo_cloud_view_voxel_grid_batch(self, h, frames, F, leaf, n, nraw, rcs):
        self.calls.append(dict(h=h, F=F, leaf=leaf, frames=self._frames(frames, F)))
        for i in range(F):
            (C.c_int * 1).from_address(addr(n) + 4 * i)[0] = 10 + i
            (C.c_int * 1).from_address(addr(nraw) + 4 * i)[0] = 100 + i
        if F:
            (C.c_int * 1).from_address(addr(rcs) + 4 * (F - 1))[0] = self.rc
        return self.rc

    def tdlo_set_cloud_view_batch(self, h, slots, views, N, F, rcs):
        Nl = arr(N, F, C.c_int)
        self.calls.append(dict(h=h, F=F, slots=arr(slots, F, C.c_int), N=Nl, views=[self._view(p, Nl[i]) for i, p in enumerate(arr(views, F, C.c_void_p))]))
        if F:
            (C.c_int * 1).from_address(addr(rcs) + 4 * (F - 1))[0] = self.rc
        return self.rc

    def tdlo_tracker_tracking_step_view_batch(self, tab, F, views, N, vis, nv, ext, ne, H, stats, rcs):
        Nl, nvl, nel = arr(N, F, C.c_int), arr(nv, F, C.c_int), arr(ne, F, C.c_int)
        pv, pe = arr(vis, F, C.c_void_p), arr(ext, F, C.c_void_p)
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, N=Nl, views=[self._view(p, Nl[i]) for i, p in enumerate(arr(views, F, C.c_void_p))],
                               vis=[arr(pv[i], nvl[i], C.c_int) for i in range(F)], ext=[arr(pe[i], nel[i], C.c_int) for i in range(F)],
                               H=None if not addr(H) else [None if not p else arr(p, nel[i] ** 2, C.c_double) for i, p in enumerate(arr(H, F, C.c_void_p))]))
        st = (B.Stats * (2 * F)).from_address(addr(stats))
        for i in range(2 * F):
            st[i].iters = 100 + i
        (C.c_int * F).from_address(addr(rcs))[F - 1] = self.rc
        return self.rc

    def tdlo_tracker_frames_from_cloud_view_batch(self, tab, F, frames, leaf, d_vis, vis, nv, ext, ne, n, nraw, stats, rcs):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, leaf=leaf, d_vis=d_vis, frames=self._frames(frames, F)))
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


def clouds():
    rng = np.random.default_rng(4)
    a = rng.standard_normal((5, 3)).astype(np.float32)                        # packed float32
    b = rng.standard_normal((4, 8)).astype(np.float32)                        # PointXYZRGB: 8 floats a point
    c = np.asfortranarray(rng.standard_normal((6, 3)))                        # column-major float64
    return a, b, c


def test_voxel_grid_view_batch_marshalling(lib):
    ctx = stub_context(lib)
    ctx._async_src = None
    a, b, c = clouds()
    sel = np.array([1, 0, 0, 7], dtype=np.uint8)
    selb = np.array([True, False, True, True, False, True])
    n, nraw, codes = ctx.voxel_grid_view_batch([(5, a, None), (0, b, sel), (3, c, selb), (2, a[::-1], None)], 0.008)
    k = lib.calls[-1]
    assert (k["h"], k["F"], k["leaf"]) == (0x1234, 4, 0.008)
    f = k["frames"]
    assert [(x["slot"], x["N"]) for x in f] == [(5, 5), (0, 4), (3, 6), (2, 5)]
    assert [(x["view"]["dtype"], x["view"]["sp"], x["view"]["sc"], x["view"]["location"]) for x in f] == \
        [(B.F32, 3, 1, B.MEM_HOST), (B.F32, 8, 1, B.MEM_HOST), (B.F64, 1, 6, B.MEM_HOST), (B.F32, -3, 1, B.MEM_HOST)]
    assert np.array_equal(np.array(f[0]["view"]["pts"], dtype=np.float32), a) and np.array_equal(np.array(f[1]["view"]["pts"], dtype=np.float32), b[:, :3])
    assert np.array_equal(np.array(f[2]["view"]["pts"]), c) and np.array_equal(np.array(f[3]["view"]["pts"], dtype=np.float32), a[::-1])
    assert f[0]["select"] is None and f[1]["select"] == [1, 0, 0, 7] and f[2]["select"] == [1, 0, 1, 1, 0, 1] and f[3]["select"] is None
    assert (n, nraw, codes) == ([10, 11, 12, 13], [100, 101, 102, 103], [0, 0, 0, 0])
    # one view named by several frames: the same tdlo_cloud_view, different selection bytes
    v = B.cloud_view(b)
    ctx.voxel_grid_view_batch([(0, v, sel), (1, v, None), (2, v, 1 - (sel != 0))], 0.01)
    f = lib.calls[-1]["frames"]
    assert [x["select"] for x in f] == [[1, 0, 0, 7], None, [0, 1, 1, 0]] and all(x["view"] == f[0]["view"] for x in f)
    # a per-frame code: returned with check=False, raised otherwise
    lib.rc = B.TDLO_E_INVALID
    assert ctx.voxel_grid_view_batch([(0, a, None)], 0.008, check=False)[2] == [B.TDLO_E_INVALID]
    with pytest.raises(B.TdloError):
        ctx.voxel_grid_view_batch([(0, a, None)], 0.008)
    # selection bytes of the wrong length never reach the library
    ncalls = len(lib.calls)
    with pytest.raises(ValueError):
        ctx.voxel_grid_view_batch([(0, a, sel)], 0.008)
    assert len(lib.calls) == ncalls


def test_set_cloud_view_batch_marshalling(lib):
    ctx = stub_context(lib)
    ctx._async_src = None
    a, b, c = clouds()
    assert ctx.set_cloud_view_batch([4, 1, 7], [a, b, c]) == [0, 0, 0]
    k = lib.calls[-1]
    assert (k["h"], k["F"], k["slots"], k["N"]) == (0x1234, 3, [4, 1, 7], [5, 4, 6])
    assert [(v["dtype"], v["sp"], v["sc"]) for v in k["views"]] == [(B.F32, 3, 1), (B.F32, 8, 1), (B.F64, 1, 6)]
    assert np.array_equal(np.array(k["views"][1]["pts"], dtype=np.float32), b[:, :3]) and np.array_equal(np.array(k["views"][2]["pts"]), c)
    lib.rc = B.TDLO_E_INVALID
    assert ctx.set_cloud_view_batch([0, 1], [a, b], check=False) == [0, B.TDLO_E_INVALID]
    with pytest.raises(B.TdloError):
        ctx.set_cloud_view_batch([0, 1], [a, b])


def test_tracker_entrances_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    a, b, c = clouds()
    H = np.arange(4.0).reshape(2, 2)
    codes = B.tracking_step_view_batch(trk, [a, b, c], [[0, 1], [2], []], [[0, 1, 2], [2, 3], [1, 2]], H_pre=[None, H, None])
    k = lib.calls[-1]
    assert k["trackers"] == [0x3000, 0x3001, 0x3002] and (k["F"], k["N"]) == (3, [5, 4, 6])
    assert [(v["dtype"], v["sp"], v["sc"]) for v in k["views"]] == [(B.F32, 3, 1), (B.F32, 8, 1), (B.F64, 1, 6)]
    assert k["vis"] == [[0, 1], [2], []] and k["ext"] == [[0, 1, 2], [2, 3], [1, 2]]
    assert k["H"][0] is None and k["H"][2] is None and k["H"][1] == [0.0, 2.0, 1.0, 3.0]      # (column-major, as the library takes H)
    assert codes == [0, 0, 0] and [s["iters"] for s in trk[2].last_stats] == [104, 105]
    B.tracking_step_view_batch(trk, [a, b, c], [[0]] * 3, [[0, 1]] * 3)
    assert lib.calls[-1]["H"] is None
    sel = np.array([0, 1, 1, 0], dtype=np.uint8)
    codes, vis, ext, n, nraw = B.frames_from_cloud_view_batch(trk, [a, b, c], 0.008, 0.06, selects=[None, sel, None])
    k = lib.calls[-1]
    assert k["trackers"] == [0x3000, 0x3001, 0x3002] and (k["F"], k["leaf"], k["d_vis"]) == (3, 0.008, 0.06)
    assert [x["N"] for x in k["frames"]] == [5, 4, 6] and [x["select"] for x in k["frames"]] == [None, [0, 1, 1, 0], None]
    assert codes == [0, 0, 0] and [v.tolist() for v in vis] == [[0], [1], [2]] and [e.tolist() for e in ext] == [[0, 1], [1, 2], [2, 3]]
    assert n == [50, 51, 52] and nraw == [500, 501, 502] and [s["iters"] for s in trk[2].last_stats] == [304, 305]
    B.frames_from_cloud_view_batch(trk, [a, b, c], 0.008, 0.06)
    assert [x["select"] for x in lib.calls[-1]["frames"]] == [None, None, None]
    lib.rc = B.TDLO_E_EMPTY
    assert B.frames_from_cloud_view_batch(trk, [a, b, c], 0.008, 0.06, check=False)[0] == [0, 0, B.TDLO_E_EMPTY]
    with pytest.raises(B.TdloError):
        B.frames_from_cloud_view_batch(trk, [a, b, c], 0.008, 0.06)
    for t in trk:
        t.h = None           # (nothing for __del__ to destroy)
