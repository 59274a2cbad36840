"""Raw depth aligned for many cameras in one call, without a GPU: the new names are declared, exported, documented and marshalled as the header lays them out;
the arena plan of csrc/tdlo_align_batch_plan.h keeps its blocks apart and aligned on random size lists, refuses beyond the budget and outside J = 1 .. 1024;
the grids of the two batch kernels, walked on the host in a sanitized stand-alone program over two consecutive different layouts of every scene list without a
fill in between, give the statement's planes and counts and leave every scratch word armed; the distinct-job rule of the aligning rig calls."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tracker_batch_cpu import addr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B
import align_ref as AR
import align_batch_scenes as S

NEW = ["tdlo_align_depth_batch", "tdlo_rig_to_cloud_aligning", "tdlo_tracker_frame_from_rig_aligning", "tdlo_tracker_frames_from_rig_aligning_batch",
       "tdlo_debug_align_batch_plan", "tdlo_debug_align_batch_arena", "tdlo_debug_align_distinct_jobs"]


def test_the_new_names_are_declared_exported_and_documented():
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_align_job;" in hdr and "tdlo_rig_raw_frame;" in hdr
    assert C.sizeof(B.AlignJobC) == 32 + 96 and B.AlignJobC.p.offset == 32 and C.sizeof(B.RigRawFrameC) == 32
    assert (B.RigRawFrameC.slot.offset, B.RigRawFrameC.cams.offset, B.RigRawFrameC.raw.offset, B.RigRawFrameC.K.offset) == (0, 8, 16, 24)
    for k in (61, 62, 63):
        assert lib.tdlo_debug_route_count(None, k) == -1
    assert re.search(r"\* 61 / 62 / 63: jobs of tdlo_align_depth_batch", text) and "a batch form for F frames or a rig's K cameras" not in text
    for word in ("NO HOST WAIT", "kAlignBatchMin", "TDLO_ALIGN_BATCH_MIN", "DISTINCT JOBS", "tdlo_tracker_frame_views_batch"):
        assert word in text, word
    for doc in ("README.md", "DESIGN.md"):
        assert "tdlo_align_depth_batch" in open(os.path.join(ROOT, doc)).read(), doc
    mk = open(os.path.join(ROOT, "trackdlo_amd", "csrc", "Makefile")).read()
    line = [ln for ln in mk.splitlines() if "-c tdlo_align_batch.hip" in ln]
    single = [ln for ln in mk.splitlines() if "-c tdlo_align.hip" in ln]
    assert len(line) == 1 and "-ffp-contract=off" in line[0] and "fast-math" not in line[0].split("#")[0] and "build/tdlo_align_batch.o" in mk.split("OBJ :=")[1].splitlines()[0]
    assert line[0].split("#")[0].replace("tdlo_align_batch.hip", "tdlo_align.hip").split() == single[0].split("#")[0].split()      # the single unit's flags exactly
    assert "tdlo_align_batch.hip" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()
    plan = open(os.path.join(ROOT, "trackdlo_amd", "csrc", "tdlo_align_batch_plan.h")).read()
    assert "EVERY WORD OF THE SCRATCH REGION IS ARMED" in plan


def test_the_scene_lists_have_the_properties_they_are_there_for():
    q = S.properties()
    assert q["one_tail"] == 3 and q["tail1"] == 1 and q["largest_second"] and q["Pd_off_block"] and q["Pc_mod4_2"]
    assert q["kinds"] == {"packed", "pitched", "bottom_up"} and q["wheres"] == {"host", "device"} and q["zero"] and q["f32"] and q["mf64"]
    assert len(S.LISTS["mixed7"]) == 7 and len(S.LISTS["one_5x7"]) == 1 and len(S.LISTS["full"]) == 3
    assert [j["share"] for j in S.LISTS["same_view"]] == [None, 0, None, 0]
    refs = S.reference("same_view")
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(refs[0][0], refs[3][0])          # one view, three different planes
    assert any(j["name"] == "fused" for j in S.LISTS["fused_among"])
    f = S.LISTS["full"]
    assert all(j["s"]["D"].shape == (480, 640) and (j["s"]["p"]["rows_c"], j["s"]["p"]["cols_c"]) == (720, 1280) for j in f)
    assert not np.array_equal(f[0]["s"]["D"], f[1]["s"]["D"]) and not np.array_equal(f[1]["s"]["D"], f[2]["s"]["D"])


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------------
def _blocks(rows, cols, plan):
    J = len(rows)
    out = []
    for j in range(J):
        P = rows[j] * cols[j]
        out += [("scratch", plan["scratch"][j], 4 * P), ("plane", plan["plane"][j], 2 * P), ("counts", plan["counts"][j], 32)]
    out.append(("table", plan["table"], 256 * J))
    return out


def test_plan_properties_over_random_size_lists():
    rng = np.random.default_rng(7)
    for trial in range(200):
        J = int(rng.integers(1, 40)) if trial else 1024
        rows = [int(v) for v in rng.integers(1, 90, J)]
        cols = [int(v) for v in rng.integers(1, 130, J)]
        plan = B.align_batch_plan(rows, cols)
        assert plan is not None
        blocks = sorted(_blocks(rows, cols, plan), key=lambda b: b[1])
        for (ka, a, na), (kb, b, nb) in zip(blocks, blocks[1:]):
            assert a + na <= b, (ka, kb)                                              # no two blocks overlap
        assert blocks[0][1] >= 0 and blocks[-1][1] + blocks[-1][2] <= plan["total"]
        sb = plan["scratch_bytes"]
        assert sb % 256 == 0
        for kind, at, n in blocks:
            if kind == "scratch":
                assert at % 16 == 0 and at + n <= sb                                   # all scratch lies inside [0, scratch_bytes) ...
            else:
                assert at >= sb                                                        # ... and nothing else does
            if kind == "plane":
                assert at % 256 == 0
            if kind == "counts":
                assert at % 8 == 0
            if kind == "table":
                assert at % 16 == 0
        assert plan["counts"] == [plan["counts"][0] + 32 * j for j in range(J)] and plan["table"] >= plan["counts"][-1] + 32
        # what a job gets depends only on the sizes in front of it: the reversed list is another layout of the same bytes
        rev = B.align_batch_plan(rows[::-1], cols[::-1])
        assert rev["total"] == plan["total"] and rev["scratch_bytes"] == sb
        # the budget: exactly the total passes, one byte less does not
        assert B.align_batch_plan(rows, cols, budget=plan["total"]) == plan and B.align_batch_plan(rows, cols, budget=plan["total"] - 1) is None


def test_plan_limits():
    assert B.align_batch_plan([], []) is None and B.align_batch_plan([4] * 1025, [4] * 1025) is None and B.align_batch_plan([4] * 1024, [4] * 1024) is not None
    assert B.align_batch_plan([0], [4]) is None and B.align_batch_plan([4], [-1]) is None and B.align_batch_plan([1 << 13], [(1 << 13) + 1]) is None
    big = B.align_batch_plan([720] * 64, [1280] * 64)                                   # 64 cameras at 1280 x 720: about 0.35 GiB
    assert big is not None and 0.32 < big["total"] / 2 ** 30 < 0.36
    assert B.align_batch_plan([720] * 200, [1280] * 200) is None                        # beyond the library's 1 GiB
    assert B.align_batch_plan([1 << 13] * 3, [1 << 13] * 3) is None


# ---- the kernels' grids on the host, sanitized -----------------------------------------------------------------------------------------------------------
def test_the_batch_grids_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/align_batch_host_test.cpp with csrc/tdlo_align_host.cpp and csrc/tdlo_image_host.cpp: no HIP, -fsanitize=address,undefined with the runtime
    linked into the program, run as a child process.  Every list in the given and in the reversed order, one arena, no fill between the two layouts."""
    names = list(S.LISTS)
    blob = [struct.pack("<i", len(names))]
    for name in names:
        blob.append(struct.pack("<i", len(S.LISTS[name])))
        for j in S.LISTS[name]:
            p, D = j["s"]["p"], np.ascontiguousarray(j["s"]["D"])
            blob.append(struct.pack("<8i", p["rows_d"], p["cols_d"], p["rows_c"], p["cols_c"], B.IMG_F32C1 if D.dtype == np.float32 else B.IMG_U16C1,
                                    int(p["T"] is not None), p["max_footprint"], ("packed", "pitched", "bottom_up").index(j["kind"])))
            T = np.zeros(12) if p["T"] is None else p["T"].reshape(12)
            blob.append(struct.pack("<20d", *[p[k] for k in ("fx_d", "fy_d", "cx_d", "cy_d", "fx_c", "fy_c", "cx_c", "cy_c")], *T))
            blob.append(D.tobytes())
    path, out = tmp_path / "lists.bin", tmp_path / "planes.bin"
    path.write_bytes(b"".join(blob))
    exe = str(tmp_path / "align_batch_host_test")
    csrc = os.path.join(ROOT, "trackdlo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "align_batch_host_test.cpp"), os.path.join(csrc, "tdlo_align_host.cpp"),
                        os.path.join(csrc, "tdlo_image_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(path), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"(\d+) calls, (\d+) lanes, (\d+) fills, 0 words not armed\n", r.stdout)
    assert m and int(m.group(1)) == 2 * len(names) and int(m.group(2)) % 256 == 0, r.stdout
    # the lists' scratch regions (bytes): a fill happens exactly where a region is longer than what the call before left armed, never for a reversed list
    sb = [B.align_batch_plan([j["s"]["p"]["rows_c"] for j in S.LISTS[n]], [j["s"]["p"]["cols_c"] for j in S.LISTS[n]])["scratch_bytes"] for n in names]
    assert int(m.group(3)) == sum(1 for i, b in enumerate(sb) if i == 0 or b > sb[i - 1]) and int(m.group(3)) >= 2
    raw = out.read_bytes()
    at = 0
    for name in names:
        refs = S.reference(name)
        for order in (range(len(refs)), reversed(range(len(refs)))):
            for j in order:
                A, n = refs[j]
                got = np.frombuffer(raw, np.uint16, A.size, at).reshape(A.shape); at += 2 * A.size
                gn = list(struct.unpack_from("<4q", raw, at)); at += 32
                assert np.array_equal(got, A) and gn == n, (name, j, gn, n)
    assert at == len(raw)


# ---- the distinct-job rule ---------------------------------------------------------------------------------------------------------------------------
def test_the_distinct_job_rule():
    s = AR.scene_upscale()
    D = s["D"]
    p = B.make_align_params(**s["p"])
    base = B.make_align_job(D, p)
    same = B.make_align_job(D, B.make_align_params(**dict(s["p"], T=s["p"]["T"].copy())))          # another matrix object holding the same twelve doubles
    assert base.p.depth_to_colour != same.p.depth_to_colour and B.align_distinct_jobs([base, same, base]) == [0, 0, 0]
    D2 = D.copy()
    diff = [B.make_align_job(D2, p)]                                                   # equal contents at another address: another view
    for field, value in (("format", B.IMG_F32C1), ("row_stride", 2 * D.shape[1] + 2), ("location", B.MEM_AUTO), ("ready_stream", 0x40)):
        j = B.make_align_job(D, p); setattr(j.depth, field, value); diff.append(j)
    T2 = s["p"]["T"].copy(); T2[1, 3] = np.nextafter(T2[1, 3], 1.0)
    for over in (dict(rows_d=47), dict(cols_d=63), dict(fx_d=61.0), dict(fy_d=61.0), dict(cx_d=1.0), dict(cy_d=1.0), dict(rows_c=71), dict(cols_c=95),
                 dict(fx_c=91.0), dict(fy_c=91.0), dict(cx_c=1.0), dict(cy_c=1.0), dict(T=None), dict(T=T2), dict(max_footprint=16), dict(cx_d=-s["p"]["cx_d"])):
        diff.append(B.make_align_job(D, B.make_align_params(**dict(s["p"], **over))))
    for j in diff:
        assert B.align_distinct_jobs([base, j]) == [0, 1]
    # bytewise: max_footprint 0 means 16 to the lane, but 0 and 16 are two jobs; +0.0 and -0.0 are two jobs
    z = dict(s["p"], cx_d=0.0)
    assert B.align_distinct_jobs([B.make_align_job(D, B.make_align_params(**z)), B.make_align_job(D, B.make_align_params(**dict(z, cx_d=-0.0)))]) == [0, 1]
    # numbered in order of first appearance, every entry against every earlier one
    order = [diff[0], base, diff[0], diff[3], same, diff[3]]
    assert B.align_distinct_jobs(order) == [0, 1, 0, 2, 1, 2]
    null_a = B.make_align_job(D, B.make_align_params(**dict(s["p"], T=None)))
    null_b = B.make_align_job(D, B.make_align_params(**dict(s["p"], T=None)))
    assert B.align_distinct_jobs([null_a, null_b]) == [0, 0]


# ---- marshalling against a stand-in library ----------------------------------------------------------------------------------------------------------
class StubLib:
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    @staticmethod
    def _jobs(p, n):
        out = []
        for j in (B.AlignJobC * n).from_address(addr(p)):
            T = list((C.c_double * 12).from_address(j.p.depth_to_colour)) if j.p.depth_to_colour else None
            out.append(dict(data=j.depth.data, format=j.depth.format, location=j.depth.location, row_stride=j.depth.row_stride, ready_stream=j.depth.ready_stream,
                            rows_d=j.p.rows_d, rows_c=j.p.rows_c, cols_c=j.p.cols_c, fx_c=j.p.fx_c, max_footprint=j.p.max_footprint, T=T))
        return out

    @staticmethod
    def _cams(p, n):
        return [dict(depth=c.depth, mask=c.mask, colour=c.colour, fx=c.fx, cy=c.cy, cam_to_rig=c.cam_to_rig) for c in (B.RigCameraC * n).from_address(addr(p))]

    @staticmethod
    def _counts(cnt, rows, base):
        if addr(cnt):
            a = (C.c_longlong * (4 * rows)).from_address(addr(cnt))
            for i in range(4 * rows):
                a[i] = base + i

    def tdlo_align_depth_batch(self, h, jobs, J, out, planes, cnt, rcs):               # (the header's order)
        self.calls.append(dict(h=h, J=J, jobs=self._jobs(jobs, J), out=list((C.c_void_p * J).from_address(addr(out))) if addr(out) else None, counts=addr(cnt) != 0))
        pl = (C.c_void_p * J).from_address(addr(planes))
        for j in range(J):
            pl[j] = 0xA000 + 0x100 * j
        self._counts(cnt, J, 10)
        return self.rc

    def tdlo_rig_to_cloud_aligning(self, h, slot, cams, raw, K, rows, cols, leaf, X, cap, n, nraw, cnt):
        self.calls.append(dict(h=h, slot=slot, cams=self._cams(cams, K), raw=self._jobs(raw, K), K=K, rows=rows, cols=cols, leaf=leaf, X=addr(X), cap=cap))
        n._obj.value = 0; nraw._obj.value = 5
        self._counts(cnt, K, 20)
        return self.rc

    def tdlo_tracker_frame_from_rig_aligning(self, t, cams, raw, K, rows, cols, leaf, d_vis, vis, nv, ext, ne, n, nraw, st, cnt):
        self.calls.append(dict(t=t, cams=self._cams(cams, K), raw=self._jobs(raw, K), K=K, rows=rows, cols=cols, leaf=leaf, d_vis=d_vis, st=addr(st)))
        nv._obj.value = 1; ne._obj.value = 2; n._obj.value = 7; nraw._obj.value = 9
        (C.c_int * 1).from_address(addr(vis))[0] = 3
        (C.c_int * 2).from_address(addr(ext))[:] = [2, 3]
        self._counts(cnt, K, 30)
        return self.rc

    def tdlo_tracker_frames_from_rig_aligning_batch(self, trk, F, frames, rows, cols, leaf, d_vis, vis, nv, ext, ne, n, nraw, st, rcs, cnt):
        fr = (B.RigRawFrameC * F).from_address(addr(frames))
        self.calls.append(dict(trackers=list((C.c_void_p * F).from_address(addr(trk))), F=F, rows=rows, cols=cols, leaf=leaf, d_vis=d_vis,
                               frames=[dict(K=f.K, cams=self._cams(f.cams, f.K), raw=self._jobs(f.raw, f.K)) for f in fr]))
        for i in range(F):
            (C.c_int * F).from_address(addr(nv))[i] = 1
            (C.c_int * F).from_address(addr(n))[i] = 40 + i
        self._counts(cnt, sum(f.K for f in fr), 50)
        return self.rc


def test_argtypes_are_the_header_s():
    L = B.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read(), flags=re.S)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    for name in NEW[:4] + NEW[4:]:
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
        args = [a.strip() for a in decl.split(",")]
        types = getattr(L, name).argtypes
        assert len(types) == len(args), (name, len(types), len(args))
        for a, t in zip(args, types):
            if "*" in a:
                assert t not in (ci, cd, C.c_longlong), (name, a)
            elif a.startswith("double"):
                assert t is cd, (name, a)
            elif a.startswith("long long"):
                assert t is C.c_longlong, (name, a)
            else:
                assert a.startswith("int") and t is ci, (name, a)


def test_marshalling_against_a_stand_in_library():
    lib = StubLib()
    ctx = stub_context(lib)
    ctx.get_cloud = lambda slot: "cloud"
    s = AR.scene_upscale()
    p = B.make_align_params(**s["p"])
    p1 = B.make_align_params(**dict(s["p"], T=None, max_footprint=3))
    D = s["D"]
    Df = AR.scene_f32()["D"]
    jobs = [B.make_align_job(D, p), (Df, p1), B.make_align_job(D, p1, ready_stream=0x77)]
    A, cnt, planes = ctx.align_depth_batch(jobs)
    k = lib.calls[-1]
    assert k["h"] == 0x1234 and k["J"] == 3 and k["counts"] and k["out"] == [a.ctypes.data for a in A] and all(a.shape == (72, 96) for a in A)
    assert [j["data"] for j in k["jobs"]] == [D.ctypes.data, Df.ctypes.data, D.ctypes.data] and [j["format"] for j in k["jobs"]] == [B.IMG_U16C1, B.IMG_F32C1, B.IMG_U16C1]
    assert [j["row_stride"] for j in k["jobs"]] == [2 * 64, 4 * 24, 2 * 64] and [j["ready_stream"] for j in k["jobs"]] == [None, None, 0x77]
    assert k["jobs"][0]["T"] == s["p"]["T"].reshape(-1).tolist() and k["jobs"][1]["T"] is None and [j["max_footprint"] for j in k["jobs"]] == [0, 3, 3]
    assert cnt == [[10, 11, 12, 13], [14, 15, 16, 17], [18, 19, 20, 21]] and planes == [0xA000, 0xA100, 0xA200]
    A, cnt, planes = ctx.align_depth_batch(jobs, out=None, counts=False)                # the no-wait form: nothing goes to the host
    assert A is None and cnt is None and lib.calls[-1]["out"] is None and not lib.calls[-1]["counts"] and planes[2] == 0xA200
    mine = np.zeros((72, 96), np.uint16)
    A, _, _ = ctx.align_depth_batch(jobs, out=[None, 0x7002, mine])
    assert lib.calls[-1]["out"] == [None, 0x7002, mine.ctypes.data] and A[0] is None and A[1] is None and A[2] is mine
    with pytest.raises(ValueError):
        ctx.align_depth_batch(jobs, out=[None])
    # the rig entrances
    mask = np.ones((72, 96), np.uint8)
    T = np.arange(12.0)
    cams = [B.RigCamera(None, mask=mask, cam=(90.0, 91.0, 48.0, 36.0)), B.RigCamera(None, mask=mask, cam=(92.0, 93.0, 47.0, 35.0), cam_to_rig=T)]
    X, n, nraw, cnt = ctx.rig_to_cloud_aligning(1, cams, jobs[:2], 0.008)
    k = lib.calls[-1]
    assert (k["slot"], k["K"], k["rows"], k["cols"], k["leaf"], k["X"], k["cap"]) == (1, 2, 72, 96, 0.008, 0, 0) and (X, n, nraw) == ("cloud", 0, 5)
    assert [c["depth"] for c in k["cams"]] == [None, None] and [c["mask"] for c in k["cams"]] == [mask.ctypes.data] * 2 and k["cams"][1]["fx"] == 92.0 and k["cams"][0]["cy"] == 36.0
    assert k["cams"][0]["cam_to_rig"] is None and list((C.c_double * 12).from_address(k["cams"][1]["cam_to_rig"])) == T.tolist()
    assert [j["data"] for j in k["raw"]] == [D.ctypes.data, Df.ctypes.data] and cnt == [[20, 21, 22, 23], [24, 25, 26, 27]]
    with pytest.raises(ValueError):
        ctx.rig_to_cloud_aligning(1, [B.RigCamera(D, mask=mask)], jobs[:1], 0.008)      # a camera that brings a depth plane
    with pytest.raises(ValueError):
        ctx.rig_to_cloud_aligning(1, cams, jobs[:1], 0.008)                             # one job per camera
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(2)]
    patched_handles(trk)
    v, e, n, nraw, cnt = trk[0].frame_from_rig_aligning(cams, jobs[:2], 0.01, 0.05)
    k = lib.calls[-1]
    assert k["t"] == 0x3000 and (k["K"], k["rows"], k["cols"], k["leaf"], k["d_vis"]) == (2, 72, 96, 0.01, 0.05) and k["st"] == addr(trk[0]._st_ptr)
    assert v.tolist() == [3] and e.tolist() == [2, 3] and (n, nraw) == (7, 9) and cnt == [[30, 31, 32, 33], [34, 35, 36, 37]]
    codes, vis, ext, n, nraw, cnt = B.frames_from_rig_aligning_batch(trk, [cams, cams[:1]], [jobs[:2], jobs[2:]], 0.008, 0.06)
    k = lib.calls[-1]
    assert k["trackers"] == [0x3000, 0x3001] and (k["F"], k["rows"], k["cols"], k["leaf"], k["d_vis"]) == (2, 72, 96, 0.008, 0.06)
    assert [f["K"] for f in k["frames"]] == [2, 1] and k["frames"][1]["raw"][0]["ready_stream"] == 0x77 and k["frames"][0]["cams"][1]["fx"] == 92.0
    assert codes == [0, 0] and n == [40, 41] and len(cnt) == 3 and cnt[2] == [58, 59, 60, 61] and [len(x) for x in vis] == [1, 1]
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.align_depth_batch(jobs)
    with pytest.raises(B.TdloError):
        ctx.rig_to_cloud_aligning(1, cams, jobs[:2], 0.008)
    with pytest.raises(B.TdloError):
        trk[0].frame_from_rig_aligning(cams, jobs[:2])
    for t in trk:
        t.h = None
