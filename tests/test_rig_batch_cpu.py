"""tdlo_rig_to_cloud_batch / tdlo_tracker_frames_from_rig_batch without a GPU: the names are declared, required and exported; the arena plan
(csrc/tdlo_rig_batch_plan.h) keeps the blocks of a launch apart, aligned and inside its total, with a frame's state block at 256 x its slot, every shared
plane once, and the budget rule splitting the frames into launches as the header states -- through the library's export and in a stand-alone sanitized
program; the binding's marshalling is what the header lays down, checked against a stand-in library as tests/test_tracker_batch_cpu.py does; the whole-call
refusals that tdlo_rig_check decides; and for the scenes of tests/test_rig_batch_gpu.py the reference alone says which frames the batch launch serves."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles
from trackdlo_amd import binding as B
import rig_batch_scenes as BS
import rig_ref as R
import rig_scenes as S

NEW = ["tdlo_rig_to_cloud_batch", "tdlo_tracker_frames_from_rig_batch", "tdlo_debug_rig_batch_plan", "tdlo_debug_rig_batch_arena"]
TILE, NMAX = 4096, 32704


def test_the_new_names_are_declared_required_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_rig_frame;" in hdr
    for name in ("rig_to_cloud_batch", "rig_batch_route_counts", "rig_batch_arena"):
        assert callable(getattr(B.Context, name))
    assert callable(B.frames_from_rig_batch) and callable(B.rig_batch_plan)
    # the struct as the C ABI lays it out: {int, pointer, int}
    assert [f[0] for f in B.RigFrameC._fields_] == ["slot", "cams", "K"] and C.sizeof(B.RigFrameC) == 24
    assert (B.RigFrameC.cams.offset, B.RigFrameC.K.offset) == (8, 16)
    # the route counters: -1 for a null context; 49 and 50 stand in the header's list
    assert lib.tdlo_debug_route_count(None, 49) == -1 and lib.tdlo_debug_route_count(None, 50) == -1
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    assert re.search(r"\* 49 / 50: frames of tdlo_rig_to_cloud_batch", text)


def test_null_arguments_and_what_tdlo_rig_check_decides():
    """Without a context the calls answer TDLO_E_INVALID; the part of the whole-call refusal that needs no GPU is tdlo_rig_check on every frame's rig."""
    lib = B.load_library()
    one, three, colour = BS.companions(8, 8)
    tab, F, rows, cols, keep = B._rig_frames([(0, S.binding_cams(B, three))])
    n = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tdlo_rig_to_cloud_batch(None, C.cast(tab, C.c_void_p), 1, rows, cols, 0.008, p(n), p(n), None) == B.TDLO_E_INVALID
    assert lib.tdlo_tracker_frames_from_rig_batch(None, 1, C.cast(tab, C.c_void_p), rows, cols, 0.008, 0.06, None, None, None, None, None, None, None, None) == B.TDLO_E_INVALID
    assert lib.tdlo_debug_rig_batch_arena(None, None, None) == B.TDLO_E_INVALID
    assert B.rig_check(S.binding_cams(B, three)) == 0 and B.rig_check(S.binding_cams(B, colour)) == 0
    bad = {"mixed kinds": [three[0], colour[0]], "fx = 0": [three[0].replaced(cam=(0.0, 600.0, 1.0, 1.0))], "65 cameras": [one[0]] * 65,
           "nan in cam_to_rig": [three[1].replaced(T=np.where(np.arange(12).reshape(3, 4) == 5, np.nan, three[1].T))]}
    for what, cams in bad.items():
        assert B.rig_check(S.binding_cams(B, cams)) == B.TDLO_E_INVALID, what
    # rigs of different image sizes never reach the library
    with pytest.raises(ValueError):
        B._rig_frames([(0, S.binding_cams(B, three)), (1, S.binding_cams(B, BS.companions(8, 9)[0]))])


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
def keys_of(Ks, share=None, colour=()):
    """Plane keys of frames of Ks[f] mask cameras (frames in `colour`: colour cameras with an occluder): every plane distinct, except that the frames in
    `share` name frame share[0]'s depth (and colour) planes."""
    keys, nxt = [], [1000]

    def new():
        nxt[0] += 8
        return nxt[0]
    first = {}
    for f, K in enumerate(Ks):
        for k in range(K):
            shared = share and f in share
            depth = first.setdefault(("d", k), new()) if shared else new()
            if f in colour:
                img = first.setdefault(("c", k), new()) if shared else new()
                keys += [depth, 0, img, new()]
            else:
                keys += [depth, new(), 0, 0]
    return keys


def blocks_of(plan, slots, Ks, P, keys, launch):
    """(offset, bytes, name) of everything a launch addresses: the fixed part and the blocks of the launch's own frames."""
    Tc = (P + TILE - 1) // TILE
    out = [(plan["table"], plan["cams"][0] - plan["table"], "table"), (plan["cams"][0], min(o for o in plan["plane"] if o >= 0) - plan["cams"][0], "cameras")]
    size = {0: 2 * P, 1: P, 2: 3 * P + 9, 3: P}
    for off in sorted({o for o in plan["plane"] if o >= 0}):
        kind = {e & 3 for e, o in enumerate(plan["plane"]) if o == off}
        assert len(kind) == 1
        out.append((off, size[kind.pop()], f"plane at {off}"))
    for f, K in enumerate(Ks):
        out.append((plan["state"][f], 256, f"state {f}"))
        if plan["launch"][f] == launch:
            out += [(plan["tiles"][f], 12 * K * Tc * TILE, f"tiles {f}"), (plan["pts"][f], 12 * NMAX, f"pts {f}"), (plan["cnt"][f], 4 * K * Tc, f"cnt {f}")]
    return out


CASES = {
    "one frame": dict(slots=[0], Ks=[1], P=1),
    "three K": dict(slots=[5, 0, 2], Ks=[1, 3, 2], P=65 * 64),
    "shared planes": dict(slots=[0, 1, 2, 3], Ks=[3, 3, 3, 3], P=640 * 480, share=(0, 1, 2, 3), colour=(0, 1, 2, 3)),
    "mixed kinds": dict(slots=[7, 6, 1], Ks=[2, 64, 1], P=48 * 56, share=(0, 2), colour=(1, )),
    "two launches": dict(slots=[0, 1, 2, 3, 4], Ks=[3, 3, 1, 3, 2], P=640 * 480, budget=40 << 20),
}


def case_plan(c, Fcap=8):
    keys = keys_of(c["Ks"], c.get("share"), c.get("colour", ()))
    rows, cols = (1, c["P"]) if c["P"] < 4096 * 16 else (480, c["P"] // 480)
    return keys, B.rig_batch_plan(c["slots"], c["Ks"], rows, cols, keys, Fcap, c.get("budget", 0))


@pytest.mark.parametrize("name", list(CASES))
def test_plan_blocks_are_disjoint_aligned_and_inside_the_total(name):
    c = CASES[name]
    keys, plan = case_plan(c)
    assert plan is not None
    for launch in range(plan["n_launches"]):
        blocks = sorted(blocks_of(plan, c["slots"], c["Ks"], c["P"], keys, launch))
        for off, size, what in blocks:
            assert off % 256 == 0 and off % 8 == 0 and size > 0 and off + size <= plan["total"], what
        for (o0, s0, n0), (o1, _, n1) in zip(blocks, blocks[1:]):
            assert o0 + s0 <= o1, (n0, n1)
    # a frame's state block is its SLOT's, in front of everything else
    assert plan["state"] == [256 * s for s in c["slots"]] and plan["table"] == 256 * 8
    # frame f's camera records follow those of the frames in front of it
    lib_cam = (plan["cams"][1] - plan["cams"][0]) // c["Ks"][0] if len(c["Ks"]) > 1 else None
    if lib_cam:
        assert all(plan["cams"][f + 1] - plan["cams"][f] == lib_cam * c["Ks"][f] for f in range(len(c["Ks"]) - 1))


def test_the_state_block_depends_on_the_slot_alone():
    a = B.rig_batch_plan([3], [2], 48, 56, keys_of([2]), 8)
    b = B.rig_batch_plan([1, 3, 0], [1, 50, 3], 480, 640, keys_of([1, 50, 3]), 8)
    c = B.rig_batch_plan([0, 3], [3, 1], 1, 1, keys_of([3, 1]), 8)
    assert a["state"][0] == b["state"][1] == c["state"][1] == 256 * 3
    assert B.rig_batch_plan([3], [2], 48, 56, keys_of([2]), 16)["state"] == [768]


def test_a_plane_named_by_several_frames_appears_once():
    c = CASES["shared planes"]
    keys, plan = case_plan(c)
    # four colour frames of three cameras under one rig: three depth and three colour planes for all, an occluder plane of its own per frame and camera
    assert plan["n_planes"] == 3 + 3 + 12
    per_frame = [plan["plane"][12 * f:12 * f + 12] for f in range(4)]
    for f in range(1, 4):
        assert [per_frame[f][4 * k] for k in range(3)] == [per_frame[0][4 * k] for k in range(3)]
        assert [per_frame[f][4 * k + 2] for k in range(3)] == [per_frame[0][4 * k + 2] for k in range(3)]
        assert all(per_frame[f][4 * k + 3] != per_frame[0][4 * k + 3] for k in range(3)) and all(per_frame[f][4 * k + 1] == -1 for k in range(3))
    # the same key under another kind is another plane
    p = B.rig_batch_plan([0, 1], [1, 1], 8, 8, [64, 72, 0, 0, 72, 64, 0, 0], 4)
    assert p["n_planes"] == 4 and len(set(p["plane"]) - {-1}) == 4
    # the bytes: the header's formula
    r = lambda b: (b + 255) & ~255
    P = 640 * 480
    frame = r(12 * 3 * 75 * 4096) + r(12 * NMAX) + r(4 * 3 * 75)
    planes = 3 * r(2 * P) + 3 * r(3 * P + 16) + 12 * r(P + 16)
    first_plane = min(o for o in plan["plane"] if o >= 0)
    assert plan["tiles"][0] - first_plane == planes and [plan["tiles"][f + 1] - plan["tiles"][f] for f in range(3)] == [frame] * 3
    assert plan["total"] == plan["tiles"][0] + 4 * frame


def test_the_budget_rule_splits_the_frames_into_launches():
    c = CASES["two launches"]
    keys, plan = case_plan(c)
    r = lambda b: (b + 255) & ~255
    frame = lambda K: r(12 * K * 75 * 4096) + r(12 * NMAX) + r(4 * K * 75)
    fixed = plan["tiles"][0]
    # the rule, walked by hand: a frame that would push fixed + the launch's blocks beyond the budget starts the next launch
    want, cur, launch = [], 0, 0
    for K in c["Ks"]:
        if cur > 0 and fixed + cur + frame(K) > c["budget"]:
            launch, cur = launch + 1, 0
        want.append(launch); cur += frame(K)
    assert plan["launch"] == want and plan["n_launches"] == want[-1] + 1 and plan["n_launches"] >= 2
    # every launch's first frame lies at the end of the fixed part; the total is the fixed part and the largest launch
    firsts = [want.index(l) for l in range(plan["n_launches"])]
    assert all(plan["tiles"][f] == fixed for f in firsts)
    assert plan["total"] == fixed + max(sum(frame(K) for K, l in zip(c["Ks"], want) if l == m) for m in range(plan["n_launches"]))
    # a budget nothing fits still gives every frame a launch of its own; the library's own budget holds these five frames in one launch
    tiny = B.rig_batch_plan(c["slots"], c["Ks"], 480, 640, keys, 8, budget=1)
    assert tiny["launch"] == [0, 1, 2, 3, 4] and tiny["total"] == fixed + frame(3)
    assert B.rig_batch_plan(c["slots"], c["Ks"], 480, 640, keys, 8)["n_launches"] == 1
    # three 1280 x 720 cameras: about 33 MB a frame, so 1 GiB holds 30 frames a launch
    big = B.rig_batch_plan(list(range(32)), [3] * 32, 720, 1280, keys_of([3] * 32), 32)
    assert 32e6 < big["tiles"][1] - big["tiles"][0] < 35e6 and big["n_launches"] == 2 and big["total"] <= 1 << 30


def test_plan_refusals():
    k = keys_of([1, 1])
    ok = lambda slots, Ks, Fcap=4, rows=8, cols=8, keys=None: B.rig_batch_plan(slots, Ks, rows, cols, keys_of(Ks) if keys is None else keys, Fcap)
    assert ok([0, 1], [1, 1]) is not None
    assert ok([], []) is None and ok([0, 0], [1, 1]) is None and ok([0, 4], [1, 1]) is None and ok([0, -1], [1, 1]) is None
    assert ok([0, 1, 2, 3, 0], [1] * 5) is None                    # more frames than slots
    assert ok([0], [0], keys=[]) is None and ok([0], [65], keys=[1] * 260) is None
    assert ok([0], [64], rows=480, cols=640) is None and ok([0], [54], rows=480, cols=640) is not None      # 64 x 75 tiles > 4095 >= 54 x 75
    assert ok([0], [1], rows=0) is None
    lib = B.load_library()
    sl = np.array([0, 1], dtype=np.int32); Ka = np.array([1, 1], dtype=np.int32); ka = np.array(k, dtype=np.uint64); total = C.c_longlong(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = (None, ) * 7
    assert lib.tdlo_debug_rig_batch_plan(p(sl), p(Ka), 2, 4, 8, 8, p(ka), 0, *args, None, C.byref(total), None, None) == 0 and total.value == ok([0, 1], [1, 1])["total"]
    assert lib.tdlo_debug_rig_batch_plan(None, p(Ka), 2, 4, 8, 8, p(ka), 0, *args, None, C.byref(total), None, None) == B.TDLO_E_INVALID


def test_plan_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/rig_batch_plan_host_test.cpp: the plan header alone (no HIP), built with -fsanitize=address,undefined (the runtime linked into the program), run
    as a child process of its own on the cases above: it fills every block of every launch in a heap arena of exactly `total` bytes.  Nothing sanitized is
    loaded into python."""
    exe = str(tmp_path / "rig_batch_plan_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I" + os.path.join(ROOT, "trackdlo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "rig_batch_plan_host_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name, c in CASES.items():
        keys, plan = case_plan(c)
        # the program is given the library's own record sizes, read off the plan
        F = len(c["Ks"])
        cam = (plan["cams"][1] - plan["cams"][0]) // c["Ks"][0] if F > 1 else 192
        room = plan["cams"][0] - plan["table"]
        desc = room // F
        argv = [exe, "8", str(c["P"]), str(desc), str(cam), str(c.get("budget", 1 << 30))]
        e = 0
        for f in range(F):
            argv += [str(c["slots"][f]), str(c["Ks"][f])] + [str(k) for k in keys[e:e + 4 * c["Ks"][f]]]
            e += 4 * c["Ks"][f]
        r = subprocess.run(argv, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stdout + r.stderr)
        lines = r.stdout.split("\n")
        m = re.fullmatch(r"F=(\d+) table=(\d+) total=(\d+) planes=(\d+) launches=(\d+)", lines[0])
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(4)), int(m.group(5))) == (F, plan["table"], plan["n_planes"], plan["n_launches"]), name
        rows = [[int(x) for x in ln.split()] for ln in lines[1:1 + F]]
        assert [row[0] for row in rows] == plan["state"] and [row[5] for row in rows] == plan["launch"], name
        if F > 1:                                                  # (the library's own record sizes: the same arena to the byte)
            shift = rows[0][2] - plan["tiles"][0]
            assert abs(shift) < 256 * F + 256
            assert [[row[2] - shift, row[3] - shift, row[4] - shift] for row in rows] == [list(t) for t in zip(plan["tiles"], plan["pts"], plan["cnt"])], name
            assert int(m.group(3)) - shift == plan["total"], name
    r = subprocess.run([exe, "4", "64", "600", "192", "1000000", "0", "1", "8", "16", "0", "0", "0", "1", "24", "32", "0", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "refused" in r.stdout           # a slot named twice
    r = subprocess.run([exe, "1", "64", "600", "192", "1000000", "0", "1", "8", "16", "0", "0", "1", "1", "24", "32", "0", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "refused" in r.stdout           # more frames than slots


# ---- the routes of the GPU file's scenes, from the reference alone -----------------------------------------------------------------------------------
def test_the_reference_says_which_frames_are_served():
    L = S.LEAF
    for rows, cols in ((64, 64), (65, 64), (1, 1), (3, 5)):
        assert [BS.route(S.sized(rows, cols, K)[0], L) for K in (1, 2, 3)] == ["served"] * 3
    want = {"shared_cells": "served", "irrational": "served", "fused_boundary": "served", "minus_zero": "passed", "minus_zero colour": "passed",
            "border 32704": "served", "border 32705": "passed"}
    scenes = {"shared_cells": S.shared_cells(), "irrational": S.irrational(), "fused_boundary": S.fused_boundary(), "minus_zero": S.minus_zero(False),
              "minus_zero colour": S.minus_zero(True), "border 32704": S.border(32704), "border 32705": S.border(32705)}
    assert {k: BS.route(*v) for k, v in scenes.items()} == want
    assert R.rig_ref(*S.border(32704))[1] == NMAX and R.rig_ref(*S.border(32705))[1] == NMAX + 1
    # the companions are ordinary: served under the ordinary leaf at every size the GPU file uses
    for shape in ((65, 64), (56, 60), (40, 41), (48, 48), (128, 128)):
        routes = [BS.route(cams, L) for cams in BS.companions(*shape)]
        assert routes == (["served"] * 3 if shape != (128, 128) else ["served", "passed", "served"]), shape      # (three full 128 x 128 cameras keep 39 000 pixels)
    assert [BS.route(cams, 0.001) for cams in BS.companions(40, 52)] == ["served"] * 3
    # the mixed call: overflow() is served by the reference's rule (its second camera keeps one column), the crowded frame and the far one are passed on
    assert BS.route(S.overflow()[0], L) == "served" and R.rig_ref(*S.overflow())[1] == 40 * 41 + 40
    crowd = BS.crowded(40, 41)
    assert BS.route(crowd, L) == "passed" and R.rig_ref(crowd, L)[1] == len(crowd) * 40 * 41 > NMAX and len(crowd) * 1 <= 4095
    assert BS.route(BS.too_far(40, 41), L) == "passed"
    with pytest.raises(Exception):
        R.rig_ref(BS.too_far(40, 41), L)
    # the capacity case: served by the rule, more cells than a slot of 1024 points holds
    many = BS.many_cells()
    assert BS.route(many, BS.FINE) == "served" and R.rig_ref(many, BS.FINE)[0].shape[0] > 1024
    assert [BS.route(cams, BS.FINE) for cams in BS.companions(65, 64)] == ["served"] * 3
    # the ropes under one rig: every frame served, the ranges and masks tell the frames apart
    col, msk = BS.ropes_under_one_colour_rig(4, 2), BS.ropes_under_one_mask_rig(3, 2)
    assert BS.counts(col + msk, L) == [7, 0]
    assert len({R.rig_ref(f, L)[1] for f in col}) == 4 and len({R.rig_ref(f, L)[1] for f in msk}) == 3
    assert all(a.depth is b.depth and a.colour is b.colour for f in col[1:] for a, b in zip(f, col[0]))
    assert all(a.depth is b.depth and a.mask is not b.mask for f in msk[1:] for a, b in zip(f, msk[0]))
    # with the one-launch form off every frame is handed to the single call
    assert BS.counts(BS.companions(65, 64), L, fused=False) == [0, 3]


# ---- the binding's marshalling ----------------------------------------------------------------------------------------------------------------------
class StubLib:
    """Records what the binding hands to the two entry points and fills the outputs like the library would."""
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    @staticmethod
    def _frames(frames, F, rows, cols):
        out = []
        for f in (B.RigFrameC * F).from_address(addr(frames)) if F else []:
            cams = []
            for c in (B.RigCameraC * f.K).from_address(f.cams):
                P = rows * cols
                cams.append(dict(depth=c.depth, mask=c.mask, colour=c.colour, occluder=c.occluder, cam=(c.fx, c.fy, c.cx, c.cy),
                                 depth0=arr(c.depth, P, C.c_uint16), mask0=arr(c.mask, P, C.c_uint8) if c.mask else None,
                                 ranges=None if not c.colour_params else B.ColourParams.from_address(c.colour_params).n_ranges,
                                 T=None if not c.cam_to_rig else arr(c.cam_to_rig, 12, C.c_double)))
            out.append(dict(slot=f.slot, K=f.K, cams=cams))
        return out

    def tdlo_rig_to_cloud_batch(self, h, frames, F, rows, cols, leaf, n, nraw, rcs):
        self.calls.append(dict(h=h, F=F, rows=rows, cols=cols, leaf=leaf, frames=self._frames(frames, F, rows, cols)))
        for i in range(F):
            (C.c_int * 1).from_address(addr(n) + 4 * i)[0] = 10 + i
            (C.c_int * 1).from_address(addr(nraw) + 4 * i)[0] = 100 + i
        if F:
            (C.c_int * 1).from_address(addr(rcs) + 4 * (F - 1))[0] = self.rc
        return self.rc

    def tdlo_tracker_frames_from_rig_batch(self, tab, F, frames, rows, cols, leaf, d_vis, vis, nv, ext, ne, n, nraw, stats, rcs):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, rows=rows, cols=cols, leaf=leaf, d_vis=d_vis, frames=self._frames(frames, F, rows, cols)))
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


def small_rigs():
    rng = np.random.default_rng(3)
    d0 = rng.integers(400, 700, (3, 5)).astype(np.uint16); d1 = rng.integers(400, 700, (3, 5)).astype(np.uint16)
    m = [(rng.random((3, 5)) < 0.6).astype(np.uint8) * 255 for _ in range(3)]
    img = rng.integers(0, 256, (3, 5, 3)).astype(np.uint8)
    T = np.arange(12.0).reshape(3, 4)
    blue = B.make_colour_params(*S.RED_RANGE, rgb_order=0)
    a = [B.RigCamera(d0, mask=m[0], cam=(600.0, 601.0, 2.0, 1.0)), B.RigCamera(d1, mask=m[1], cam=(610.0, 611.0, 2.5, 1.5), cam_to_rig=T)]
    b = [B.RigCamera(d0, mask=m[2], cam=(600.0, 601.0, 2.0, 1.0))]                       # the same depth plane under another mask
    c = [B.RigCamera(d1, colour=img, params=blue, cam=(1.0, 2.0, 3.0, 4.0))]
    return (d0, d1, m, img, T), a, b, c


def test_rig_to_cloud_batch_marshalling(lib):
    ctx = stub_context(lib)
    ctx._async_src = None
    (d0, d1, m, img, T), a, b, c = small_rigs()
    n, nraw, codes = ctx.rig_to_cloud_batch([(5, a), (0, b), (3, c)], 0.008)
    k = lib.calls[-1]
    assert (k["h"], k["F"], k["rows"], k["cols"], k["leaf"]) == (0x1234, 3, 3, 5, 0.008)
    f = k["frames"]
    assert [(x["slot"], x["K"]) for x in f] == [(5, 2), (0, 1), (3, 1)]
    assert f[0]["cams"][0]["depth0"] == d0.reshape(-1).tolist() and f[0]["cams"][1]["depth0"] == d1.reshape(-1).tolist()
    assert f[0]["cams"][0]["mask0"] == m[0].reshape(-1).tolist() and f[1]["cams"][0]["mask0"] == m[2].reshape(-1).tolist()
    assert f[0]["cams"][0]["cam"] == (600.0, 601.0, 2.0, 1.0) and f[0]["cams"][1]["cam"] == (610.0, 611.0, 2.5, 1.5)
    assert f[0]["cams"][0]["T"] is None and f[0]["cams"][1]["T"] == T.reshape(-1).tolist()
    # a plane handed over as one object is one address, whichever frame names it
    assert f[0]["cams"][0]["depth"] == f[1]["cams"][0]["depth"] == d0.ctypes.data and f[2]["cams"][0]["depth"] == f[0]["cams"][1]["depth"] == d1.ctypes.data
    assert f[2]["cams"][0]["mask"] is None and f[2]["cams"][0]["colour"] == img.ctypes.data and f[2]["cams"][0]["ranges"] == 1 and f[0]["cams"][0]["ranges"] is None
    assert (n, nraw, codes) == ([10, 11, 12], [100, 101, 102], [0, 0, 0])
    keys, keep = B.rig_plane_keys([(5, a), (0, b), (3, c)])
    assert keys == [d0.ctypes.data, m[0].ctypes.data, 0, 0, d1.ctypes.data, m[1].ctypes.data, 0, 0, d0.ctypes.data, m[2].ctypes.data, 0, 0, d1.ctypes.data, 0, img.ctypes.data, 0]
    assert B.rig_batch_plan([5, 0, 3], [2, 1, 1], 3, 5, keys, 8)["n_planes"] == 6
    # a per-frame code: returned with check=False, raised otherwise
    lib.rc = B.TDLO_E_INVALID
    assert ctx.rig_to_cloud_batch([(0, a)], 0.008, check=False)[2] == [B.TDLO_E_INVALID]
    with pytest.raises(B.TdloError):
        ctx.rig_to_cloud_batch([(0, a)], 0.008)
    # rigs of two image sizes, or a rig without cameras, never reach the library
    ncalls = len(lib.calls)
    with pytest.raises(ValueError):
        ctx.rig_to_cloud_batch([(0, a), (1, [B.RigCamera(np.zeros((3, 6), np.uint16), mask=np.zeros((3, 6), np.uint8))])], 0.008)
    with pytest.raises(ValueError):
        ctx.rig_to_cloud_batch([(0, a), (1, [])], 0.008)
    assert len(lib.calls) == ncalls


def test_tracker_entrance_marshalling(lib):
    ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    (d0, d1, m, img, T), a, b, c = small_rigs()
    codes, vis, ext, n, nraw = B.frames_from_rig_batch(trk, [a, b, c], 0.008, 0.06)
    k = lib.calls[-1]
    assert k["trackers"] == [0x3000, 0x3001, 0x3002] and (k["F"], k["rows"], k["cols"], k["leaf"], k["d_vis"]) == (3, 3, 5, 0.008, 0.06)
    assert [x["K"] for x in k["frames"]] == [2, 1, 1] and k["frames"][1]["cams"][0]["mask0"] == m[2].reshape(-1).tolist()
    assert codes == [0, 0, 0] and [v.tolist() for v in vis] == [[0], [1], [2]] and [e.tolist() for e in ext] == [[0, 1], [1, 2], [2, 3]]
    assert n == [50, 51, 52] and nraw == [500, 501, 502] and [s["iters"] for s in trk[2].last_stats] == [304, 305]
    lib.rc = B.TDLO_E_EMPTY
    assert B.frames_from_rig_batch(trk, [a, b, c], 0.008, 0.06, check=False)[0] == [0, 0, B.TDLO_E_EMPTY]
    with pytest.raises(B.TdloError):
        B.frames_from_rig_batch(trk, [a, b, c], 0.008, 0.06)
    for t in trk:
        t.h = None           # (nothing for __del__ to destroy)
