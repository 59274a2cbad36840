"""tdlo_align_depth_batch and the aligning rig calls on the GPU (k_align_splat_batch / k_align_pack_batch, csrc/tdlo_align_batch.hip): every plane and every count
is compared on bits -- against the numpy statement (tests/align_ref.py through tests/align_batch_scenes.py), against tdlo_align_depth job by job, against the
composition by hand for the rig entrances; there is no tolerance anywhere.  Contexts are made under TDLO_ALIGN_BATCH_MIN=1 (the batch launches) unless a test
says otherwise; the route test runs both crossover values and the host route in child processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import align_batch_scenes as S
import align_ref as AR
import colour_ref
from test_prepass_gpu import make_ctx

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    return binding


@pytest.fixture(scope="module")
def synth():
    from trackdlo_amd import synth
    return synth


def bctx(frames=4, **env):
    e = {"TDLO_ALIGN_BATCH_MIN": 1}
    e.update(env)
    return make_ctx(e, max_frames=frames, max_points=1 << 15, max_nodes=64)


@pytest.fixture(scope="module")
def ctx():
    c = bctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def single():
    """the comparator: tdlo_align_depth job by job"""
    c = bctx()
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _Raw:
    def __init__(self, address, n):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr="<u2", data=(int(address), False), version=2)


def read_plane(torch, address, shape):
    """rows x cols uint16 at a device address"""
    n = int(shape[0]) * int(shape[1])
    return torch.as_tensor(_Raw(address, n), device="cuda").cpu().numpy().view(np.uint16).reshape(shape).copy()


def _view(B, torch, D, kind, device):
    """An ImageView of D laid out as `kind` (packed, pitched, bottom_up) in host or device memory"""
    buf, off, stride = AR.as_view_array(D, kind)
    owner = torch.from_numpy(buf.view(np.int16) if buf.dtype == np.uint16 else buf).cuda() if device else buf
    base = owner.data_ptr() if device else buf.ctypes.data
    v = B.ImageView(base + off, B.IMG_F32C1 if D.dtype == np.float32 else B.IMG_U16C1, B.MEM_DEVICE if device else B.MEM_HOST, stride, None)
    v.rows, v.cols, v.owner = D.shape[0], D.shape[1], owner
    return v


def make_jobs(B, torch, name):
    """the AlignJobC list of a scene list; a job with share = i names job i's view"""
    views, jobs = [], []
    for j in S.LISTS[name]:
        v = views[j["share"]] if j["share"] is not None else _view(B, torch, j["s"]["D"], j["kind"], j["where"] == "device")
        views.append(v)
        jobs.append(B.make_align_job(v, B.make_align_params(**j["s"]["p"])))
    return jobs


def check(name, planes, counts, order=None):
    refs = S.reference(name)
    order = list(range(len(refs))) if order is None else order
    for at, j in enumerate(order):
        A, n = refs[j]
        assert np.array_equal(np.asarray(planes[at]).reshape(A.shape), A) and counts[at] == n, (name, j, counts[at], n, int((np.asarray(planes[at]).reshape(A.shape) != A).sum()))


# ---- 1. every scene list ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.LISTS))
def test_scene_lists_against_the_statement_the_single_call_and_the_reversed_order(B, torch, ctx, single, name):
    jobs = make_jobs(B, torch, name)
    J = len(jobs)
    before = ctx.align_batch_route_counts()
    A, cnt, planes = ctx.align_depth_batch(jobs)                                      # host outputs
    check(name, A, cnt)
    assert ctx.align_batch_route_counts() == [before[0] + J, before[1], before[2]] and len(set(planes)) == J and all(p and p % 256 == 0 for p in planes)
    got = [read_plane(torch, planes[j], A[j].shape) for j in range(J)]                 # the arena's planes hold the same bits, all J together
    check(name, got, cnt)
    for j in range(J):                                                                 # tdlo_align_depth on job j alone
        G, gn, _ = single.align_depth(jobs[j].owner[0], jobs[j].owner[2])
        assert np.array_equal(G, A[j]) and gn == cnt[j], (name, j)
    dev = [torch.full((a.size,), 0x3c3c, dtype=torch.int16, device="cuda") for a in A]   # device outputs, the jobs in reversed order
    R, rcnt, _ = ctx.align_depth_batch(jobs[::-1], out=[d.data_ptr() for d in dev[::-1]])
    torch.cuda.synchronize()
    assert all(r is None for r in R)
    check(name, [d.cpu().numpy().view(np.uint16) for d in dev[::-1]], rcnt, order=list(range(J))[::-1])


# ---- 2. caller-provided device outputs between canaries -----------------------------------------------------------------------------------------------------
def test_device_outputs_between_canaries_and_the_device_planes(B, torch, ctx):
    """aligned_out in device memory at addresses aligned to 2 bytes but not to 4, and in host memory; the bytes on both sides of each stay; device_planes hold
    the same bits; an entry that is NULL receives nothing"""
    name = "mixed7"
    jobs = make_jobs(B, torch, name)
    refs = S.reference(name)
    bufs, outs = [], []
    for j, (A, _) in enumerate(refs):
        if j == 3:
            bufs.append(None); outs.append(None)
        elif j == 5:
            h = np.full(A.size + 16, 0xBEEF, np.uint16); bufs.append(h); outs.append(h[8:8 + A.size])
        else:
            d = torch.full((A.size + 16,), 0x5A5A, dtype=torch.int16, device="cuda")
            assert (d.data_ptr() + 2 * 7) % 4 == 2
            bufs.append(d); outs.append(d.data_ptr() + 2 * 7)
    _, cnt, planes = ctx.align_depth_batch(jobs, out=outs)
    torch.cuda.synchronize()
    for j, (A, n) in enumerate(refs):
        assert cnt[j] == n and np.array_equal(read_plane(torch, planes[j], A.shape), A), j
        if j == 3:
            continue
        if j == 5:
            h = bufs[j]
            assert np.array_equal(h[8:8 + A.size].reshape(A.shape), A) and (h[:8] == 0xBEEF).all() and (h[8 + A.size:] == 0xBEEF).all()
            continue
        got = bufs[j].cpu().numpy().view(np.uint16)
        assert np.array_equal(got[7:7 + A.size].reshape(A.shape), A) and (got[:7] == 0x5A5A).all() and (got[7 + A.size:] == 0x5A5A).all(), j


# ---- 3. layout changes on one context -------------------------------------------------------------------------------------------------------------------
def test_layout_changes_on_one_context_leave_no_stale_word(B, torch):
    c = bctx()
    try:
        a, b = AR.scene_downscale(), AR.scene_upscale()                                # A: every output pixel under four footprints; B: larger
        big = AR.scene_ratio20(64)                                                      # 300 x 400: grows the arena
        zero = dict(a, D=np.zeros_like(a["D"]))
        ref = {k: AR.align(s["D"], s["p"]) for k, s in dict(a=a, b=b, big=big, zero=zero).items()}
        sc = dict(a=a, b=b, big=big, zero=zero)

        def call(keys, device):
            jobs = [B.make_align_job(_view(B, torch, sc[k]["D"], "packed", device), B.make_align_params(**sc[k]["p"])) for k in keys]
            A, cnt, planes = c.align_depth_batch(jobs)
            for j, k in enumerate(keys):
                assert np.array_equal(A[j], ref[k][0]) and cnt[j] == ref[k][1], (keys, k)
            return planes

        call("ab", True)
        arena = c.align_batch_arena()
        call("ba", False)                                                               # the same bytes laid out the other way round: no fill
        assert c.align_batch_arena() == arena
        call(["b", "zero"], True)                                                       # A's place, an all-zero image: nothing of A's plane is left
        call(["a", "big", "b"], True)                                                   # grows the arena
        assert c.align_batch_arena()[1] > arena[1]
        planes = call("a", False)                                                       # A alone: its scratch lies where big's lay
        call(["zero", "zero"], True)
        planes = call(["a", "b"], True)
        # the single call has a plane of its own: it is still right, and the batch planes of the previous call still read back unchanged
        G, gn, plane = c.align_depth(big["D"], B.make_align_params(**big["p"]))
        assert np.array_equal(G, ref["big"][0]) and gn == ref["big"][1] and plane not in planes
        assert np.array_equal(read_plane(torch, planes[0], ref["a"][0].shape), ref["a"][0]) and np.array_equal(read_plane(torch, planes[1], ref["b"][0].shape), ref["b"][0])
        assert c.align_batch_route_counts() == [14, 0, 0] and c.align_route_counts() == [1, 0]
    finally:
        c.close()


# ---- 4. the no-wait form -----------------------------------------------------------------------------------------------------------------------------------
def _raw_rig(synth, K, frame=1, occluder=None, M=30):
    """A rig of K RGB-D cameras as their raw streams: every camera sees synth.colour_scene's frame at 120 x 160 (colour, occluder, mask) and delivers its depth
    at the depth sensor's 96 x 128 (the colour camera's rays at 0.8 of its focal length), under its own depth_to_colour and its own cam_to_rig.
    Returns (cameras [dict], Y0): D, p (align params as a dict), mask, colour, occ, cam, cam_to_rig"""
    depth_c, colour, occ, mask, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=frame, rows=120, cols=160, occluder=occluder)
    v = np.clip(np.rint((np.arange(96) + 0.5) / 0.8 - 0.5).astype(int), 0, 119)
    u = np.clip(np.rint((np.arange(128) + 0.5) / 0.8 - 0.5).astype(int), 0, 159)
    D = np.ascontiguousarray(depth_c[v][:, u])
    cams = []
    for k in range(K):
        T = AR.transform(AR.rot("z", 0.1 + 0.05 * k), (0.002 + 0.006 * k, 0.003 * k, 0.0))      # (a pixel or two apart: other footprints leave the image, the counts differ)
        p = AR.params(96, 128, (0.8 * cam["fx"], 0.8 * cam["fy"]), (0.8 * (cam["cx"] + 0.5) - 0.5, 0.8 * (cam["cy"] + 0.5) - 0.5), 120, 160, (cam["fx"], cam["fy"]),
                      (cam["cx"], cam["cy"]), T)
        to_rig = np.hstack([np.eye(3), np.array([[0.0004 * k], [-0.0003 * k], [0.0002 * k]])])
        cams.append(dict(D=D, p=p, mask=mask, colour=colour, occ=occ, cam=(cam["fx"], cam["fy"], cam["cx"], cam["cy"]), cam_to_rig=to_rig))
    return cams, Y0


def _rig_args(B, torch, cams, device, colour_rig=False, cp=None):
    """(RigCamera list without depth, AlignJobC list): device views as float32 metres, host views as pitched uint16"""
    rc, raw = [], []
    for q in cams:
        D = q["D"]
        src = torch.from_numpy((D / 1000.0).astype(np.float32)).cuda() if device else _view(B, torch, D, "pitched", False)
        raw.append(B.make_align_job(src, B.make_align_params(**q["p"])))
        if colour_rig:
            rc.append(B.RigCamera(None, colour=q["colour"], params=cp, occluder=q["occ"], cam=q["cam"], cam_to_rig=q["cam_to_rig"]))
        else:
            rc.append(B.RigCamera(None, mask=q["mask"], cam=q["cam"], cam_to_rig=q["cam_to_rig"]))
    return rc, raw


def _by_hand(B, torch, cb, rc, raw):
    """tdlo_align_depth per camera, each plane kept in a tensor of its own; the rig's cameras with those planes as device depth planes"""
    kept, counts, out = [], [], []
    for cm, j in zip(rc, raw):
        p = j.owner[2]
        t = torch.zeros((p.rows_c, p.cols_c), dtype=torch.int16, device="cuda")
        _, n, _ = cb.align_depth(j.owner[0], p, out=t.data_ptr())
        kept.append(t); counts.append(n)
        out.append(B.RigCamera(t, mask=cm.mask, colour=cm.colour, params=cm.params, occluder=cm.occluder, cam=cm.cam, cam_to_rig=cm.cam_to_rig))
    return out, counts, kept


def test_the_no_wait_form_in_front_of_a_rig_call(B, torch, synth, ctx, single):
    """all outputs NULL or device memory, counts NULL, then tdlo_rig_to_cloud on device_planes with no synchronisation by the test: the cloud of the waited
    composition, bit for bit"""
    cams, _ = _raw_rig(synth, 3)
    rc, raw = _rig_args(B, torch, cams, True)
    dev = torch.zeros((120, 160), dtype=torch.int16, device="cuda")
    A, cnt, planes = ctx.align_depth_batch(raw, out=[None, dev.data_ptr(), None], counts=False)
    assert A == [None, None, None] and cnt is None
    rig = [B.RigCamera(_DevPlane(planes[k], (120, 160)), mask=rc[k].mask, cam=rc[k].cam, cam_to_rig=rc[k].cam_to_rig) for k in range(3)]
    Xa, na, nrawa = ctx.rig_to_cloud(0, rig, 0.008)
    hand, counts, kept = _by_hand(B, torch, single, rc, raw)
    Xb, nb, nrawb = single.rig_to_cloud(0, hand, 0.008)
    assert (na, nrawa) == (nb, nrawb) and na > 100 and np.array_equal(_bits(Xa), _bits(Xb))
    assert np.array_equal(dev.cpu().numpy(), kept[1].cpu().numpy())
    for k in range(3):
        assert counts[k] == AR.align((cams[k]["D"] / 1000.0).astype(np.float32), cams[k]["p"])[1]


class _DevPlane:
    """what binding._batch_plane takes for a packed device plane: an address with a shape"""
    def __init__(self, address, shape):
        self.address, self.shape = int(address), tuple(shape)

    def data_ptr(self):
        return self.address

    def element_size(self):
        return 2

    def is_contiguous(self):
        return True


# ---- 5. ready_stream ------------------------------------------------------------------------------------------------------------------------------------
def test_ready_streams_of_two_jobs(B, torch, ctx):
    """each of two jobs' depth is filled on a stream of its own behind enough work that it has not run when the call is made"""
    sa, sb = AR.scene_upscale(), AR.scene_downscale()
    srcs = [torch.from_numpy(s["D"].view(np.int16)).cuda() for s in (sa, sb)]
    dsts = [torch.zeros_like(t) for t in srcs]
    bigs = [torch.ones((2048, 2048), device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(2):
        with torch.cuda.stream(sides[i]):
            for _ in range(20):
                bigs[i] = bigs[i] @ bigs[i] * 1e-4
            dsts[i].copy_(srcs[i])
    jobs = [B.make_align_job(B.image_view(dsts[i], format=B.IMG_U16C1, ready_stream=sides[i].cuda_stream), B.make_align_params(**s["p"])) for i, s in enumerate((sa, sb))]
    A, cnt, _ = ctx.align_depth_batch(jobs)
    for i, s in enumerate((sa, sb)):
        R, n = AR.align(s["D"], s["p"])
        assert np.array_equal(A[i], R) and cnt[i] == n, i
    torch.cuda.synchronize()


# ---- 6. routes ----------------------------------------------------------------------------------------------------------------------------------------------
_ROUTE_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import align_batch_scenes as S
import test_align_batch_gpu as T
from trackdlo_amd import binding as B
want = sys.argv[2]
c = B.Context(device=0, max_frames=1, max_points=1 << 14, max_nodes=64, timing=False)
total = 0
for name in S.SMALL:
    jobs = T.make_jobs(B, torch, name)
    A, cnt, planes = c.align_depth_batch(jobs)
    T.check(name, A, cnt)
    T.check(name, [T.read_plane(torch, planes[j], A[j].shape) for j in range(len(jobs))], cnt)
    total += len(jobs)
    r = [int(c.lib.tdlo_debug_route_count(c.h, k)) for k in range(59, 64)]
    assert r == dict(batch=[0, 0, total, 0, 0], loop=[total, 0, 0, total, 0], host=[0, total, 0, 0, 0])[want], (name, r)
c.close()
print("route ok", want, total)
"""


@pytest.mark.parametrize("want,env", [("batch", dict(TDLO_ALIGN_BATCH_MIN="1")), ("loop", dict(TDLO_ALIGN_BATCH_MIN="1025")), ("host", dict(TDLO_ALIGN="host"))])
def test_routes_in_a_child_process(want, env):
    """TDLO_ALIGN_BATCH_MIN=1 / =1025 and TDLO_ALIGN=host, each read when a fresh process makes its context: the same bits, counters 61 / 62 (and 59) / 60"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = {k: v for k, v in os.environ.items() if k not in ("TDLO_ALIGN", "TDLO_ALIGN_BATCH_MIN")}
    r = subprocess.run([sys.executable, "-c", _ROUTE_SCRIPT, root, want], env=dict(e, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "route ok " + want in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- 7. the rig entrances against the composition by hand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,device,colour_rig", [(2, True, False), (3, False, False), (3, True, True)], ids=["K2-mask-device", "K3-mask-host", "K3-colour-occluder"])
def test_rig_clouds_against_the_composition_by_hand(B, torch, synth, K, device, colour_rig):
    ca, cb = bctx(), bctx()
    try:
        cp = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
        cams, _ = _raw_rig(synth, K, occluder=(40, 100, 60, 72) if colour_rig else None)
        rc, raw = _rig_args(B, torch, cams, device, colour_rig, cp)
        Xa, na, nrawa, counts = ca.rig_to_cloud_aligning(0, rc, raw, 0.008)
        hand, counts_b, kept = _by_hand(B, torch, cb, rc, raw)
        Xb, nb, nrawb = cb.rig_to_cloud(0, hand, 0.008)
        assert counts == counts_b and (na, nrawa) == (nb, nrawb) and na > 100 and np.array_equal(_bits(Xa), _bits(Xb))
        assert len({tuple(c) for c in counts}) == K                                    # (the cameras' transforms differ: K different planes)
        assert ca.align_batch_route_counts() == [K, 0, K] and ca.rig_route_counts()[:2] == cb.rig_route_counts()[:2]
    finally:
        ca.close(); cb.close()


def targs(synth, M):
    P = synth.LAUNCH_PARAMS
    return (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])


def _state(t):
    return (t.get_tracking_result().copy(), t.get_sigma2(), [(s["iters"], s["converged"], s["n_kept"], s["status"]) for s in (t.last_stats or [])])


def _same_state(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.float64(a[1]).view(np.uint64) == np.float64(b[1]).view(np.uint64) and a[2] == b[2]


@pytest.mark.parametrize("painter", [False, True], ids=["plain", "rig-self-occlusion"])
def test_a_tracker_frame_from_a_raw_rig(B, torch, synth, painter):
    """nodes, sigma2 and the visible sets over three frames, K = 2; one run with tdlo_tracker_set_rig_self_occlusion on"""
    M = 30
    ca, cb = bctx(), bctx()
    try:
        ta, tb = B.trackdlo(*targs(synth, M), ctx=ca), B.trackdlo(*targs(synth, M), ctx=cb)
        for f in range(3):
            cams, Y0 = _raw_rig(synth, 2, frame=f, M=M)
            if f == 0:
                for t in (ta, tb):
                    t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
                    if painter:
                        t.set_rig_self_occlusion(None, 2, 10)
            rc, raw = _rig_args(B, torch, cams, f % 2 == 0)
            va, ea, na, nrawa, counts = ta.frame_from_rig_aligning(rc, raw, 0.008, 0.06)
            hand, counts_b, kept = _by_hand(B, torch, cb, rc, raw)
            vb, eb, nb, nrawb = tb.frame_from_rig(hand, 0.008, 0.06)
            assert list(va) == list(vb) and list(ea) == list(eb) and (na, nrawa) == (nb, nrawb) and counts == counts_b and na > 100, f
            assert _same_state(_state(ta), _state(tb)), f
        assert ca.align_batch_route_counts() == [6, 0, 6]
        assert [int(ca.lib.tdlo_debug_route_count(ca.h, k)) for k in (51, 52)] == [int(cb.lib.tdlo_debug_route_count(cb.h, k)) for k in (51, 52)]
    finally:
        ca.close(); cb.close()


def test_four_trackers_under_one_raw_rig(B, torch, synth):
    """F = 4 trackers under one K = 3 rig sharing the raw views: bit for bit tdlo_tracker_frames_from_rig_batch on hand-aligned planes; three planes are
    formed, not twelve; counts has twelve rows, the three distinct rows repeated"""
    M, F, K = 30, 4, 3
    ca, cb = bctx(), bctx()
    try:
        cams, Y0 = _raw_rig(synth, K, frame=1, M=M)
        coord = synth.geodesic_coord(Y0)
        ta = [B.trackdlo(*targs(synth, M), ctx=ca, slot=i) for i in range(F)]
        tb = [B.trackdlo(*targs(synth, M), ctx=cb, slot=i) for i in range(F)]
        for i in range(F):
            for t in (ta[i], tb[i]):
                t.initialize_nodes(Y0 + np.array([0.0, 0.0005 * i, 0.0])); t.initialize_geodesic_coord(coord)
        rc, raw = _rig_args(B, torch, cams, True)
        before = ca.align_batch_route_counts()
        codes, vis, ext, n, nraw, counts = B.frames_from_rig_aligning_batch(ta, [rc] * F, [raw] * F, 0.008, 0.06)
        moved = [a - b for a, b in zip(ca.align_batch_route_counts(), before)]
        assert moved == [K, 0, K] and codes == [0] * F
        hand, counts_b, kept = _by_hand(B, torch, cb, rc, raw)
        codes_b, vis_b, ext_b, n_b, nraw_b = B.frames_from_rig_batch(tb, [hand] * F, 0.008, 0.06)
        assert codes_b == codes and n == n_b and nraw == nraw_b and min(n) > 100
        assert len(counts) == F * K and counts == counts_b * F and len({tuple(c) for c in counts}) == K
        for i in range(F):
            assert np.array_equal(vis[i], vis_b[i]) and np.array_equal(ext[i], ext_b[i]) and np.array_equal(_bits(ca.get_cloud(i)), _bits(cb.get_cloud(i))), i
            assert _same_state(_state(ta[i]), _state(tb[i])), i
        # the same rig with one frame's camera under other params: four distinct jobs
        other = list(raw)
        other[2] = B.make_align_job(raw[2].owner[0], B.make_align_params(**dict(cams[2]["p"], max_footprint=5)))
        before = ca.align_batch_route_counts()
        B.frames_from_rig_aligning_batch(ta, [rc, rc, rc, rc], [raw, other, raw, raw], 0.008, 0.06)
        assert [a - b for a, b in zip(ca.align_batch_route_counts(), before)] == [K + 1, 0, K + 1]
    finally:
        ca.close(); cb.close()


# ---- 8. refusals touch nothing ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(B, torch, synth):
    M = 30
    c = bctx()
    try:
        cams, Y0 = _raw_rig(synth, 2, frame=0, M=M)
        t = B.trackdlo(*targs(synth, M), ctx=c, slot=0)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
        fresh = B.trackdlo(*targs(synth, M), ctx=c, slot=1)                            # a tracker without nodes
        lone = B.trackdlo(*targs(synth, M), ctx=c, slot=2)                             # a tracker with the single self-occlusion switch on
        lone.initialize_nodes(Y0); lone.initialize_geodesic_coord(synth.geodesic_coord(Y0))
        lone.set_self_occlusion(np.hstack([np.diag([cams[0]["cam"][0], cams[0]["cam"][1], 1.0]), np.zeros((3, 1))]), 10)
        rc, raw = _rig_args(B, torch, cams, True)
        t.frame_from_rig_aligning(rc, raw, 0.008, 0.06)
        jobs = make_jobs(B, torch, "same_view")
        refs = S.reference("same_view")
        _, _, planes = c.align_depth_batch(jobs, out=None, counts=False)                # the previous call whose planes must stay
        base, size = c.align_batch_arena()
        cloud, state = c.get_cloud(0), _state(t)[:2] + ([],)      # nodes and sigma2: what the LIBRARY holds (last_stats is the binding's record of the last call's outputs)
        counters = [int(c.lib.tdlo_debug_route_count(c.h, k)) for k in range(64)]
        up = AR.scene_upscale()
        D, pu = up["D"], up["p"]

        def untouched(what):
            assert [int(c.lib.tdlo_debug_route_count(c.h, k)) for k in range(64)] == counters, what
            assert c.align_batch_arena() == (base, size), what
            for j, (A, _) in enumerate(refs):
                assert np.array_equal(read_plane(torch, planes[j], A.shape), A), (what, j)
            assert np.array_equal(_bits(c.get_cloud(0)), _bits(cloud)) and _same_state(_state(t)[:2] + ([],), state), what

        def job(D=D, **over):
            return B.make_align_job(D, B.make_align_params(**dict(pu, **over)))

        good = job()
        odd = B.make_align_job(D, B.make_align_params(**pu)); odd.depth.data += 1
        fmt = B.make_align_job(D, B.make_align_params(**pu)); fmt.depth.format = B.IMG_U8C1
        liar = B.make_align_job(D, B.make_align_params(**pu)); liar.depth.location = B.MEM_DEVICE
        overlap = B.make_align_job(D, B.make_align_params(**pu)); overlap.depth.row_stride = 2 * D.shape[1] - 2      # rows that overlap
        inside = B.make_align_job(_DevView(B, planes[0], 48, 64), B.make_align_params(**pu))      # a device view that lies in the arena
        batch_cases = dict(
            none=[], too_many=[good] * 1025, bad_focal=[good, job(fx_d=0.0)], bad_T=[job(T=np.full((3, 4), np.nan)), good], footprint=[good, job(max_footprint=65)],
            no_rows=[job(rows_c=0)], overlapping_rows=[good, overlap], misaligned=[good, odd], wrong_format=[fmt], not_device=[good, liar],
            view_in_arena=[good, inside], budget=[job(rows_c=8192, cols_c=8192)] * 3)
        for what, js in batch_cases.items():
            with pytest.raises(B.TdloError) as e:
                c.align_depth_batch(js, out=None)
            assert e.value.code == B.TDLO_E_INVALID, what
            untouched(what)
        with pytest.raises(B.TdloError) as e:                                           # a device aligned_out that overlaps the arena
            c.align_depth_batch([good], out=[base + size - 64])
        assert e.value.code == B.TDLO_E_INVALID
        untouched("out in arena")
        if torch.cuda.device_count() > 1:                                               # a pointer on another GPU
            far = torch.zeros((48, 64), dtype=torch.int16, device="cuda:1")
            with pytest.raises(B.TdloError):
                c.align_depth_batch([good, B.make_align_job(B.image_view(far, format=B.IMG_U16C1), B.make_align_params(**pu))], out=None)
            untouched("another GPU")

        # ---- the rig entrances
        def rig_call(rc_, raw_, slot=0, leaf=0.008):
            return c.rig_to_cloud_aligning(slot, rc_, raw_, leaf)

        small = B.make_align_job(cams[1]["D"], B.make_align_params(**dict(cams[1]["p"], rows_c=119)))
        nothing = [rc[0], B.RigCamera(None, cam=rc[1].cam)]
        mixed = [rc[0], B.RigCamera(None, colour=cams[1]["colour"], params=B.make_colour_params(*colour_ref.LAUNCH_RANGE), cam=rc[1].cam)]
        bad_T = [rc[0], B.RigCamera(None, mask=cams[1]["mask"], cam=rc[1].cam, cam_to_rig=np.full((3, 4), np.inf))]
        rig_cases = dict(colour_size=lambda: rig_call(rc, [raw[0], small]), bad_params=lambda: rig_call(rc, [raw[0], job(fy_c=np.nan)]),
                         bad_view=lambda: rig_call(rc, [raw[0], odd]), bad_slot=lambda: rig_call(rc, raw, slot=99), bad_leaf=lambda: rig_call(rc, raw, leaf=-1.0),
                         neither=lambda: rig_call(nothing, raw), mixed_kinds=lambda: rig_call(mixed, raw), bad_cam_to_rig=lambda: rig_call(bad_T, raw),
                         raw_in_arena=lambda: rig_call(rc, [raw[0], B.make_align_job(_DevView(B, planes[0], 96, 128), B.make_align_params(**cams[1]["p"]))]),
                         tracker=lambda: t.frame_from_rig_aligning(rc, [raw[0], small]), tracker_leaf=lambda: t.frame_from_rig_aligning(rc, raw, -1.0),
                         no_nodes=lambda: fresh.frame_from_rig_aligning(rc, raw), single_switch=lambda: lone.frame_from_rig_aligning(rc, raw),
                         batch_size=lambda: B.frames_from_rig_aligning_batch([t], [rc], [[raw[0], small]], 0.008, 0.06),
                         batch_no_nodes=lambda: B.frames_from_rig_aligning_batch([t, fresh], [rc, rc], [raw, raw], 0.008, 0.06),
                         batch_switch=lambda: B.frames_from_rig_aligning_batch([t, lone], [rc, rc], [raw, raw], 0.008, 0.06),
                         batch_leaf=lambda: B.frames_from_rig_aligning_batch([t], [rc], [raw], 0.0, 0.06))
        for what, call in rig_cases.items():
            with pytest.raises(B.TdloError) as e:
                call()
            assert e.value.code == B.TDLO_E_INVALID, what
            untouched(what)
        # a camera that brings a depth plane (the binding refuses that itself: the library is called directly)
        tab, jtab, K, rows, cols, keep = B._rig_cameras_raw(rc, raw)
        tab[1].depth = cams[1]["D"].ctypes.data
        n = C.c_int(0); nraw = C.c_int(0)
        assert c.lib.tdlo_rig_to_cloud_aligning(c.h, 0, C.cast(tab, C.c_void_p), C.cast(jtab, C.c_void_p), K, rows, cols, 0.008, None, 0, C.byref(n), C.byref(nraw), None) == B.TDLO_E_INVALID
        untouched("a camera with a depth plane")
        # the context serves the next calls
        va, ea, na, nrawa, counts = t.frame_from_rig_aligning(rc, raw, 0.008, 0.06)
        assert na > 100 and counts[0] == AR.align((cams[0]["D"] / 1000.0).astype(np.float32), cams[0]["p"])[1]
        A, cnt, _ = c.align_depth_batch(jobs)
        check("same_view", A, cnt)
    finally:
        c.close()


def _DevView(B, address, rows, cols):
    v = B.ImageView(int(address), B.IMG_U16C1, B.MEM_DEVICE, 2 * cols, None)
    v.rows, v.cols = rows, cols
    return v
