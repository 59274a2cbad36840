"""tdlo_cloud_view_voxel_grid_batch / tdlo_set_cloud_view_batch and the two tracker entrances (k_cloud_view_batch, k_cloud_import_batch): every slot's cloud, n
and n_raw are those of the single call on that frame alone -- compared on bits (uint64 views) against the single calls on a second context, or against
tests/voxel_ref.py; there is no tolerance anywhere.  Contexts are made under TDLO_VIEW_BATCH_MIN=1; the route counters 38 / 39 / 40 / 41 are asserted in every
case, against what tests/view_batch_scenes.py says from the reference alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_prepass_gpu import make_ctx
from test_cloud_view_gpu import _layouts, _view
import view_batch_scenes as S
import voxel_ref

pytestmark = pytest.mark.gpu
LEAF = S.LEAF


def bctx(frames=16, points=1 << 15, **env):
    e = {"TDLO_VIEW_BATCH_MIN": 1}
    e.update(env)
    return make_ctx(e, max_frames=frames, max_points=points, max_nodes=64)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ca():
    c = bctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def cb():
    """The comparator: the single calls."""
    c = bctx()
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(np.asfortranarray(a, dtype=np.float64).T).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def run_voxel(ca, cb, frames, leaf=LEAF, label=""):
    """frames: (slot, view-or-array, select).  The batch on ca, the single calls on cb (same slots); clouds, n, n_raw compared on bits.  Returns (n, n_raw)."""
    before = ca.view_batch_route_counts()
    n, nraw, codes = ca.voxel_grid_view_batch(frames, leaf)
    assert codes == [0] * len(frames), (label, codes)
    for i, (slot, view, sel) in enumerate(frames):
        _, n1, nraw1 = cb.voxel_grid_view(slot, view, leaf, select=sel, want_cloud=False)
        assert (n[i], nraw[i]) == (n1, nraw1), (label, i, n[i], nraw[i], n1, nraw1)
        assert same_bits(ca.get_cloud(slot), cb.get_cloud(slot)), (label, i)
    after = ca.view_batch_route_counts()
    return n, nraw, [a - b for a, b in zip(after, before)]


def test_sizes_in_one_call(ca, cb):
    """N = 1 .. 8193 in ONE call: the last word of a view, the tile border, frames of one and three tiles side by side (workgroups beyond a frame's tiles
    leave); then with the slots reversed, so that every slot held another (often larger) cloud before."""
    clouds = [S.rope(N, 40 + k) for k, N in enumerate(S.SIZES)]
    want = S.counts([(P, None) for P in clouds])
    assert want == [len(clouds), 0]
    for order in (list(range(8)), list(range(7, -1, -1)), list(range(8))):
        frames = [(order[k], clouds[k], None) for k in range(8)]
        n, nraw, d = run_voxel(ca, cb, frames, label=f"slots {order}")
        assert d == [8, 0, 0, 0], d
        assert nraw == list(S.SIZES)
        for k, P in enumerate(clouds):
            X, _ = voxel_ref.voxel_ref(P, None, LEAF)
            assert same_bits(ca.get_cloud(order[k]), X), k


def test_forms_in_one_call(ca, cb, torch):
    """Every load form in one call: float64, float32 at point strides 3 / 4 / 8, column-major pairs with odd and even N, odd and negative strides, host and
    device mixed, NaN in every element the views do not address."""
    from trackdlo_amd import binding as B
    for N in (257, 4098):
        rng = np.random.default_rng(50 + N)
        frames, keep = [], []
        for k, (name, flat, off, sp, sc) in enumerate(_layouts(N, rng)):
            flat *= np.asarray(0.05, dtype=flat.dtype)                   # (a compact cloud; NaN stays NaN)
            if k % 2:
                t = dev(torch, flat)
                keep.append(t)
                v = _view(B, t.data_ptr() + off * flat.itemsize, flat.dtype, sp, sc, N, t, B.MEM_DEVICE if k % 4 == 1 else B.MEM_AUTO)
            else:
                v = _view(B, flat.ctypes.data + off * flat.itemsize, flat.dtype, sp, sc, N, flat)
            frames.append((k, v, None))
        torch.cuda.synchronize()
        assert len(frames) == 14
        n, nraw, d = run_voxel(ca, cb, frames, label=f"forms N={N}")
        assert d == [14, 0, 0, 0] and nraw == [N] * 14, (d, nraw)
    # column-major pairs with an odd N: the last element is loaded on its own
    N = 4099
    P = S.rope(N, 61)
    cols = np.asfortranarray(np.full((N + 1, 3), np.nan, dtype=np.float32))
    cols[:N] = P
    v = _view(B, cols.ctypes.data, np.float32, 1, N + 1, N, cols)
    t = dev(torch, cols.T.reshape(-1))
    vd = _view(B, t.data_ptr(), np.float32, 1, N + 1, N, t, B.MEM_DEVICE)
    n, nraw, d = run_voxel(ca, cb, [(0, v, None), (1, vd, None)], label="odd pairs")
    assert d == [2, 0, 0, 0] and nraw == [N, N]
    X, _ = voxel_ref.voxel_ref(P, None, LEAF)
    assert same_bits(ca.get_cloud(0), X) and same_bits(ca.get_cloud(1), X)


def test_selections(ca, cb, torch):
    """No selection, host selections, device selections starting 1, 2, 3 bytes into their allocation with set bytes around them, and three frames selecting
    disjoint ropes out of ONE organized view (host and device)."""
    P, sels = S.organized()
    N = len(P)
    assert S.counts([(P, s) for s in sels] + [(P, None)]) == [4, 0]
    frames = [(0, P, sels[0]), (1, P, sels[1]), (2, P, sels[2]), (3, P, None)]
    n, nraw, d = run_voxel(ca, cb, frames, label="one host view, three ropes")
    assert d == [4, 0, 0, 0]
    for k in range(3):
        X, r = voxel_ref.voxel_ref(P, sels[k], LEAF)
        assert nraw[k] == r and same_bits(ca.get_cloud(k), X), k
    tP = dev(torch, P)
    dsel, frames = [], []
    for k in range(3):
        buf = torch.full((N + 8,), 255, dtype=torch.uint8, device="cuda")
        buf[k + 1:k + 1 + N] = torch.from_numpy(np.array(sels[k])).cuda()
        dsel.append(buf)
        frames.append((4 + k, tP, buf[k + 1:k + 1 + N]))
    frames.append((7, tP, sels[0]))                                         # a device view under host selection bytes
    torch.cuda.synchronize()
    n2, nraw2, d = run_voxel(ca, cb, frames, label="one device view, unaligned device selections")
    assert d == [4, 0, 0, 0] and nraw2 == nraw[:3] + [nraw[0]] and n2 == n[:3] + [n[0]]
    for k in range(3):
        assert same_bits(ca.get_cloud(4 + k), ca.get_cloud(k)), k


def test_borders_of_the_in_lds_sort(ca, cb):
    """32 704 kept points served, 32 705 passed on; rb + kb = 33, pass-through and a view above 1 048 576 elements passed on; a frame keeping nothing;
    non-finite points dropped; -0.0f -- each among served frames, whose results must not move."""
    sc = S.borders()
    Pb, sb = S.big_view()
    frames = [(k, P, sel) for k, (_, P, sel) in enumerate(sc)] + [(len(sc), Pb, sb)]
    want = S.counts([(P, sel) for _, P, sel in sc] + [(Pb, sb)])
    assert want == [6, 4]
    n, nraw, d = run_voxel(ca, cb, frames, label="borders")
    assert d == want + [0, 0], d
    names = [s[0] for s in sc]
    assert nraw[names.index("32704 kept")] == S.NMAX and nraw[names.index("32705 kept")] == S.NMAX + 1
    k0 = names.index("keeps nothing")
    assert (n[k0], nraw[k0]) == (0, 0) and ca.get_cloud(k0).shape[0] == 0
    for k, (name, P, sel) in enumerate(sc):
        if S.route(P, sel) == "served" or name in ("pass-through", "rb + kb = 33"):
            X, r = voxel_ref.voxel_ref(P, sel, LEAF)
            assert nraw[k] == r and same_bits(ca.get_cloud(k), X), name
    X = ca.get_cloud(names.index("non-finite, -0.0f"))
    z = X[(X[:, 0] == 0) & (X[:, 1] == 0)]
    assert len(z) == 1 and not np.signbit(z[0, :2]).any()                     # a cell of -0.0f only comes out +0.0 (CentroidPoint starts from 0.0f)
    # ... and the served frames alone give the same clouds
    alone = [(k, P, sel) for k, (_, P, sel) in enumerate(sc) if S.route(P, sel) == "served"]
    got = {k: ca.get_cloud(k) for k, _, _ in alone}
    n3, nraw3, d = run_voxel(ca, cb, alone, label="the served frames alone")
    assert d == [6, 0, 0, 0]
    for k, _, _ in alone:
        assert same_bits(ca.get_cloud(k), got[k]), k


@pytest.mark.parametrize("F", [1, 2, 8])
def test_batch_sizes(ca, cb, F):
    """F = 1, 2, 8, a single-tile frame first and last."""
    sizes = [5] + [8193, 4097, 700, 4096, 9000, 1, 12289][:max(F - 2, 0)] + ([300] if F > 1 else [])
    frames = [(k, S.rope(N, 70 + k), None) for k, N in enumerate(sizes)]
    assert len(frames) == F
    n, nraw, d = run_voxel(ca, cb, frames, label=f"F={F}")
    assert d == [F, 0, 0, 0] and nraw == sizes


def test_refusals_touch_nothing(ca, torch):
    from trackdlo_amd import binding as B
    P = [S.rope(500, 80), S.rope(600, 81)]
    ca.voxel_grid_view_batch([(0, P[0], None), (1, P[1], None)], LEAF)
    held = [ca.get_cloud(0), ca.get_cloud(1)]
    from trackdlo_amd import synth
    t0 = B.trackdlo(*targs(), ctx=ca, slot=0)
    t0.initialize_nodes(synth.nodes(M)); t0.initialize_geodesic_coord(synth.geodesic_coord(synth.nodes(M)))
    nodes = t0.get_tracking_result().copy()
    before = (ca.view_batch_route_counts(), ca.view_route_counts(), ca.voxel_view_calls())
    xraw = dev(torch, np.zeros((4, 3), dtype=np.float32))
    bad = B.cloud_view(P[1]); bad.stride_comp = 0
    asyn = B.cloud_view(xraw, asynchronous=True)

    def refused(frames, leaf=LEAF):
        with pytest.raises(B.TdloError) as e:
            ca.voxel_grid_view_batch(frames, leaf)
        assert e.value.code == B.TDLO_E_INVALID
        n, nraw, codes = ca.voxel_grid_view_batch(frames, leaf, check=False)
        assert n == [0] * len(frames) and codes == [0] * len(frames)          # (refused as a whole: no per-frame code)

    refused([(0, P[0], None), (0, P[1], None)])                                # a slot named twice
    refused([(0, P[0], None), (99, P[1], None)])                               # a slot out of range
    refused([(0, P[0], None), (1, asyn, None)])                                # TDLO_VIEW_ASYNC
    refused([(0, P[0], None), (1, bad, None)])                                 # a bad view in the last frame
    refused([(0, P[0], None)], leaf=0.0)
    refused([(0, P[0], None)], leaf=float("inf"))
    refused([(k, P[0], None) for k in range(17)])                              # more frames than slots
    # a device view over the resident clouds of slots the call names.  A slot's address is not public, so the test cannot aim at ONE slot's cloud (and so cannot
    # tell "any named slot" from "its own slot": that the check walks every named slot is read in view_batch_refusal, not shown here).  Two views of two
    # elements each reach 2^46 bytes up and 2^46 bytes down from a small tensor; whichever side of the tensor the slots' clouds lie on, at least one of the two
    # spans them and must be refused.  The far element is deselected, so a call that goes through loads the tensor's own three floats and nothing else
    # (tdlo_view_lane.h: an element is loaded only where its selection byte is set)
    small = dev(torch, np.array([[0.1, 0.2, 0.6]], dtype=np.float32))
    torch.cuda.synchronize()
    only_first = np.array([1, 0], dtype=np.uint8)
    verdicts = []
    for sp in (1 << 44, -(1 << 44)):
        over = B.CloudView(small.data_ptr(), B.F32, B.MEM_DEVICE, sp, 1, None, 0); over.N = 2; over.owner = small
        frames = [(1, over, only_first), (0, P[0], None)]
        try:
            ca.voxel_grid_view_batch(frames, LEAF)
            verdicts.append(0)
            ca.voxel_grid_view_batch([(0, P[0], None), (1, P[1], None)], LEAF)      # (it went through: the two clouds as they were, for what follows)
            before = (ca.view_batch_route_counts(), ca.view_route_counts(), ca.voxel_view_calls())
        except B.TdloError as e:
            assert e.code == B.TDLO_E_INVALID
            verdicts.append(1)
    assert sum(verdicts) >= 1, verdicts
    with pytest.raises(B.TdloError) as e:
        ca.set_cloud_view_batch([0, 0], [P[0], P[1]])
    assert e.value.code == B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ca.set_cloud_view_batch([0, 1], [P[0], asyn])
    with pytest.raises(B.TdloError):
        ca.set_cloud_view_batch([0, 1], [P[0], bad])
    with pytest.raises(B.TdloError):
        B.frames_from_cloud_view_batch([t0], [bad], LEAF, 0.06)
    assert (ca.view_batch_route_counts(), ca.view_route_counts(), ca.voxel_view_calls()) == before
    assert same_bits(ca.get_cloud(0), held[0]) and same_bits(ca.get_cloud(1), held[1])
    assert np.array_equal(t0.get_tracking_result(), nodes)


def test_a_frame_that_fails_on_its_own(ca, cb):
    """A cloud too far from the origin for the leaf (case 8): its code in rc_each, the call returns it, the others complete."""
    from trackdlo_amd import binding as B
    frames = [(0, S.rope(4097, 90), None), (1, S.far_cloud(), None), (2, S.rope(5, 91), None)]
    assert S.counts([(f[1], None) for f in frames]) == [2, 1]
    before = ca.view_batch_route_counts()
    with pytest.raises(B.TdloError) as e:
        ca.voxel_grid_view_batch(frames, LEAF)
    assert e.value.code == B.TDLO_E_INVALID
    n, nraw, codes = ca.voxel_grid_view_batch(frames, LEAF, check=False)
    assert codes == [0, B.TDLO_E_INVALID, 0]
    assert [a - b for a, b in zip(ca.view_batch_route_counts(), before)] == [4, 2, 0, 0]
    for k in (0, 2):
        X, r = voxel_ref.voxel_ref(frames[k][1], None, LEAF)
        assert nraw[k] == r and same_bits(ca.get_cloud(k), X), k
    with pytest.raises(B.TdloError):
        cb.voxel_grid_view(1, S.far_cloud(), LEAF)


def test_single_calls_after_a_batch_and_a_batch_after_single_calls(ca, cb):
    """On ONE context: the arming of both routes' state words survives either order."""
    A, Bc = S.rope(4097, 95), S.rope(9000, 96)
    want = [voxel_ref.voxel_ref(P, None, LEAF)[0] for P in (A, Bc)]
    for rnd in range(2):
        d0 = ca.view_batch_route_counts(); s0 = ca.view_route_counts()
        ca.voxel_grid_view_batch([(0, A, None), (1, Bc, None)], LEAF)
        assert same_bits(ca.get_cloud(0), want[0]) and same_bits(ca.get_cloud(1), want[1]), rnd
        X, _, _ = ca.voxel_grid_view(1, A, LEAF)
        assert same_bits(X, want[0]), rnd
        X, _, _ = ca.voxel_grid_view(0, Bc, LEAF)
        assert same_bits(X, want[1]), rnd
        ca.set_cloud_view(2, A)
        assert [a - b for a, b in zip(ca.view_batch_route_counts(), d0)] == [2, 0, 0, 0]
        assert [a - b for a, b in zip(ca.view_route_counts(), s0)][:2] == [2, 0]


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from trackdlo_amd import binding as B
import view_batch_scenes as S
one_by_one = sys.argv[3] == "one-by-one"
ctx = B.Context(device=0, max_frames=8, max_points=1 << 15, max_nodes=64, timing=False)
frames = [(k, S.rope(N, 40 + k), None) for k, N in enumerate(S.SIZES)]
imports = ([0, 1], [S.rope(257, 1), S.rope(5, 2)])
def voxel():
    if not one_by_one:
        return ctx.voxel_grid_view_batch(frames, S.LEAF)[:2]
    r = [ctx.voxel_grid_view_batch([f], S.LEAF) for f in frames]
    return [x[0][0] for x in r], [x[1][0] for x in r]
n, nraw = voxel()
if one_by_one:
    for s, P in zip(*imports):
        ctx.set_cloud_view_batch([s], [P])
else:
    ctx.set_cloud_view_batch(*imports)
out = [ctx.get_cloud(k) for k in range(8)]
voxel()
routes, single = ctx.view_batch_route_counts(), ctx.view_route_counts()
X = {f"X{k}": ctx.get_cloud(k) for k in range(8)}
ctx.voxel_grid_view_batch(frames[:2], S.LEAF); ctx.set_cloud_view_batch(*imports)       # two frames in one call: what the library's own crossover does with them
np.savez(sys.argv[2], n=n, nraw=nraw, routes=routes, single=single, two=ctx.view_batch_route_counts(), I0=out[0], I1=out[1], **X)
ctx.close()
"""


@pytest.mark.parametrize("env", [{"TDLO_VIEW_BATCH_MIN": None}, {"TDLO_VIEW_BATCH_MIN": "1000"}, {"TDLO_VIEW_BATCH_MIN": "1", "TDLO_CLOUD_FUSED": "0"}],
                         ids=["min-unset", "min-large", "fused-off"])
def test_comparator_routes_give_the_same_bits(tmp_path, env):
    """TDLO_VIEW_BATCH_MIN unset or large, and TDLO_CLOUD_FUSED=0, each in a child process: the same bits through the single route.  Unset, the bare calls take
    the batch launches from two frames on (kViewBatchMin), so that child hands its frames over one call at a time -- and then two in one call, which must take
    the batch launches."""
    e = dict(os.environ)
    for k, v in env.items():
        if v is None:
            e.pop(k, None)
        else:
            e[k] = v
    unset = env.get("TDLO_VIEW_BATCH_MIN") is None
    out = str(tmp_path / "r.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out, "one-by-one" if unset else "together"], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    for k, N in enumerate(S.SIZES):
        X, nr = voxel_ref.voxel_ref(S.rope(N, 40 + k), None, LEAF)
        assert z["nraw"][k] == nr and z["n"][k] == X.shape[0] and same_bits(z[f"X{k}"], X), (env, k)
    assert same_bits(z["I0"], S.rope(257, 1).astype(np.float64)) and same_bits(z["I1"], S.rope(5, 2).astype(np.float64))
    routes, single, two = [int(v) for v in z["routes"]], [int(v) for v in z["single"]][:2], [int(v) for v in z["two"]]
    if env.get("TDLO_CLOUD_FUSED") == "0":
        assert routes == [0, 16, 2, 0] and single == [0, 0]      # every frame handed to the single call, which takes the multi-launch form
    else:
        assert routes == [0, 0, 0, 2] and single == [16, 0]      # the single route: the one-launch kernel of the single call served every frame
    if unset:
        assert two == [2, 0, 2, 2]                               # the library's own crossover: two frames in one call are the batch launches
    elif env.get("TDLO_VIEW_BATCH_MIN") == "1000":
        assert two == [0, 0, 0, 4]


@pytest.mark.parametrize("N", [1, 3, 255, 256, 257, 4099])
def test_the_import_in_one_call(ca, cb, torch, N):
    """tdlo_set_cloud_view_batch: every layout of tests/test_cloud_view_gpu.py at N, host and device mixed, in ONE call, against tdlo_set_cloud_view."""
    from trackdlo_amd import binding as B
    import cloud_view_ref as R
    rng = np.random.default_rng(2000 + N)
    views, want, keep = [], [], []
    for k, (name, flat, off, sp, sc) in enumerate(_layouts(N, rng)):
        want.append(R.widen(flat, flat.dtype, off, sp, sc, N))
        if k % 2 == 0:
            t = dev(torch, flat)
            keep.append(t)
            views.append(_view(B, t.data_ptr() + off * flat.itemsize, flat.dtype, sp, sc, N, t, B.MEM_DEVICE))
        else:
            views.append(_view(B, flat.ctypes.data + off * flat.itemsize, flat.dtype, sp, sc, N, flat))
    torch.cuda.synchronize()
    F = len(views)
    before = ca.view_batch_route_counts()
    slots = list(range(F - 1, -1, -1))
    assert ca.set_cloud_view_batch(slots, views) == [0] * F
    assert [a - b for a, b in zip(ca.view_batch_route_counts(), before)] == [0, 0, F, 0]
    for k in range(F):
        cb.set_cloud_view(slots[k], views[k])
        assert same_bits(ca.get_cloud(slots[k]), want[k]) and same_bits(cb.get_cloud(slots[k]), want[k]), (N, k)


def test_the_import_sizes_and_the_copy_route(torch):
    """Frames of 1 .. 8193 points in one import; non-finite values as (double) widens them; TDLO_VIEW_INPLACE=0 copies the packed views first: the same bits."""
    for env in ({}, {"TDLO_VIEW_INPLACE": 0}):
        c = bctx(**env)
        try:
            clouds = [np.array(S.rope(N, 40 + k)) for k, N in enumerate(S.SIZES)]
            clouds[4][7] = [np.nan, np.inf, -0.0]
            views = [dev(torch, P) if k % 3 == 0 else P for k, P in enumerate(clouds)]
            torch.cuda.synchronize()
            assert c.set_cloud_view_batch(list(range(8)), views) == [0] * 8
            assert c.view_batch_route_counts() == [0, 0, 8, 0]
            for k, P in enumerate(clouds):
                assert same_bits(c.get_cloud(k), P.astype(np.float64)), (env, k)
        finally:
            c.close()


# ---- trackers -------------------------------------------------------------------------------------------------------------------------------------
M, D_VIS = 30, 0.06


def targs():
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    return (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])


_ROPE = {}


def rope_clouds():
    """Four frames of one rope in motion as float32 clouds: the points of the masked pixels of synth.depth_scene, a few thousand each."""
    from trackdlo_amd import synth
    if not _ROPE:
        out = []
        for i in range(4):
            depth, mask, cam, _ = synth.depth_scene(M, config=20, frame=i)
            P = voxel_ref.backproject(depth, mask, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
            P.setflags(write=False)
            out.append(P)
        _ROPE["c"] = out
        _ROPE["cam"] = cam
    return _ROPE["c"]


def make_trackers(ctx, n):
    from trackdlo_amd import binding as B, synth
    Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
    out = []
    for i in range(n):
        t = B.trackdlo(*targs(), ctx=ctx, slot=i)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        out.append(t)
    return out


def state(t):
    return (t.get_tracking_result().copy(), t.get_sigma2(), [(s["iters"], s["converged"], s["n_kept"], s["status"]) for s in (t.last_stats or [])])


def assert_same_state(a, b, label):
    assert same_bits(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], (label, a[1], b[1], a[2], b[2])


def tctx():
    return bctx(frames=8, points=1 << 14, TDLO_ESTEP2=0)


@pytest.mark.parametrize("F", [3, 8])
def test_tracker_frames_from_cloud_views(torch, F):
    """frames_from_cloud_view_batch against twins on another context stepped by frame_from_cloud_view: nodes, sigma2, visible sets, n / n_raw bit for bit, two
    frames; the self-occlusion switch on for one of them; host and device views mixed."""
    from trackdlo_amd import binding as B
    xa, xb = tctx(), tctx()
    try:
        ta, tb = make_trackers(xa, F), make_trackers(xb, F)
        rc = rope_clouds()
        cam = _ROPE["cam"]
        proj = np.array([[cam["fx"], 0, cam["cx"], 0], [0, cam["fy"], cam["cy"], 0], [0, 0, 1, 0]], dtype=np.float64)
        ta[1].set_self_occlusion(proj, 10); tb[1].set_self_occlusion(proj, 10)
        for step in range(2):
            clouds = [rc[(i + step) % 4] for i in range(F)]
            views = [dev(torch, P) if i % 2 else P for i, P in enumerate(clouds)]
            torch.cuda.synchronize()
            codes, vis, ext, n, nraw = B.frames_from_cloud_view_batch(ta, views, LEAF, D_VIS)
            assert codes == [0] * F and xa.view_batch_route_counts() == [F * (step + 1), 0, 0, 0]
            for i in range(F):
                v1, e1, n1, nraw1 = tb[i].frame_from_cloud_view(views[i], LEAF, D_VIS)
                assert (n1, nraw1) == (n[i], nraw[i]) and np.array_equal(v1, vis[i]) and np.array_equal(e1, ext[i]), (step, i)
                assert same_bits(xa.get_cloud(i), xb.get_cloud(i)), (step, i)
                assert_same_state(state(ta[i]), state(tb[i]), f"step {step}, tracker {i}")
                assert ta[i].last_stats[1]["iters"] > 0
    finally:
        xa.close(); xb.close()


@pytest.mark.parametrize("F", [3, 8])
def test_tracker_steps_on_cloud_views(torch, F):
    """tracking_step_view_batch -- k_cloud_import_batch enqueued without a wait, tracking_step_batch behind it -- against twins on another context stepped by
    tracking_step_view: clouds, nodes, sigma2 and iteration counts bit for bit, three frames; host and device views mixed."""
    from trackdlo_amd import binding as B
    xa, xb = tctx(), tctx()
    try:
        ta, tb = make_trackers(xa, F), make_trackers(xb, F)
        rc = rope_clouds()
        vis = [np.arange(M, dtype=np.int32)] * F
        for step in range(3):
            down = [voxel_ref.voxel_ref(rc[(i + step) % 4], None, LEAF)[0].astype(np.float32) for i in range(F)]
            views = [dev(torch, P) if i % 3 == 1 else P for i, P in enumerate(down)]
            torch.cuda.synchronize()
            assert B.tracking_step_view_batch(ta, views, vis, vis) == [0] * F
            assert xa.view_batch_route_counts() == [0, 0, F * (step + 1), 0]
            for i in range(F):
                tb[i].tracking_step_view(views[i], vis[i], vis[i])
                assert same_bits(xa.get_cloud(i), down[i].astype(np.float64)) and same_bits(xa.get_cloud(i), xb.get_cloud(i)), (step, i)
                assert_same_state(state(ta[i]), state(tb[i]), f"step {step}, tracker {i}")
                assert ta[i].last_stats[1]["iters"] > 0
        assert xb.view_batch_route_counts() == [0, 0, 0, 0]
    finally:
        xa.close(); xb.close()


def test_a_tracker_whose_view_keeps_nothing_is_left_alone():
    from trackdlo_amd import binding as B
    xa, xb = tctx(), tctx()
    try:
        ta, tb = make_trackers(xa, 4), make_trackers(xb, 4)
        rc = rope_clouds()
        sels = [None, None, np.zeros(len(rc[2]), dtype=np.uint8), None]
        before = state(ta[2])
        codes, vis, ext, n, nraw = B.frames_from_cloud_view_batch(ta, rc, LEAF, D_VIS, selects=sels, check=False)
        assert codes == [0, 0, B.TDLO_E_EMPTY, 0] and n[2] == 0 and nraw[2] == 0 and len(vis[2]) == 0 and len(ext[2]) == 0
        assert xa.view_batch_route_counts() == [4, 0, 0, 0]
        assert same_bits(ta[2].get_tracking_result(), before[0]) and ta[2].get_sigma2() == before[1]
        with pytest.raises(B.TdloError) as e:
            B.frames_from_cloud_view_batch(ta, rc, LEAF, D_VIS, selects=sels)
        assert e.value.code == B.TDLO_E_EMPTY
        three = [tb[i] for i in (0, 1, 3)]
        for _ in range(2):                                                                  # (the call above stepped the three a second time)
            for i in (0, 1, 3):
                xb.voxel_grid_view(i, rc[i], LEAF, want_cloud=False)
            assert B.frame_batch(three, D_VIS)[0] == [0, 0, 0]
        for i in (0, 1, 3):
            assert_same_state(state(ta[i]), state(tb[i]), f"tracker {i} beside the empty one")
    finally:
        xa.close(); xb.close()
