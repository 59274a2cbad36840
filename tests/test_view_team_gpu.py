"""GPU suite for the voxel grid on cloud views in ONE launch (k_cloud_team's view instantiations, csrc/tdlo_cloud.hip + csrc/tdlo_view_lane.h;
tdlo_cloud_view_voxel_grid, tdlo_cloud_view_voxel_grid_visibility, tdlo_tracker_frame_from_cloud_view).  Every comparison is on bits against
tests/voxel_ref.py (its power on the scene catalogue is established in tests/test_cloud_scenes_ref.py and tests/test_view_team_ref.py); every case asserts
the route it took through tdlo_debug_route_count 27 / 28 / 29 (Context.view_route_counts).  The comparator contexts -- TDLO_CLOUD_TEAM=0 and
TDLO_CLOUD_FUSED=0, where every view call takes the multi-launch form -- keep that form covered."""
import os

import numpy as np
import pytest

import cloud_scenes as S
import prepass_ref
import voxel_ref as R
from test_cloud_view_gpu import _layouts, _view, _same_tracker_state
from test_voxel_view_gpu import _points, _Fixed, _laid_out, _box_cloud, _empty_slot_report

pytestmark = pytest.mark.gpu

LEAF = 0.05
ROUTES = ("team", "one", "multi")                                  # the default; TDLO_CLOUD_TEAM=0; TDLO_CLOUD_FUSED=0 -- the last two are the comparators


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    return binding


def _make(route, **kw):
    from trackdlo_amd import binding as B
    old = {k: os.environ.get(k) for k in ("TDLO_CLOUD_TEAM", "TDLO_CLOUD_FUSED")}
    try:
        for k in old:
            os.environ.pop(k, None)
        if route == "one":
            os.environ["TDLO_CLOUD_TEAM"] = "0"
        elif route == "multi":
            os.environ["TDLO_CLOUD_FUSED"] = "0"
        return B.Context(device=0, timing=False, **dict(dict(max_frames=2, max_points=1 << 15, max_nodes=64), **kw))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    c = {r: _make(r) for r in ROUTES}
    yield c
    for x in c.values():
        x.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what=None):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).any(axis=1).sum()), "rows differ")


def _check(got, want, what=None):
    """(X, n, n_raw) of voxel_grid_view against (X, n_raw) of voxel_ref."""
    X, n, n_raw = got
    assert n == want[0].shape[0] and n_raw == want[1], (what, n, n_raw, want[0].shape, want[1])
    _same_bits(X, want[0], what)


class _Counted:
    """with _Counted(ctx, [taken, passed, rides], what): the route counters 27 / 28 / 29 move by exactly that."""

    def __init__(self, ctx, delta, what=None):
        self.ctx, self.delta, self.what = ctx, list(delta), what

    def __enter__(self):
        self.before = self.ctx.view_route_counts()
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            after = self.ctx.view_route_counts()
            assert [a - b for a, b in zip(after, self.before)] == self.delta, (self.what, self.before, after, self.delta)
        return False


def _delta(scene_route, calls=1):
    return {"taken": [calls, 0, 0], "passed": [0, calls, 0], "untouched": [0, 0, 0]}[scene_route]


# ---- 1. layouts -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_every_layout_with_and_without_selection(B, ctxs, torch, N):
    """The last word of a view and the tile border (4096 elements; 8193: three tiles, the last of one element), every layout of the cloud-view suite with NaN
    in every element the view does not address, host and device memory, no selection / a selection / a device selection that starts 1, 2, 3 bytes into
    its allocation with set bytes in front of and behind it."""
    ctx = ctxs["team"]
    rng = np.random.default_rng(4000 + N)
    P = _points(N, rng)
    sel = ((rng.random(N) < 0.7) * rng.integers(1, 256, N)).astype(np.uint8)
    sel[rng.integers(0, N)] = 7                                   # (at least one element is selected)
    pad = torch.full((N + 16,), 255, dtype=torch.uint8, device="cuda")
    seld = []
    for off in (0, 1, 2, 3):
        buf = pad.clone()
        buf[off:off + N] = torch.from_numpy(sel).cuda()
        seld.append(buf[off:off + N])
        assert seld[-1].data_ptr() % 4 == off
    calls = 0
    with _Counted(ctx, [14 * 8, 0, 0], N):
        for name, flat, off, sp, sc in _layouts(N, _Fixed(P)):
            pts = _laid_out(flat, off, sp, sc, N)
            want_all, want_sel = R.voxel_ref(pts, None, LEAF), R.voxel_ref(pts, sel, LEAF)
            assert want_all[1] == N and 0 < want_sel[1] <= N
            es = flat.itemsize
            hv = _view(B, flat.ctypes.data + off * es, flat.dtype, sp, sc, N, flat)
            _check(ctx.voxel_grid_view(0, hv, LEAF), want_all, (name, N, "host"))
            _check(ctx.voxel_grid_view(0, hv, LEAF, select=sel), want_sel, (name, N, "host, select"))
            dev = torch.from_numpy(flat).cuda()
            dv = _view(B, dev.data_ptr() + off * es, flat.dtype, sp, sc, N, dev)
            _check(ctx.voxel_grid_view(1, dv, LEAF), want_all, (name, N, "device"))
            _check(ctx.voxel_grid_view(1, dv, LEAF, select=sel), want_sel, (name, N, "device, host select"))
            for o, s in enumerate(seld):
                _check(ctx.voxel_grid_view(1, dv, LEAF, select=s), want_sel, (name, N, "device, device select +%d" % o))
            calls += 8
            del dev
    assert calls == 14 * 8


# ---- 2. the scene catalogue as organized clouds --------------------------------------------------------------------------------------------------------
def _organized(s):
    return R.backproject(s.depth, np.ones_like(s.mask), *s.cam), np.asarray(s.mask).reshape(-1).copy()


@pytest.mark.parametrize("name", [n for n in S.NAMES if n not in S.LARGE])
def test_scene_as_an_organized_cloud(ctxs, torch, name):
    """view = every pixel back-projected, select = the mask (slice borders, runs longer than the staging window, 32 704 and 32 705 points, rb + kb = 32 / 33,
    the pass-through scene), from host and device memory; then compacted: view = the masked points, no selection."""
    ctx = ctxs["team"]
    s = S.get(name)
    org, sel = _organized(s)
    pts = s.points()
    with _Counted(ctx, _delta(s.route, 4), name):
        _check(ctx.voxel_grid_view(0, org, s.leaf, select=sel), s.ref, (name, "organized, host"))
        _check(ctx.voxel_grid_view(1, torch.from_numpy(org).cuda(), s.leaf, select=torch.from_numpy(sel).cuda()), s.ref, (name, "organized, device"))
        _check(ctx.voxel_grid_view(0, pts, s.leaf), s.ref, (name, "compacted, host"))
        _check(ctx.voxel_grid_view(1, torch.from_numpy(pts).cuda(), s.leaf), s.ref, (name, "compacted, device"))


@pytest.mark.parametrize("name", ["E_max", "E_over"])
def test_4095_and_4096_tiles(ctxs, torch, name):
    """The most tiles the one-launch kernel takes, and one element more (the host does not launch it): device memory only, once each."""
    ctx = ctxs["team"]
    s = S.get(name)
    assert S.tiles(s.P) == (S.kFTmax if name == "E_max" else S.kFTmax + 1)
    org, sel = _organized(s)
    with _Counted(ctx, _delta(s.route), name):
        _check(ctx.voxel_grid_view(1, torch.from_numpy(org).cuda(), s.leaf, select=torch.from_numpy(sel).cuda()), s.ref, name)


# ---- 3. non-finite points -----------------------------------------------------------------------------------------------------------------------------
def test_non_finite_points(ctxs, torch):
    """An organized float32 cloud with NaN where there is no return -- in unselected and in selected elements --, +-inf, float64 beyond float range, and
    cells whose only point has -0.0f coordinates (the sum starts from 0.0f: +0.0 comes out)."""
    ctx = ctxs["team"]
    rng = np.random.default_rng(51)
    rows, cols = 96, 131
    N = rows * cols
    i, j = np.mgrid[0:rows, 0:cols]
    z = (0.6 + 0.002 * j + 0.001 * i + 0.001 * rng.random((rows, cols))).astype(np.float32)
    org = np.stack([((j - 64.5) * z / 600).astype(np.float32), ((i - 47.5) * z / 600).astype(np.float32), z], axis=2).reshape(N, 3)
    org[rng.random(N) < 0.3] = np.nan                              # no return
    sel = ((rng.random(N) < 0.25) * 255).astype(np.uint8)
    assert (np.isnan(org[:, 0]) & (sel != 0)).sum() > 500 and (np.isnan(org[:, 0]) & (sel == 0)).sum() > 500
    inf = org.copy()
    hit = rng.random(N) < 0.05
    inf[hit, rng.integers(0, 3, N)[hit]] = rng.choice(np.array([np.inf, -np.inf], dtype=np.float32), N)[hit]
    big = org.astype(np.float64)
    big[::5, 0] = 1e300; big[1::7, 2] = -3.5e38; big[2::9, 1] = 3.4028235677973366e38
    zero = org.copy()
    zero[::97] = (-0.0, -0.0, 0.0); zero[5::101, 0] = -0.0
    zsel = sel.copy(); zsel[::97] = 1
    cases = (("nan", org, sel), ("nan, all selected", org, None), ("inf", inf, sel), ("f64 range", big, sel), ("f64 range, all", big, None), ("-0.0f", zero, zsel))
    with _Counted(ctx, [2 * len(cases), 0, 0]):
        for what, arr, s in cases:
            want = R.voxel_ref(arr, s, 0.008)
            assert 0 < want[0].shape[0] < want[1] < (N if s is None else (s != 0).sum())      # (non-finite points among the selected)
            _check(ctx.voxel_grid_view(0, arr, 0.008, select=s), want, (what, "host"))
            _check(ctx.voxel_grid_view(1, torch.from_numpy(arr).cuda(), 0.008, select=None if s is None else torch.from_numpy(s).cuda()), want, (what, "device"))
    want = R.voxel_ref(zero, zsel, 0.008)
    assert (_bits(want[0])[:, :2] == 0).all(axis=1).sum() >= 1 and not (_bits(want[0]) == 1 << 63).any()


# ---- 4. comparator ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("one", "multi"))
def test_the_comparator_contexts_take_the_multi_launch_form(B, ctxs, torch, route):
    """TDLO_CLOUD_TEAM=0 / TDLO_CLOUD_FUSED=0: the same calls, the same bits, and the one-launch kernel is never handed a view."""
    ctx, team = ctxs[route], ctxs["team"]
    N = 4097
    rng = np.random.default_rng(61)
    P = _points(N, rng)
    sel = ((rng.random(N) < 0.7) * rng.integers(1, 256, N)).astype(np.uint8)
    calls = ctx.voxel_view_calls()
    with _Counted(ctx, [0, 0, 0], route), _Counted(team, [14 * 2, 0, 0], "team"):
        for name, flat, off, sp, sc in _layouts(N, _Fixed(P)):
            want = R.voxel_ref(_laid_out(flat, off, sp, sc, N), sel, LEAF)
            es = flat.itemsize
            dev = torch.from_numpy(flat).cuda()
            for c in (ctx, team):
                _check(c.voxel_grid_view(0, _view(B, flat.ctypes.data + off * es, flat.dtype, sp, sc, N, flat), LEAF, select=sel), want, (name, "host"))
                _check(c.voxel_grid_view(1, _view(B, dev.data_ptr() + off * es, flat.dtype, sp, sc, N, dev), LEAF, select=torch.from_numpy(sel).cuda()), want, (name, "device"))
                _same_bits(c.get_cloud(0), c.get_cloud(1))
            del dev
    assert ctx.voxel_view_calls() == calls + 14 * 2


RADIX = [((15, 17, 1), 1), ((16, 16, 1), 2), ((257, 1, 1), 2), ((255, 257, 1), 2), ((256, 16, 16), 3), ((6, 10923, 1), 3), ((4095, 4097, 1), 3),
         ((256, 256, 256), 4), ((97, 257, 673), 4)]             # the cases of test_voxel_view_gpu.py::test_one_to_four_radix_passes


@pytest.mark.parametrize("div,passes", RADIX)
def test_one_to_four_radix_passes_of_the_view_form(B, ctxs, torch, div, passes):
    """The multi-launch form's radix passes stay exercised on the comparator contexts; on the default context the kernel takes the case or passes it on by
    the header's rule (rank bits + cell-index bits beyond 32), the same bits either way."""
    P, leaf = _box_cloud(div, np.random.default_rng(sum(div)))
    min_b, div_b, nodown = B.voxel_grid_dims(P.min(axis=0), P.max(axis=0), leaf)
    cells = int(np.prod(div_b.astype(np.int64)))
    assert not nodown and tuple(div_b) == tuple(div) and (1 << (8 * (passes - 1))) <= max(cells, 1) and (passes == 4 or cells < (1 << (8 * passes)))
    want = R.voxel_ref(P, None, leaf)
    dev = torch.from_numpy(P).cuda()
    for route in ("one", "multi"):
        with _Counted(ctxs[route], [0, 0, 0], (div, route)):
            _check(ctxs[route].voxel_grid_view(0, P, leaf), want, (div, route, "host"))
            _check(ctxs[route].voxel_grid_view(1, dev, leaf), want, (div, route, "device"))
    st = R.structure(P, None, leaf)
    with _Counted(ctxs["team"], _delta(S.route_rule(st, S.tiles(P.shape[0])), 2), (div, "team")):
        _check(ctxs["team"].voxel_grid_view(0, P, leaf), want, (div, "team", "host"))
        _check(ctxs["team"].voxel_grid_view(1, dev, leaf), want, (div, "team", "device"))


# ---- 5. refusals and capacity ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_view_leaves_the_resident_cloud(B, ctxs, torch):
    """A slot holding 300 points, then a 500-point view 1e9 leaf sizes from the origin: the kernel passes it on, the multi-launch form refuses it
    ("too far"), and the slot's cloud is what it was -- the kernel wrote nothing and the slot was not grown."""
    ctx = ctxs["team"]
    rng = np.random.default_rng(71)
    X = rng.standard_normal((300, 3))
    ctx.set_cloud(0, X)
    far = (_points(500, rng) * 0.1 + np.array([1.0e9, 0.0, 0.0])).astype(np.float32)
    with pytest.raises(R.TooFar):
        R.voxel_ref(far, None, 0.008)
    for src in (far, torch.from_numpy(far).cuda()):
        with _Counted(ctx, [0, 1, 0], "too far"):
            with pytest.raises(B.TdloError) as e:
                ctx.voxel_grid_view(0, src, 0.008)
        assert e.value.code == B.TDLO_E_INVALID and "too far" in str(e.value)
        _same_bits(ctx.get_cloud(0), X)


def test_a_slot_too_small_for_the_result_grows_on_the_way(B, torch):
    """A fresh context with the smallest slots there are (a slot's capacity is never below 1024 points): a view of 3000 occupied cells does not fit, the
    kernel says so without writing, the call grows the slot and finishes on the multi-launch form; the next call finds room and is served in one launch."""
    ctx = _make("team", max_frames=1, max_points=1)
    try:
        rng = np.random.default_rng(72)
        cells = rng.permutation(20 * 20 * 20)[:3000]
        P = ((np.stack([cells % 20, cells // 20 % 20, cells // 400], axis=1) - 7 + 0.25 + 0.5 * rng.random((3000, 3))) * LEAF).astype(np.float32)
        want = R.voxel_ref(P, None, LEAF)
        assert want[0].shape[0] == 3000
        small = P[:700]
        with _Counted(ctx, [1, 0, 0], "fits"):
            _check(ctx.voxel_grid_view(0, small, LEAF), R.voxel_ref(small, None, LEAF), "fits")
        with _Counted(ctx, [0, 1, 0], "grows"):
            _check(ctx.voxel_grid_view(0, torch.from_numpy(P).cuda(), LEAF), want, "grows")
        with _Counted(ctx, [1, 0, 0], "room"):
            _check(ctx.voxel_grid_view(0, P, LEAF), want, "room")
    finally:
        ctx.close()


def test_nothing_kept_is_the_empty_slot_of_the_depth_path(B, ctxs, torch):
    ctx = ctxs["team"]
    rng = np.random.default_rng(73)
    N = 5000
    P = _points(N, rng).astype(np.float32)
    depth = rng.integers(300, 900, size=(40, 50)).astype(np.uint16)
    ctx.set_cloud(1, P.astype(np.float64))
    X, n, n_raw = ctx.depth_to_cloud(1, depth, np.zeros((40, 50), np.uint8), 600.0, 600.0, 25.0, 20.0, 0.008)
    assert (n, n_raw) == (0, 0) and ctx.get_cloud(1).shape == (0, 3)
    want = _empty_slot_report(B, ctx, 1)
    nowhere = P.copy(); nowhere[np.arange(N), rng.integers(0, 3, N)] = np.nan
    for arr, s in ((P, np.zeros(N, np.uint8)), (P, torch.zeros(N, dtype=torch.uint8, device="cuda")), (nowhere, None), (torch.from_numpy(nowhere).cuda(), None)):
        ctx.set_cloud(0, P.astype(np.float64))
        with _Counted(ctx, [1, 0, 0], "empty"):                    # (the kernel itself reports the empty cloud)
            X, n, n_raw = ctx.voxel_grid_view(0, arr, LEAF, select=s)
        assert (n, n_raw) == (0, 0) and X.shape == (0, 3)
        assert _empty_slot_report(B, ctx, 0) == want


# ---- 6. depth frames and view calls interleaved ---------------------------------------------------------------------------------------------------------
def test_one_context_through_depth_frames_and_views_of_different_sizes(B, torch):
    """The state words, the team's sort buffers and `cloud_fused_first` are one set for both kinds of call: depth frame, view, depth frame of another size,
    view of another size -- every result its own reference, counters 6 / 7 the depth frames' alone."""
    ctx = _make("team")
    try:
        a, b, v2 = S.get("C_4097"), S.get("D_7_last"), S.get("D_2_alternate")
        P1 = _points(9001, np.random.default_rng(81)).astype(np.float32)
        org2, sel2 = _organized(v2)
        for rep in range(2):
            X, n, nraw = ctx.depth_to_cloud(0, a.depth, a.mask, *a.cam, a.leaf)
            _check((X, n, nraw), a.ref, ("depth", a.name, rep))
            _check(ctx.voxel_grid_view(0, torch.from_numpy(P1).cuda(), LEAF), R.voxel_ref(P1, None, LEAF), ("view", rep))
            X, n, nraw = ctx.depth_to_cloud(0, b.depth, b.mask, *b.cam, b.leaf)
            _check((X, n, nraw), b.ref, ("depth", b.name, rep))
            _check(ctx.voxel_grid_view(0, org2, v2.leaf, select=sel2), v2.ref, ("organized view", rep))
        assert ctx.cloud_route_counts() == [4, 0] and ctx.cloud_vis_rides() == 0
        assert ctx.view_route_counts() == [4, 0, 0] and ctx.voxel_view_calls() == 4
    finally:
        ctx.close()


# ---- 7. the ride ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rope():
    from trackdlo_amd import synth
    X, Y, _ = synth.scene(6000, 65, config=71)
    return np.ascontiguousarray(X.astype(np.float32)), np.ascontiguousarray(Y)


@pytest.mark.parametrize("M", [1, 2, 45, 64, 65])
def test_the_visibility_pre_pass_rides_in_the_launch(B, ctxs, torch, rope, M):
    """tdlo_cloud_view_voxel_grid_visibility against the two calls on a comparator context and against tests/prepass_ref.py: cloud, node distances and both
    index sets bit for bit; with up to 64 nodes the pre-pass rode (count 29), with 65 it ran behind the launch."""
    from trackdlo_amd import synth
    ctx, cmp_ = ctxs["team"], ctxs["multi"]
    X32, Y65 = rope
    Y = np.ascontiguousarray(Y65[:M] + (np.arange(M)[:, None] % 3 == 2) * 0.02)      # (a third of the nodes beyond the threshold)
    coord = np.arange(M) * 0.01
    thr, d_vis, leaf = synth.LAUNCH_PARAMS["visibility_threshold"], 0.06, 0.008
    want = R.voxel_ref(X32, None, leaf)
    for src, where in ((X32, "host"), (torch.from_numpy(X32).cuda(), "device")):
        with _Counted(ctx, [1, 0, 1 if M <= 64 else 0], (M, where)):
            dist, vis, ext, n, nraw = ctx.voxel_grid_view_visibility(0, src, leaf, Y, thr, d_vis, coord)
        with _Counted(cmp_, [0, 0, 0], (M, where)):
            Xb, nb, nrawb = cmp_.voxel_grid_view(0, src, leaf)
            db, vb, eb = cmp_.visibility_prepass(0, Y, thr, d_vis, coord)
        assert (n, nraw) == (nb, nrawb) == (want[0].shape[0], want[1])
        _same_bits(ctx.get_cloud(0), Xb, (M, where)); _same_bits(Xb, want[0], (M, where))
        assert np.array_equal(dist.view(np.uint64), db.view(np.uint64)) and np.array_equal(vis, vb) and np.array_equal(ext, eb), (M, where)
        rd, rv, re = prepass_ref.prepass(want[0], Y, thr, d_vis, coord)
        assert np.array_equal(dist.view(np.uint64), np.asarray(rd).view(np.uint64)) and np.array_equal(vis, rv) and np.array_equal(ext, re), (M, where)
        assert M < 45 or 0 < len(vis) < M
    # a selection that keeps nothing: no cloud, nothing visible, no error
    with _Counted(ctx, [1, 0, 0], (M, "nothing kept")):
        dist, vis, ext, n, nraw = ctx.voxel_grid_view_visibility(0, X32, leaf, Y, thr, d_vis, coord, select=np.zeros(X32.shape[0], np.uint8))
    assert (n, nraw, len(vis), len(ext)) == (0, 0, 0, 0)
    # ... and the next ride finds the minima armed
    with _Counted(ctx, [1, 0, 1 if M <= 64 else 0], (M, "again")):
        d2, v2, e2, n, nraw = ctx.voxel_grid_view_visibility(0, X32, leaf, Y, thr, d_vis, coord)
    assert np.array_equal(d2.view(np.uint64), np.asarray(rd).view(np.uint64)) and np.array_equal(v2, rv) and np.array_equal(e2, re)


# ---- 8. tracker frames ------------------------------------------------------------------------------------------------------------------------------------
def test_tracker_frames_ride_and_equal_the_three_calls_by_hand(B, torch):
    """Five frames through tdlo_tracker_frame_from_cloud_view on the default context against voxel grid, pre-pass and tracking_step called by hand on a
    comparator context (TDLO_CLOUD_TEAM=0: the multi-launch form, the pre-pass in a launch of its own): the same tracker state, and all five frames rode."""
    from trackdlo_amd import synth
    N, M, leaf, d_vis = 6000, 30, 0.008, 0.06
    _, Y0, _ = synth.scene(N, M, config=71)
    Pm = synth.LAUNCH_PARAMS
    args = (M, Pm["visibility_threshold"], Pm["beta"], Pm["lambda_"], Pm["alpha"], Pm["k_vis"], Pm["mu"], 30, Pm["tol"], Pm["beta_pre_proc"], Pm["lambda_pre_proc"], Pm["lle_weight"])
    ca, cb = _make("team", max_frames=1), _make("one", max_frames=1)
    ta, tb = B.trackdlo(*args, ctx=ca, precision=0), B.trackdlo(*args, ctx=cb, precision=0)
    try:
        coord = synth.geodesic_coord(Y0)
        for t in (ta, tb):
            t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        thr = Pm["visibility_threshold"]
        for fr in range(5):
            X, _, _ = synth.scene(N, M, config=71, frame=fr, occlude=(0.4, 0.5) if fr == 3 else None)
            X32 = np.ascontiguousarray(X.astype(np.float32))
            src = torch.from_numpy(X32).cuda() if fr % 2 else X32
            va, vea, na, nrawa = ta.frame_from_cloud_view(src, leaf, d_vis)
            Xb, nb, nrawb = cb.voxel_grid_view(0, src, leaf)
            _, vb, veb = cb.visibility_prepass(0, tb.get_tracking_result(), thr, d_vis, coord)
            tb.tracking_step(None, vb, veb)
            assert (na, nrawa) == (nb, nrawb) and 0 < na < nrawa == X32.shape[0]
            assert np.array_equal(va, vb) and np.array_equal(vea, veb) and len(va) > 0
            _same_tracker_state(ta, tb)
            _same_bits(ca.get_cloud(0), Xb)
        assert ca.view_route_counts() == [5, 0, 5] and cb.view_route_counts() == [0, 0, 0] and cb.voxel_view_calls() == 5
        # a frame whose selection keeps nothing: TDLO_E_EMPTY, the nodes as they were
        before = ta.get_tracking_result().copy()
        with pytest.raises(B.TdloError) as e:
            ta.frame_from_cloud_view(X32, leaf, d_vis, select=np.zeros(X32.shape[0], np.uint8))
        assert e.value.code == -4                                 # TDLO_E_EMPTY
        _same_bits(ta.get_tracking_result(), before)
        _same_tracker_state(ta, tb)
        assert ca.view_route_counts() == [6, 0, 5]
    finally:
        del ta, tb
        ca.close(); cb.close()
