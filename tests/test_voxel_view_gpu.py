"""GPU suite for the voxel grid on cloud views (tdlo_cloud_view_voxel_grid, tdlo_tracker_frame_from_cloud_view; the view source of k_cloud_bbox /
k_cloud_keys / k_cloud_centroid in csrc/tdlo_cloud.hip).  tests/voxel_ref.py is the numpy statement of V(view, N, select, leaf) from the contract in
include/trackdlo_hip.h; tests/test_voxel_ref.py holds it to the C oracle of the depth path.  Every comparison here is on bits (uint64 views); there is
no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import voxel_ref as R
from test_cloud_view_gpu import _layouts, _view, _trackers, _same_tracker_state

pytestmark = pytest.mark.gpu

LEAF = 0.05


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
def ctx(B):
    c = B.Context(device=0, max_frames=2, max_points=1 << 15, max_nodes=64, timing=False)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(np.asfortranarray(a, dtype=np.float64).T).view(np.uint64)


def _same_bits(a, b, what=None):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), what


def _check(got, want, what=None):
    """(X, n, n_raw) of voxel_grid_view against (X, n_raw) of voxel_ref."""
    X, n, n_raw = got
    assert n == want[0].shape[0] and n_raw == want[1], (what, n, n_raw, want[0].shape, want[1])
    _same_bits(X, want[0], what)


def _points(N, rng, leaf=LEAF):
    """Clustered points: cells hold from one to a few hundred points (a skewed choice among ~N / 40 cells around the origin, negative cells among them), the
    points of a cell differ in magnitude from component to component, and about a tenth of the coordinates are exact multiples of the leaf (cell edges)."""
    ncell = max(min(N, 3), N // 40)
    cells = rng.integers(-6, 7, size=(ncell, 3))
    which = np.minimum((rng.random(N) ** 3 * ncell).astype(np.int64), ncell - 1)
    u = rng.random((N, 3)) * np.array([1.0, 1e-3, 0.999])
    u[rng.random((N, 3)) < 0.1] = 0.0
    return (cells[which] + u) * leaf


class _Fixed:
    """Hands _layouts the points to lay out (it draws them with standard_normal)."""
    def __init__(self, P):
        self.P = P

    def standard_normal(self, shape):
        assert tuple(shape) == self.P.shape
        return self.P


def _laid_out(flat, off, sp, sc, N):
    idx = off + np.arange(N)[:, None] * sp + np.arange(3)[None, :] * sc
    return flat[idx]


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_every_layout_from_host_and_device_memory(B, ctx, torch, N):
    """Wave (64), workgroup (256) and tile (1024) edges of the kernels; every layout of the cloud-view suite with NaN in every element the view does not
    address (a lane read as a coordinate makes its point vanish or moves a box); host memory (AUTO, HOST) and a device tensor (AUTO, DEVICE)."""
    P = _points(N, np.random.default_rng(2000 + N))
    calls = ctx.voxel_view_calls()
    for name, flat, off, sp, sc in _layouts(N, _Fixed(P)):
        want = R.voxel_ref(_laid_out(flat, off, sp, sc, N), None, LEAF)
        assert want[1] == N and (N < 255 or want[0].shape[0] < N // 4)
        es = flat.itemsize
        for loc in (B.MEM_AUTO, B.MEM_HOST):
            _check(ctx.voxel_grid_view(0, _view(B, flat.ctypes.data + off * es, flat.dtype, sp, sc, N, flat, loc), LEAF), want, (name, N, "host", loc))
        dev = torch.from_numpy(flat).cuda()
        for loc in (B.MEM_AUTO, B.MEM_DEVICE):
            _check(ctx.voxel_grid_view(1, _view(B, dev.data_ptr() + off * es, flat.dtype, sp, sc, N, dev, loc), LEAF), want, (name, N, "device", loc))
        del dev
    assert ctx.voxel_view_calls() == calls + 14 * 4


def _empty_slot_report(B, ctx, slot):
    """What a registration on the slot says."""
    from trackdlo_amd import synth
    p = B.make_params(**{k: synth.LAUNCH_PARAMS[k] for k in ("beta", "lambda_", "lle_weight", "mu")})
    with pytest.raises(B.TdloError) as e:
        ctx.cpd_lle_resident(slot, synth.nodes(20), 0.0, p)
    return e.value.code, str(e.value)


def test_selection(B, ctx, torch):
    rng = np.random.default_rng(31)
    N = 3001
    P = _points(N, rng).astype(np.float32)
    bad = P.copy()
    hit = rng.random(N) < 0.1
    comp = rng.integers(0, 3, N)
    val = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), N)
    bad[hit, comp[hit]] = val[hit]
    assert 200 < hit.sum() < 400
    sel = (rng.random(N) < 0.6).astype(np.uint8) * rng.integers(1, 256, N).astype(np.uint8)
    sel_dev = torch.from_numpy(sel).cuda()
    xyz_ = np.full((N, 4), np.nan, dtype=np.float32); xyz_[:, :3] = bad
    cols = np.asfortranarray(bad)                                 # column-major: the paired loads (N odd: its staged host copy is read element by element)
    cols_even = np.full((3, N + 1), np.nan, dtype=np.float32); cols_even[:, :N] = bad.T
    for name, arr in (("packed", bad), ("xyz_", xyz_), ("columns", cols), ("columns-even", cols_even.T[:N]), ("f64", bad.astype(np.float64))):
        for s, sname in ((None, "all"), (sel, "host select"), (sel_dev, "device select"), (sel != 0, "bool select")):
            want = R.voxel_ref(arr, None if s is None else sel, LEAF)
            assert 0 < want[1] < N
            _check(ctx.voxel_grid_view(0, arr, LEAF, select=s), want, (name, sname, "host"))
            d = torch.from_numpy(np.ascontiguousarray(arr)).cuda() if name != "columns-even" else torch.from_numpy(cols_even).cuda().T[:N]
            _check(ctx.voxel_grid_view(1, d, LEAF, select=s), want, (name, sname, "device"))
    # float64 values beyond float range become +-inf: not kept
    big = P.astype(np.float64)
    big[::5, 0] = 1e300; big[1::7, 2] = -3.5e38; big[2::9, 1] = 3.4028235677973366e38      # (the last: above FLT_MAX + half an ulp, rounds to +inf)
    want = R.voxel_ref(big, None, LEAF)
    assert want[1] == int((np.abs(big) < 3.4028235e38).all(axis=1).sum()) < N - 900
    _check(ctx.voxel_grid_view(0, big, LEAF), want, "f64 range host")
    _check(ctx.voxel_grid_view(1, torch.from_numpy(big).cuda(), LEAF), want, "f64 range device")
    # one kept point; all points in one cell
    one = np.zeros(N, np.uint8); one[1234] = 1
    _check(ctx.voxel_grid_view(0, P, LEAF, select=one), (P[1234:1235].astype(np.float64), 1), "one kept")
    cell = ((np.array([3, -2, 5]) + rng.random((N, 3)) * 0.99) * LEAF).astype(np.float32)
    want = R.voxel_ref(cell, None, LEAF)
    assert want[0].shape[0] == 1
    _check(ctx.voxel_grid_view(0, cell, LEAF), want, "one cell")
    _check(ctx.voxel_grid_view(1, torch.from_numpy(cell).cuda(), LEAF), want, "one cell device")


def test_nothing_kept_leaves_the_slot_as_the_depth_path_leaves_it(B, ctx, torch):
    rng = np.random.default_rng(32)
    N = 2000
    P = _points(N, rng).astype(np.float32)
    depth = rng.integers(300, 900, size=(40, 50)).astype(np.uint16)
    ctx.set_cloud(0, P.astype(np.float64)); ctx.set_cloud(1, P.astype(np.float64))
    X, n, n_raw = ctx.depth_to_cloud(1, depth, np.zeros((40, 50), np.uint8), 600.0, 600.0, 25.0, 20.0, 0.008)
    assert (n, n_raw) == (0, 0) and ctx.get_cloud(1).shape == (0, 3)
    want = _empty_slot_report(B, ctx, 1)
    nowhere = P.copy(); nowhere[np.arange(N), rng.integers(0, 3, N)] = np.nan
    for arr, s in ((P, np.zeros(N, np.uint8)), (P, torch.zeros(N, dtype=torch.uint8, device="cuda")), (nowhere, None), (torch.from_numpy(nowhere).cuda(), None)):
        ctx.set_cloud(0, P.astype(np.float64))
        X, n, n_raw = ctx.voxel_grid_view(0, arr, LEAF, select=s)
        assert (n, n_raw) == (0, 0) and X.shape == (0, 3)
        assert _empty_slot_report(B, ctx, 0) == want


def _box_cloud(div, rng, n=3000, leaf=0.125):
    """Points at cell centres of a grid of exactly div[0] x div[1] x div[2] cells (leaf and centres are binary fractions: the arithmetic is exact), both
    corners among them, the grid's first cell at a negative index."""
    div = np.asarray(div)
    lo = np.array([-3, 2, -div[2] // 2])
    c = np.stack([rng.integers(0, d, n) for d in div], axis=1)
    c[: n // 2] = c[rng.integers(0, 40, n // 2)]                  # shared cells
    c[0] = 0; c[-1] = div - 1
    return ((lo + c + 0.5) * leaf).astype(np.float32), leaf


@pytest.mark.parametrize("div,passes", [((15, 17, 1), 1), ((16, 16, 1), 2), ((257, 1, 1), 2), ((255, 257, 1), 2), ((256, 16, 16), 3), ((6, 10923, 1), 3),
                                        ((4095, 4097, 1), 3), ((256, 256, 256), 4), ((97, 257, 673), 4)])
def test_one_to_four_radix_passes(B, ctx, torch, div, passes):
    """Cell counts just below, at and just above 2^8, 2^16 and 2^24 with a few thousand keys."""
    P, leaf = _box_cloud(div, np.random.default_rng(sum(div)))
    min_b, div_b, nodown = B.voxel_grid_dims(P.min(axis=0), P.max(axis=0), leaf)
    cells = int(np.prod(div_b.astype(np.int64)))
    assert not nodown and tuple(div_b) == tuple(div) and (1 << (8 * (passes - 1))) <= max(cells, 1) and (passes == 4 or cells < (1 << (8 * passes)))
    want = R.voxel_ref(P, None, leaf)
    assert 40 <= want[0].shape[0] < P.shape[0]
    _check(ctx.voxel_grid_view(0, P, leaf), want, (div, "host"))
    _check(ctx.voxel_grid_view(1, torch.from_numpy(P).cuda(), leaf), want, (div, "device"))


def test_pass_through(B, ctx, torch):
    """PCL's "leaf size too small": two clusters 10^4 leaf sizes apart on each axis; the output is the kept points in input order, bit for bit
    (points with -0.0f coordinates among them)."""
    rng = np.random.default_rng(33)
    N = 4099
    P = (rng.random((N, 3)) * 0.1 + np.where(rng.random((N, 1)) < 0.5, 0.0, 1e4 * 0.008)).astype(np.float32)
    P[::17, 1] = np.nan
    P[5::29, 0] = -0.0; P[7::31] = (-0.0, -0.0, 0.0)             # the kept points come back as they are: PCL copies them, and -0.0f stays -0.0
    sel = (rng.random(N) < 0.8).astype(np.uint8)
    keep = np.isfinite(P).all(axis=1) & (sel != 0)
    want = R.voxel_ref(P, sel, 0.008)
    assert want[0].shape[0] == want[1] == keep.sum() and np.array_equal(_bits(want[0]), _bits(P[keep].astype(np.float64)))
    assert (_bits(want[0]) == 1 << 63).sum() > 150
    _check(ctx.voxel_grid_view(0, P, 0.008, select=sel), want, "host")
    _check(ctx.voxel_grid_view(1, torch.from_numpy(P).cuda(), 0.008, select=sel), want, "device")


def _smooth_frame(rows, cols, rng, want_pixels):
    i, j = np.mgrid[0:rows, 0:cols]
    z = 450.0 + 0.5 * j + 0.3 * i + 20.0 * np.sin(i / 11.0) + rng.random((rows, cols))
    mask = np.zeros((rows, cols), np.uint8)
    band = want_pixels // cols + 1
    mask[rows // 3: rows // 3 + band] = 255
    mask[rng.random((rows, cols)) < 0.02] ^= 255
    return z.astype(np.uint16), mask


@pytest.mark.parametrize("shape,pixels", [((96, 128), 4000), ((480, 640), 40000)], ids=["96x128", "640x480"])
def test_against_the_depth_path(B, ctx, torch, shape, pixels):
    """V(P) on the back-projected float32 points of the masked pixels is what tdlo_depth_to_cloud leaves in the slot: cloud, n and n_raw."""
    rows, cols = shape
    depth, mask = _smooth_frame(rows, cols, np.random.default_rng(rows), pixels)
    fx, fy, cx, cy = 606.0, 605.5, cols / 2 - 0.5, rows / 2 - 0.5
    P = R.backproject(depth, mask, fx, fy, cx, cy)
    assert abs(P.shape[0] - pixels) < pixels // 5 and (rows < 480 or P.shape[0] > 32704)      # (beyond the one-launch form)
    xyz_ = np.full((P.shape[0], 4), np.nan, dtype=np.float32); xyz_[:, :3] = P
    dev = torch.from_numpy(xyz_).cuda()
    for leaf in (0.008, 0.02):
        Xd, n, n_raw = ctx.depth_to_cloud(1, depth, mask, fx, fy, cx, cy, leaf)
        assert n_raw == P.shape[0] and 0 < n < n_raw // 2
        _check(ctx.voxel_grid_view(0, P, leaf), (Xd, n_raw), ("host", leaf))
        _same_bits(ctx.get_cloud(0), ctx.get_cloud(1))
        _check(ctx.voxel_grid_view(0, dev, leaf), (Xd, n_raw), ("device", leaf))
    # the same as an organized cloud + the mask as selection
    org = R.backproject(depth, np.ones_like(mask), fx, fy, cx, cy)
    Xd, n, n_raw = ctx.depth_to_cloud(1, depth, mask, fx, fy, cx, cy, 0.008)
    _check(ctx.voxel_grid_view(0, org, 0.008, select=mask), (Xd, n_raw), "organized")


def test_tracker_frames_are_the_three_calls_by_hand(B, torch):
    from trackdlo_amd import synth
    N, M, leaf, d_vis = 6000, 30, 0.008, 0.06
    _, Y0, _ = synth.scene(N, M, config=71)
    (ca, ta), (cb, tb) = _trackers(B, M, Y0)
    try:
        coord = synth.geodesic_coord(Y0)
        thr = synth.LAUNCH_PARAMS["visibility_threshold"]
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
        # a frame whose selection keeps nothing: TDLO_E_EMPTY, the nodes as they were
        before = ta.get_tracking_result().copy()
        with pytest.raises(B.TdloError) as e:
            ta.frame_from_cloud_view(X32, leaf, d_vis, select=np.zeros(X32.shape[0], np.uint8))
        assert e.value.code == -4                                 # TDLO_E_EMPTY
        _same_bits(ta.get_tracking_result(), before)
        _same_tracker_state(ta, tb)
    finally:
        del ta, tb
        ca.close(); cb.close()


def test_refusals_leave_the_slot_as_it_was(B, ctx, torch):
    rng = np.random.default_rng(34)
    X = rng.standard_normal((300, 3))
    ctx.set_cloud(0, X)
    P = _points(500, rng).astype(np.float32)
    lib = ctx.lib
    n = C.c_int(-7); nraw = C.c_int(-7)

    def call(v, N, leaf=LEAF, slot=0):
        return lib.tdlo_cloud_view_voxel_grid(ctx.h, slot, C.byref(v), N, None, leaf, None, 0, C.byref(n), C.byref(nraw))

    dev = torch.from_numpy(P).cuda()
    asyn = B.cloud_view(dev, asynchronous=True)
    assert call(asyn, 500) == B.TDLO_E_INVALID and "ASYNC" in lib.tdlo_last_error(ctx.h).decode()
    good = B.cloud_view(P)
    cap_before = ctx.voxel_view_calls()
    assert call(good, (1 << 26) + 1) == B.TDLO_E_INVALID and "2^26" in lib.tdlo_last_error(ctx.h).decode()       # (before anything is allocated or read)
    for bad in (B.CloudView(good.data, 7, B.MEM_HOST, 3, 1, None, 0), B.CloudView(good.data, B.F32, B.MEM_HOST, 3, 0, None, 0),
                B.CloudView(None, B.F32, B.MEM_HOST, 3, 1, None, 0), B.CloudView(good.data + 2, B.F32, B.MEM_HOST, 3, 1, None, 0)):
        assert call(bad, 500) == B.TDLO_E_INVALID
    assert call(good, 0) == B.TDLO_E_INVALID and call(good, 500, slot=9) == B.TDLO_E_INVALID
    for leaf in (0.0, -0.05, float("nan")):
        assert call(good, 500, leaf) == B.TDLO_E_INVALID
    assert ctx.voxel_view_calls() == cap_before
    _same_bits(ctx.get_cloud(0), X)
    # a small cloud at x ~ 1e9 with an 8 mm leaf: no pass-through, and floor(x / leaf) is beyond int32
    far = (P * 0.1 + np.array([1.0e9, 0.0, 0.0])).astype(np.float32)
    with pytest.raises(R.TooFar):
        R.voxel_ref(far, None, 0.008)
    for src in (far, torch.from_numpy(far).cuda()):
        with pytest.raises(B.TdloError) as e:
            ctx.voxel_grid_view(0, src, 0.008)
        assert e.value.code == B.TDLO_E_INVALID and "too far" in str(e.value)
        _same_bits(ctx.get_cloud(0), X)
    trk = B.trackdlo(30, ctx=ctx)
    st = (B.Stats * 2)()
    assert lib.tdlo_tracker_frame_from_cloud_view(trk.h, C.byref(asyn), 500, None, 0.008, 0.06, None, None, None, None, None, None, C.cast(st, C.c_void_p)) == B.TDLO_E_INVALID
    _same_bits(ctx.get_cloud(0), X)


def test_ready_stream_orders_the_filter_behind_the_producer(B, ctx, torch):
    """The tensor is filled on a side stream behind a run of matrix products; the filter is handed that stream at once, without a host wait in between."""
    N = 4099
    P = _points(N, np.random.default_rng(35)).astype(np.float32)
    want = R.voxel_ref(P, None, LEAF)
    src = torch.from_numpy(P).cuda()
    dst = torch.full((N, 3), float("nan"), dtype=torch.float32, device="cuda")
    A = torch.randn((4096, 4096), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    (A @ A).sum().item()                                          # (the BLAS library's first call is out of the way)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            A = (A @ A) * 1e-4
        dst.copy_(src)
    _check(ctx.voxel_grid_view(0, dst, LEAF, ready_stream=side.cuda_stream), want, "ready_stream")
    torch.cuda.synchronize()
