"""GPU suite for cloud views (tdlo_set_cloud_view, tdlo_get_cloud, tdlo_tracker_tracking_step_view; csrc/tdlo_import.hip): a cloud taken as it arrives --
float32 or float64, any strides, host or device memory -- must become, BIT FOR BIT, the resident cloud that tdlo_set_cloud makes of the widened,
column-major copy (float -> double is exact), and everything registered or tracked from it must be the bits of the double path.  Every comparison
here is on bits (uint64 views); there is no tolerance anywhere.  tests/cloud_view_ref.py is the numpy statement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import cloud_view_ref as R

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
def ctx(B):
    c = B.Context(device=0, max_frames=2, max_points=1 << 15, max_nodes=64, timing=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_copy(B):
    """A context whose host views take the comparator route: the packed block copied to the device in front of the import kernel."""
    old = os.environ.get("TDLO_VIEW_INPLACE")
    os.environ["TDLO_VIEW_INPLACE"] = "0"                          # (read when the context is made)
    try:
        c = B.Context(device=0, max_points=1 << 15, max_nodes=64, timing=False)
    finally:
        if old is None:
            del os.environ["TDLO_VIEW_INPLACE"]
        else:
            os.environ["TDLO_VIEW_INPLACE"] = old
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(np.asfortranarray(a, dtype=np.float64).T).view(np.uint64)


def _same_bits(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _layouts(N, rng):
    """(name, flat buffer, element offset of `data`, stride_point, stride_comp): every element the view does not address is NaN, so a lane read as a
    coordinate shows."""
    P64 = rng.standard_normal((N, 3))                 # (float64 sources keep all their bits; float32 ones are widened exactly)

    def lay(dtype, size, off, sp, sc):
        flat = np.full(size, np.nan, dtype=dtype)
        idx = off + np.arange(N)[:, None] * sp + np.arange(3)[None, :] * sc
        flat[idx] = P64.astype(dtype)
        return flat, off, sp, sc

    ld = N + 5
    return [("packed",) + lay(np.float32, 3 * N, 0, 3, 1),
            ("xyz_",) + lay(np.float32, 4 * N, 0, 4, 1),
            ("xyzrgb",) + lay(np.float32, 8 * N, 0, 8, 1),
            ("columns",) + lay(np.float32, 3 * ld, 0, 1, ld),
            ("columns-even-ld",) + lay(np.float32, 3 * (ld + ld % 2), 0, 1, ld + ld % 2),
            ("packed+1",) + lay(np.float32, 3 * N + 1, 1, 3, 1),
            ("xyz_+1",) + lay(np.float32, 4 * N + 1, 1, 4, 1),
            ("columns+1",) + lay(np.float32, 3 * (ld + ld % 2) + 1, 1, 1, ld + ld % 2),
            ("reversed",) + lay(np.float32, 3 * N, 3 * (N - 1), -3, 1),
            ("reversed-columns",) + lay(np.float32, 3 * ld, 2 * ld, 1, -ld),
            ("stride-5",) + lay(np.float32, 5 * N, 0, 5, 2),
            ("packed-f64",) + lay(np.float64, 3 * N, 0, 3, 1),
            ("columns-f64",) + lay(np.float64, 3 * N, 0, 1, N),
            ("reversed-f64+1",) + lay(np.float64, 4 * N + 1, 1 + 4 * (N - 1), -4, 1)]


def _view(B, ptr, dtype, sp, sc, N, owner, location=0):
    v = B.CloudView(ptr, B.F32 if np.dtype(dtype).itemsize == 4 else B.F64, location, sp, sc, None, 0)
    v.N = N; v.owner = owner
    return v


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 255, 256, 257, 4099])
def test_get_cloud_after_set_cloud_view_equals_the_numpy_statement(B, ctx, ctx_copy, torch, N):
    """Wave (64), workgroup (256) and vector-tail boundaries, every layout, from host memory and from a device tensor."""
    rng = np.random.default_rng(1000 + N)
    for name, flat, off, sp, sc in _layouts(N, rng):
        want = R.widen(flat, flat.dtype, off, sp, sc, N)
        assert not np.isnan(want).any()
        es = flat.itemsize
        # host memory the runtime has never seen (TDLO_MEM_AUTO must call it host), and the same said outright
        for loc in (B.MEM_AUTO, B.MEM_HOST):
            ctx.set_cloud_view(0, _view(B, flat.ctypes.data + off * es, flat.dtype, sp, sc, N, flat, loc))
            _same_bits(ctx.get_cloud(0), want)
        ctx_copy.set_cloud_view(0, _view(B, flat.ctypes.data + off * es, flat.dtype, sp, sc, N, flat))
        _same_bits(ctx_copy.get_cloud(0), want)
        dev = torch.from_numpy(flat).cuda()
        for loc in (B.MEM_AUTO, B.MEM_DEVICE):
            ctx.set_cloud_view(1, _view(B, dev.data_ptr() + off * es, flat.dtype, sp, sc, N, dev, loc))
            got = ctx.get_cloud(1)
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (name, N, loc)
        del dev


def test_torch_tensors_through_their_array_interface(B, ctx, torch):
    """binding.cloud_view on real tensors: contiguous, a column slice of N x 8, a transposed (column-major) one, float64."""
    rng = np.random.default_rng(7)
    N = 1000
    wide = torch.from_numpy(rng.standard_normal((N, 8)).astype(np.float32)).cuda()
    cols = torch.from_numpy(rng.standard_normal((3, N + 6)).astype(np.float32)).cuda()
    for t in (wide[:, :3].contiguous(), wide, wide[:, 2:5], cols.T[:N], cols.T[3:N:2], wide[:, :3].double()):
        ctx.set_cloud_view(0, t)
        _same_bits(ctx.get_cloud(0), t[:, :3].cpu().numpy().astype(np.float64))
    assert B.cloud_view(wide).location == B.MEM_DEVICE and B.cloud_view(wide).stride_point == 8


def test_offsets_beyond_2_31_bytes(B, ctx, torch):
    """stride_point = 2^28 float32 elements, N = 3: the third point lies 2 GiB from the first.  The buffer is left uninitialised but for the nine
    elements the view addresses."""
    raw = torch.empty((1 << 31) + 64, dtype=torch.uint8, device="cuda")
    f = raw.view(torch.float32)
    sp = 1 << 28
    P = np.random.default_rng(3).standard_normal((3, 3)).astype(np.float32)
    idx = torch.from_numpy((np.arange(3)[:, None] * sp + np.arange(3)[None, :]).reshape(-1)).cuda()
    f[idx] = torch.from_numpy(P.reshape(-1)).cuda()
    torch.cuda.synchronize()
    v = _view(B, raw.data_ptr(), np.float32, sp, 1, 3, raw)
    assert B.cloud_view_extent(v) == (0, (2 * sp + 3) * 4) and B.cloud_view_extent(v)[1] <= raw.numel()
    ctx.set_cloud_view(0, v)
    _same_bits(ctx.get_cloud(0), P.astype(np.float64))
    # ... and walked from the far end (negative offsets of the same size)
    ctx.set_cloud_view(0, _view(B, raw.data_ptr() + 2 * sp * 4, np.float32, -sp, 1, 3, raw))
    _same_bits(ctx.get_cloud(0), P[::-1].astype(np.float64))
    del f, raw


def _param_sets(B, P):
    return [B.make_params(P["beta"], P["lambda_"], P["lle_weight"], P["mu"], 12, 0.0, False, precision=0),
            B.make_params(P["beta"], P["lambda_"], P["lle_weight"], P["mu"], 12, 0.0, False, P["alpha"], P["k_vis"], P["visibility_threshold"], precision=1),
            B.make_params(P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"], P["mu"], 8, 0.0, True, precision=0),
            B.make_params(P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"], P["mu"], 8, 0.0, True, precision=1)]


def _same_reg(a, b):
    _same_bits(a["Y"], b["Y"])
    assert np.float64(a["sigma2"]).view(np.uint64) == np.float64(b["sigma2"]).view(np.uint64)
    for k in ("iters", "n_kept", "status", "converged", "rc"):
        assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("N", [5000, 20000])
def test_registration_from_a_view_equals_the_double_path(B, ctx, torch, N):
    from trackdlo_amd import synth
    M = 45
    X, Y0, vis = synth.scene(N, M, config=31, occlude=(0.4, 0.55), outliers=7)
    vext = synth.extend_visible(vis, M, synth.geodesic_coord(Y0))
    X32 = np.ascontiguousarray(X.astype(np.float32))                   # row-major float32, as Open3D or a PointCloud2 buffer holds it
    assert np.array_equal(X32.astype(np.float64), X)
    Xd = torch.from_numpy(X32).cuda()
    for i, p in enumerate(_param_sets(B, synth.LAUNCH_PARAMS)):
        kw = dict(visible_nodes=vext) if i == 1 else {}
        s2 = 3e-5 if p.include_lle else 0.0
        want = ctx.cpd_lle(X, Y0, s2, p, **kw)
        for src in (X32, Xd):
            ctx.set_cloud_view(0, src)
            got = ctx.cpd_lle_resident(0, Y0, s2, p, **kw)
            assert got["sort_reused"] == 0
            _same_reg(got, want)


def _trackers(B, M, Y0, precision=0):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    out = []
    for _ in range(2):
        c = B.Context(device=0, max_points=1 << 15, max_nodes=64, timing=False)
        t = B.trackdlo(*args, ctx=c, precision=precision)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
        out.append((c, t))
    return out


def _same_tracker_state(a, b):
    _same_bits(a.get_tracking_result(), b.get_tracking_result())
    _same_bits(a.get_guide_nodes(), b.get_guide_nodes())
    pa, pb = a.get_correspondence_pairs(), b.get_correspondence_pairs()
    assert pa.shape == pb.shape and len(pa) > 0 and np.array_equal(pa.view(np.uint64), pb.view(np.uint64))
    assert np.float64(a.get_sigma2()).view(np.uint64) == np.float64(b.get_sigma2()).view(np.uint64)
    for sa, sb in zip(a.last_stats, b.last_stats):
        for k in ("iters", "converged", "n_kept", "status", "band_retry"):
            assert sa[k] == sb[k], (k, sa[k], sb[k])


def _routes(c):
    return [int(c.lib.tdlo_debug_route_count(c.h, k)) for k in (17, 18)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_tracker_small_frame_from_a_host_view(B, dtype):
    """Three frames of a moving rope at production size: the host view is widened straight into the pinned staging (route 18), and the frame is the
    route of the double call from there on -- the same bits, the paired registrations (sort_reused == 2), no import kernel."""
    from trackdlo_amd import synth
    N, M = 5000, 45
    _, Y0, _ = synth.scene(N, M, config=52)
    (ca, ta), (cb, tb) = _trackers(B, M, Y0)
    try:
        v = np.arange(M, dtype=np.int32)
        for fr in range(3):
            X, _, _ = synth.scene(N, M, config=52, frame=fr)
            wide = np.full((N, 8), np.nan, dtype=dtype); wide[:, :3] = X          # PointXYZRGB's stride
            assert np.array_equal(wide[:, :3].astype(np.float64), X)
            ta.tracking_step_view(wide, v, v)
            tb.tracking_step(X, v, v)
            _same_tracker_state(ta, tb)
            assert ta.last_stats[1]["sort_reused"] == 2 and tb.last_stats[1]["sort_reused"] == 2
            assert _routes(ca) == [0, fr + 1] and _routes(cb) == [0, 0]
            _same_bits(ca.get_cloud(0), X)
        assert ca.route_counts() == cb.route_counts()
    finally:
        ca.close(); cb.close()


@pytest.mark.parametrize("case", ["device-5000", "host-20000"])
def test_tracker_from_a_device_view_or_a_large_frame(B, torch, case):
    """The import kernel in front of the X == NULL route (route 17 once per frame): three frames with every node visible, then one with a stretch hidden."""
    from trackdlo_amd import synth
    N, M = (5000, 45) if case == "device-5000" else (20000, 45)
    _, Y0, _ = synth.scene(N, M, config=53)
    (ca, ta), (cb, tb) = _trackers(B, M, Y0)
    try:
        coord = synth.geodesic_coord(Y0)
        for fr in range(4):
            X, _, vis = synth.scene(N, M, config=53, frame=min(fr, 2), occlude=(0.45, 0.55) if fr == 3 else None)
            assert case == "device-5000" or X.shape[0] > 16384          # (beyond the staged route's limit on every frame, the occluded one too)
            v = np.arange(M, dtype=np.int32) if fr < 3 else np.asarray(vis, dtype=np.int32)
            ve = v if fr < 3 else synth.extend_visible(vis, M, coord)
            assert (len(ve) < M) == (fr == 3)
            X32 = np.ascontiguousarray(X.astype(np.float32))
            src = torch.from_numpy(X32).cuda() if case == "device-5000" else X32
            ta.tracking_step_view(src, v, ve)
            tb.tracking_step(X, v, ve)
            _same_tracker_state(ta, tb)
            assert _routes(ca) == [fr + 1, 0] and _routes(cb) == [0, 0]
            _same_bits(ca.get_cloud(0), X)
    finally:
        ca.close(); cb.close()


def test_non_finite_rows(B, ctx, torch):
    """1 % of the points are NaN, +Inf or -Inf rows: widened as (double) widens them, dropped by the prune as on the double path."""
    from trackdlo_amd import synth
    N, M = 5000, 45
    X, Y0, _ = synth.scene(N, M, config=61)
    X32 = np.ascontiguousarray(X.astype(np.float32))
    rows = np.random.default_rng(61).choice(N, N // 100, replace=False)
    X32[rows[0::3]] = np.nan; X32[rows[1::3]] = np.inf; X32[rows[2::3]] = -np.inf
    X32[rows[0], 1:] = 1.0                                        # (one row with a single bad component)
    want = R.widen(X32, np.float32, 0, 3, 1, N)
    nan = np.isnan(want)
    assert nan.any() and np.isinf(want).any()
    p = _param_sets(B, synth.LAUNCH_PARAMS)[0]
    ref = ctx.cpd_lle(want, Y0, 0.0, p)
    assert ref["n_kept"] <= N - len(rows)
    for src in (X32, torch.from_numpy(X32).cuda()):
        ctx.set_cloud_view(0, src)
        got = ctx.get_cloud(0)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(np.where(nan, 0.0, got)), _bits(np.where(nan, 0.0, want)))
        _same_reg(ctx.cpd_lle_resident(0, Y0, 0.0, p), ref)


def test_set_cloud_view_invalidates_the_sorted_cloud(B, ctx):
    from trackdlo_amd import synth
    N, M = 5000, 45
    X, Y0, _ = synth.scene(N, M, config=62)
    X32 = np.ascontiguousarray(X.astype(np.float32))
    p = _param_sets(B, synth.LAUNCH_PARAMS)[0]
    ctx.set_cloud_view(0, X32)
    first = ctx.cpd_lle_resident(0, Y0, 0.0, p)
    again = ctx.cpd_lle_resident(0, Y0, 0.0, p)
    assert first["sort_reused"] == 0 and again["sort_reused"] == 1           # (the slot holds a sorted cloud)
    ctx.set_cloud_view(0, X32)
    after = ctx.cpd_lle_resident(0, Y0, 0.0, p)
    assert after["sort_reused"] == 0
    _same_reg(after, first); _same_reg(again, first)


@pytest.mark.parametrize("asynchronous", [False, True], ids=["waits", "async"])
def test_ready_stream_orders_the_import_behind_the_producer(B, ctx, torch, asynchronous):
    """The tensor is filled on a side stream behind a few hundred milliseconds of matrix products; the import is handed that stream at once."""
    N = 4099
    P = np.random.default_rng(8).standard_normal((N, 3)).astype(np.float32)
    src = torch.from_numpy(P).cuda()
    dst = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    A = torch.randn((8192, 8192), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    (A @ A).sum().item()                                          # (the BLAS library's first call is out of the way)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(30):
            A = (A @ A) * 1e-4
        dst.copy_(src)
    ctx.set_cloud_view(0, dst, ready_stream=side.cuda_stream, asynchronous=asynchronous)
    if asynchronous:
        assert not side.query()                                   # (the call did not wait on the host: the producer is still running)
        ctx.synchronize()
    _same_bits(ctx.get_cloud(0), P.astype(np.float64))
    torch.cuda.synchronize()


def test_refusals_leave_the_slot_as_it_was(B, ctx):
    lib = ctx.lib
    X = np.asfortranarray(np.random.default_rng(9).standard_normal((300, 3)))
    ctx.set_cloud(0, X)
    buf = np.zeros((300, 3), dtype=np.float32)
    good = B.cloud_view(buf)
    bad_dtype = B.cloud_view(buf); bad_dtype.dtype = 7
    assert lib.tdlo_set_cloud_view(ctx.h, 0, C.byref(good), 0) == B.TDLO_E_INVALID
    assert lib.tdlo_set_cloud_view(ctx.h, 0, C.byref(bad_dtype), 300) == B.TDLO_E_INVALID
    assert lib.tdlo_set_cloud_view(ctx.h, 0, None, 300) == B.TDLO_E_INVALID
    assert lib.tdlo_set_cloud_view(ctx.h, 99, C.byref(good), 300) == B.TDLO_E_INVALID
    assert b"cloud view" in lib.tdlo_last_error(ctx.h) or b"slot" in lib.tdlo_last_error(ctx.h)
    _same_bits(ctx.get_cloud(0), X)
    out = np.zeros((299, 3), order="F"); n = C.c_int(-1)
    assert lib.tdlo_get_cloud(ctx.h, 0, out.ctypes.data_as(C.c_void_p), 299, C.byref(n)) == B.TDLO_E_INVALID and n.value == 300
    assert not out.any()
    trk = B.trackdlo(45, ctx=ctx)
    st = (B.Stats * 2)()
    v = np.arange(45, dtype=np.int32)
    assert lib.tdlo_tracker_tracking_step_view(trk.h, C.byref(bad_dtype), 300, v.ctypes.data_as(C.c_void_p), 45, v.ctypes.data_as(C.c_void_p), 45, None, C.cast(st, C.c_void_p)) == B.TDLO_E_INVALID
    _same_bits(ctx.get_cloud(0), X)


def test_existing_calls_are_read_back_unchanged(B, ctx):
    from trackdlo_amd import synth
    X = np.asfortranarray(np.random.default_rng(10).standard_normal((4099, 3)))
    X[5, 1] = np.float64(1) / 3                                   # (not a float32 value: the double path keeps all 64 bits)
    ctx.set_cloud(0, X)
    _same_bits(ctx.get_cloud(0), X)
    depth, mask, cam, _ = synth.depth_scene(30, config=9, frame=2)
    Xg, n, _ = ctx.depth_to_cloud(1, depth, mask, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.008)
    assert n > 0
    _same_bits(ctx.get_cloud(1), Xg)
    _same_bits(ctx.get_cloud(0), X)


def test_cpp_view_overloads():
    """include/trackdlo_shim.hpp: tdlo::view_of on a float cloud at a 32-byte point stride into tracking_step and cpd_lle, against the Matrix overloads
    on the widened cloud, inside the C++ program (tests/cpp/view_test.cpp, built by __graft_entry__.build())."""
    exe = os.path.join(ROOT, "tests", "cpp", "view_test")
    assert os.path.exists(exe), "tests/cpp/view_test is missing: run __graft_entry__.build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout
