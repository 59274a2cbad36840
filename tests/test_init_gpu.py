"""GPU suite of the chain order and of a tracker started from its first cloud: k_sort_pts (csrc/tdlo_init.hip) against the numpy statement of
utils.cpp:95-170 (tests/init_ref.py) -- permutation exactly, nodes and chain coordinate bit for bit, both forms of the kernel on both sides of
their boundary --, what it refuses, and tdlo_tracker_initialize_from_cloud*: reg and the ordering composed on the device, on every route a cloud
can take into the slot, against statement(tdlo_reg(the same cloud)); the tracker it leaves behind against one given the same nodes and coordinates
by hand, and a refused call against an untouched twin."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT
import init_ref as R
import reg_ref

pytestmark = pytest.mark.gpu

MU, ITERS = 0.05, 20
CLOUDS = [(300, 8), (3000, 40)]                       # (points, nodes) of the composed call


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    return binding


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(device=0, timing=False)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _tracker(B, ctx, M, precision=None):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    return B.trackdlo(M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"],
                      P["lambda_pre_proc"], P["lle_weight"], ctx=ctx, precision=B.PREC_F64 if precision is None else precision)


_EXPECT = {}


def _expected(ctx, N, M):
    """(cloud, statement(tdlo_reg(cloud)), reg's sigma2), once per module."""
    if (N, M) not in _EXPECT:
        X = R.rope_cloud(N, seed=N + M)
        Yr, s2 = ctx.reg(X, M, MU, ITERS)
        st = R.statement(Yr)
        assert st["status"] == 0
        _EXPECT[(N, M)] = (X, st, s2, Yr)
    return _EXPECT[(N, M)]


# ---- ordering ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.scenes()))
def test_ordering_equals_the_statement(ctx, name):
    """M <= 64: the one-wave form; M >= 65: the workgroup form (63 | 64 | 65, 256 | 257, 890, 1024 are among the scenes)."""
    Y = R.scenes()[name]
    ref = R.ref(name)
    before = ctx.init_route_counts()
    Ys, perm, coord = ctx.sort_pts(Y)
    assert np.array_equal(perm, ref["perm"])
    assert _same(Ys, ref["Y"]) and _same(coord, ref["coord"])
    assert ctx.init_route_counts() == [before[0] + 1, before[1]]


def test_optional_outputs_and_in_place(ctx, B):
    Y = np.asfortranarray(R.scenes()["rope65"]); ref = R.ref("rope65")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    perm = np.zeros(len(Y), dtype=np.int32)
    assert ctx.lib.tdlo_sort_pts(ctx.h, p(Y), len(Y), None, p(perm), None) == 0 and np.array_equal(perm, ref["perm"])
    assert ctx.lib.tdlo_sort_pts(ctx.h, p(Y), len(Y), p(Y), None, None) == 0 and _same(Y, ref["Y"])


def test_refused_inputs_leave_the_outputs_alone(ctx, B):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for n, (Y, st) in R.error_inputs().items():
        Yf = np.asfortranarray(Y)
        Ys = np.full(Yf.shape, 7.0, order="F"); perm = np.full(len(Y), -7, dtype=np.int32); coord = np.full(len(Y), 7.0)
        assert ctx.lib.tdlo_sort_pts(ctx.h, p(Yf), len(Y), p(Ys), p(perm), p(coord)) == B.TDLO_E_NUMERIC, n
        assert (Ys == 7.0).all() and (perm == -7).all() and (coord == 7.0).all(), n
        msg = ctx.lib.tdlo_last_error(ctx.h).decode()
        assert ("non-finite", "coincide", "no edge")[st - 1] in msg, (n, msg)
    Y = np.asfortranarray(R.scenes()["end_first"])
    Ys = np.full(Y.shape, 7.0, order="F")
    for M in (1, 0, -1, 1025):
        assert ctx.lib.tdlo_sort_pts(ctx.h, p(Y), M, p(Ys), None, None) == B.TDLO_E_INVALID and (Ys == 7.0).all()
    assert ctx.lib.tdlo_sort_pts(ctx.h, None, 5, p(Ys), None, None) == B.TDLO_E_INVALID
    assert ctx.lib.tdlo_sort_pts(None, p(Y), len(Y), p(Ys), None, None) == B.TDLO_E_INVALID
    for name in ("rope64", "rope257"):                 # a good call afterwards on the same context is still right
        Ys, perm, coord = ctx.sort_pts(R.scenes()[name])
        assert np.array_equal(perm, R.ref(name)["perm"]) and _same(coord, R.ref(name)["coord"])


# ---- composition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", CLOUDS)
def test_initialize_from_cloud_is_the_statement_of_reg(ctx, B, N, M):
    X, st, s2, Yr = _expected(ctx, N, M)
    trk = _tracker(B, ctx, M)
    before = ctx.init_route_counts()
    got = trk.initialize_from_cloud(X, MU, ITERS)
    assert _same(trk.get_tracking_result(), st["Y"]) and _same([got], [s2])
    assert trk.get_sigma2() == 0.0                                           # the tracker's own sigma2 is left alone
    assert _same(trk.get_guide_nodes(), st["Y"])
    assert ctx.init_route_counts() == [before[0] + 1, before[1]]
    # reg on its own is not disturbed by the ordering that now shares its workspace: the same bits as before
    Y2, s22 = ctx.reg(X, M, MU, ITERS)
    assert _same(Y2, Yr) and _same([s22], [s2])
    # the resident route: X == NULL after tdlo_set_cloud
    ctx.set_cloud(0, X)
    trk2 = _tracker(B, ctx, M)
    assert _same([trk2.initialize_from_cloud(None, MU, ITERS)], [s2]) and _same(trk2.get_tracking_result(), st["Y"])
    # the view routes: a device tensor at its own strides, and a host view
    import torch
    t = torch.from_numpy(np.ascontiguousarray(X)).cuda()                     # N x 3 row-major on the device
    torch.cuda.synchronize()
    trk3 = _tracker(B, ctx, M)
    assert _same([trk3.initialize_from_cloud_view(t, MU, ITERS)], [s2]) and _same(trk3.get_tracking_result(), st["Y"])
    trk4 = _tracker(B, ctx, M)
    assert _same([trk4.initialize_from_cloud_view(np.ascontiguousarray(X), MU, ITERS)], [s2]) and _same(trk4.get_tracking_result(), st["Y"])
    assert ctx.init_route_counts() == [before[0] + 4, before[1]]
    # calling it again REPLACES nodes and coordinates (a second call's tracker steps like a first call's: test_tracker_started_this_way_...)
    assert _same([trk.initialize_from_cloud(X, MU, ITERS)], [s2]) and _same(trk.get_tracking_result(), st["Y"])


def test_reg_stays_inside_its_own_gate(ctx):
    """tdlo_reg is the code of before behind a helper: held here to the extended-precision reference and gate of tests/reg_ref.py on this suite's cloud."""
    N, M = CLOUDS[0]
    X, _, s2, Yr = _expected(ctx, N, M)
    qy, qs = reg_ref.ratio(Yr, s2, reg_ref.propagated(X, M, MU, ITERS))
    assert qy <= 1.0 and qs <= 1.0, (qy, qs)


def _depth_image():
    """A small constructed frame: a sine stripe three pixels thick, 0.55 .. 0.65 m away."""
    rows, cols = 48, 64
    depth = np.zeros((rows, cols), dtype=np.uint16); mask = np.zeros((rows, cols), dtype=np.uint8)
    for u in range(2, cols - 2):
        v = int(round(24 + 14 * np.sin(u / 9.0)))
        mask[v - 1:v + 2, u] = 255
        depth[v - 1:v + 2, u] = 600 + int(round(50 * np.cos(u / 7.0)))
    return depth, mask, (80.0, 80.0, 32.0, 24.0)


def test_a_cloud_born_on_the_device_becomes_a_tracker(ctx, B):
    depth, mask, cam = _depth_image()
    M = 8
    Xd, n, _ = ctx.depth_to_cloud(0, depth, mask, *cam, 0.008)
    assert n > 60
    Yr, s2 = ctx.reg(Xd, M, MU, ITERS)
    st = R.statement(Yr)
    assert st["status"] == 0
    ctx.depth_to_cloud(0, depth, mask, *cam, 0.008, fetch=False)             # the cloud is where the kernel left it
    trk = _tracker(B, ctx, M)
    assert _same([trk.initialize_from_cloud(None, MU, ITERS)], [s2]) and _same(trk.get_tracking_result(), st["Y"])


_HOST_CHILD = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    import numpy as np
    import init_ref as R
    import test_init_gpu as T
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, timing=False)
    out = {}
    for N, M in T.CLOUDS:
        trk = T._tracker(B, ctx, M)
        out[f"s2_{N}"] = np.array([trk.initialize_from_cloud(R.rope_cloud(N, seed=N + M), T.MU, T.ITERS)])
        out[f"Y_{N}"] = trk.get_tracking_result()
    out["routes"] = np.array(ctx.init_route_counts())
    try:
        T._tracker(B, ctx, 8).initialize_from_cloud(T.reg_ref.nan_cloud(), T.MU, 3)
        out["refused"] = np.array([0])
    except B.TdloError as e:
        out["refused"] = np.array([e.code])
    np.savez(sys.argv[2], **out)
    print("OK")
""")


def test_host_ordered_route_gives_the_same_bits(ctx, B, tmp_path):
    """TDLO_INIT_SORT=host, read when the context is made: a fresh child process."""
    env = dict(os.environ, TDLO_INIT_SORT="host")
    out = str(tmp_path / "host.npz")
    r = subprocess.run([sys.executable, "-c", _HOST_CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    z = np.load(out)
    assert z["routes"].tolist() == [0, len(CLOUDS)] and int(z["refused"][0]) == B.TDLO_E_NUMERIC
    for N, M in CLOUDS:
        _, st, s2, _ = _expected(ctx, N, M)
        assert _same(z[f"Y_{N}"], st["Y"]) and _same(z[f"s2_{N}"], [s2])


# ---- the tracker it leaves behind ----------------------------------------------------------------------------------------------------------
def _step(trk, X, M):
    v = np.arange(M, dtype=np.int32)
    trk.tracking_step(X, v, v)
    return trk.get_tracking_result(), trk.get_sigma2()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_tracker_started_this_way_steps_like_one_started_by_hand(B, precision):
    N, M = CLOUDS[1]
    prec = B.PREC_F32 if precision == "f32" else B.PREC_F64
    a = B.Context(device=0, timing=False); b = B.Context(device=0, timing=False)
    try:
        X, st, s2, _ = _expected(a, N, M)
        X2 = np.asfortranarray(X + np.array([0.0, 0.004, 0.0]))
        ta = _tracker(B, a, M, prec); tb = _tracker(B, b, M, prec)
        ta.initialize_geodesic_coord(np.arange(3.0))                         # what was there is replaced, not appended to
        ta.initialize_from_cloud(X, MU, ITERS)
        ta.initialize_from_cloud(X, MU, ITERS)
        tb.initialize_nodes(st["Y"]); tb.initialize_geodesic_coord(st["coord"])
        ta.set_sigma2(s2); tb.set_sigma2(s2)
        for X_k in (X2, X):
            Ya, sa = _step(ta, X_k, M); Yb, sb = _step(tb, X_k, M)
            assert _same(Ya, Yb) and _same([sa], [sb])
            assert [s["iters"] for s in ta.last_stats] == [s["iters"] for s in tb.last_stats]
        assert np.isfinite(Ya).all() and not _same(Ya, st["Y"])
    finally:
        a.close(); b.close()


def test_a_refused_call_leaves_the_tracker_as_it_was(B):
    """reg_ref.nan_cloud() is its case's cloud; the case's one node is fewer than a tracker's four, so the same point with M = 8, proved here with
    reg_ref's fp64 restatement to coincide after one iteration (status 2) and to be NaN after three (status 1)."""
    N, M = CLOUDS[0]
    Xn = reg_ref.nan_cloud()
    Y1, _ = reg_ref.reg_fp64(Xn, M, MU, 1); Y3, _ = reg_ref.reg_fp64(Xn, M, MU, 3)
    assert np.isfinite(Y1).all() and (Y1 == Y1[0]).all() and np.isnan(Y3).all()
    a = B.Context(device=0, timing=False); b = B.Context(device=0, timing=False); e = B.Context(device=0, timing=False)
    try:
        X, st, s2, _ = _expected(a, N, M)
        ta = _tracker(B, a, M); tb = _tracker(B, b, M)
        for t in (ta, tb):
            t.initialize_nodes(st["Y"]); t.initialize_geodesic_coord(st["coord"]); t.set_sigma2(s2)
        p = lambda arr: arr.ctypes.data_as(C.c_void_p)
        lib = a.lib
        s_out = C.c_double(-1.0)
        Xf = np.asfortranarray(X)
        calls = [
            (lambda: lib.tdlo_tracker_initialize_from_cloud(ta.h, p(Xn), 1, MU, 3, C.byref(s_out)), B.TDLO_E_NUMERIC, "non-finite"),
            (lambda: lib.tdlo_tracker_initialize_from_cloud(ta.h, p(Xn), 1, MU, 1, C.byref(s_out)), B.TDLO_E_NUMERIC, "coincide"),
            (lambda: lib.tdlo_tracker_initialize_from_cloud(ta.h, p(Xf), 0, MU, ITERS, C.byref(s_out)), B.TDLO_E_INVALID, "empty"),
            (lambda: lib.tdlo_tracker_initialize_from_cloud(ta.h, p(Xf), -5, MU, ITERS, C.byref(s_out)), B.TDLO_E_INVALID, "empty"),
            (lambda: lib.tdlo_tracker_initialize_from_cloud(ta.h, p(Xf), N, 1.0, ITERS, C.byref(s_out)), B.TDLO_E_INVALID, "bad reg"),
            (lambda: lib.tdlo_tracker_initialize_from_cloud(ta.h, p(Xf), N, MU, -1, C.byref(s_out)), B.TDLO_E_INVALID, "bad reg"),
        ]
        for call, code, word in calls:
            assert call() == code and word in lib.tdlo_last_error(a.h).decode(), (code, word, lib.tdlo_last_error(a.h).decode())
            assert s_out.value == -1.0
            assert _same(ta.get_tracking_result(), st["Y"]) and _same([ta.get_sigma2()], [s2]) and _same(ta.get_guide_nodes(), st["Y"])
        assert lib.tdlo_tracker_initialize_from_cloud(None, p(Xf), N, MU, ITERS, None) == B.TDLO_E_INVALID
        assert lib.tdlo_tracker_initialize_from_cloud_view(ta.h, None, N, MU, ITERS, None) == B.TDLO_E_INVALID
        # the limits on the node count, and an empty slot: trackers of a context of their own
        for Mbad in (3, 891):
            tbad = _tracker(B, e, Mbad)
            assert lib.tdlo_tracker_initialize_from_cloud(tbad.h, p(Xf), N, MU, ITERS, None) == B.TDLO_E_INVALID
        tempty = _tracker(B, e, M)
        assert lib.tdlo_tracker_initialize_from_cloud(tempty.h, None, 0, MU, ITERS, None) == B.TDLO_E_INVALID
        assert "resident" in lib.tdlo_last_error(e.h).decode() and not tempty.get_tracking_result().any()
        # the next step is the untouched twin's (the twin's context has seen none of this)
        X2 = np.asfortranarray(X + np.array([0.0, 0.004, 0.0]))
        Ya, sa = _step(ta, X2, M); Yb, sb = _step(tb, X2, M)
        assert _same(Ya, Yb) and _same([sa], [sb]) and np.isfinite(Ya).all()
    finally:
        a.close(); b.close(); e.close()


def test_drop_in_class_from_plain_cpp(tmp_path):
    """tests/cpp/init_shim_test.cpp: trackdlo::initialize_from_cloud on a matrix and on a float view, and the free sort_pts, through include/trackdlo_shim.hpp."""
    exe = str(tmp_path / "init_shim_test")
    lib_dir = os.path.join(ROOT, "trackdlo_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "init_shim_test.cpp"), "-L" + lib_dir, "-ltrackdlo_hip",
                        "-Wl,-rpath," + lib_dir, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout[-1500:], r.stderr[-3000:])
