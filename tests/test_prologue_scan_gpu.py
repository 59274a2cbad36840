"""The two-launch prologue -- k_prune_nodes (k_prune_pass1 with the node work of setup_body in a workgroup beside it) and k_scatter_scan
(k_prune_scatter whose workgroups form their own start offsets from the counts) -- against the exact reference of tests/setup_ref.py, through
check_frame / run_single of tests/test_setup_gpu.py, and bit for bit against the three-kernel form it replaces (TDLO_PROLOGUE_SCAN=0).

Every context here has TDLO_DIRECT_UPLOAD=0, so that clouds of up to 16 384 points reach the new route instead of k_prologue.  The route serves
calls whose frames all sort afresh with one tile per workgroup, nb <= 256 prune workgroups and M <= 64 nodes; tdlo_debug_route_count 48
(Context.prologue_scan_calls) counts them.  A thread of k_scatter_scan is (node = lane, quarter of the blocks = wave); the launcher picks the
kernel's tier by the call's largest nb (<= 16: 4 loads per thread, <= 64: 16, <= 128: 32, else 64), so the shapes sit either side of every tier:
nb = 1, 2, 3, 5 (empty and uneven quarters), 64 / 65, 196 (the headline's geometry), 255 / 256 (the cap) and 257 (not served)."""
import ctypes as C

import numpy as np
import pytest

import test_setup_gpu as T

pytestmark = pytest.mark.gpu

ENV_SCAN = {"TDLO_DIRECT_UPLOAD": 0, "TDLO_PROLOGUE_SCAN": None}
ENV_THREE = {"TDLO_DIRECT_UPLOAD": 0, "TDLO_PROLOGUE_SCAN": 0}
MAX_POINTS = 257 * 256


@pytest.fixture(scope="module")
def scan():
    ctx = T.make_ctx(ENV_SCAN, max_points=MAX_POINTS, max_nodes=128)
    ctx.set_sort_reuse(False)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def three():
    ctx = T.make_ctx(ENV_THREE, max_points=MAX_POINTS, max_nodes=128)
    ctx.set_sort_reuse(False)
    yield ctx
    ctx.close()


def read_backs(ctx, N0, M, frame=0):
    """What the prologue left for a frame of the last call, as arrays."""
    cloud, ctr = ctx.debug_read_cloud(N0, frame)
    out = dict(cloud=cloud, ctr=ctr)
    for what in ("keep", "Y0", "nodes", "coord", "chain"):
        out[what] = ctx.debug_read_setup(what, M, frame)
    out["sigma2"] = np.array([ctx.debug_read_setup("sigma2", M, frame)])
    return out


def same_arrays(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        assert x.shape == y.shape and np.array_equal(T.bits(x), T.bits(y)), (label, k)


def results(ctx, sc, prec, max_iter):
    g = ctx.cpd_lle(sc["X"], sc["Y0"], 0.0, T.params(prec, max_iter=max_iter), check=False)
    return dict(Y=g["Y"], sigma2=np.array([g["sigma2"]]), iters=np.array([g["iters"]]), n_kept=np.array([g["n_kept"]]), rc=np.array([g["rc"]]))


def both_routes(scan, three, sc, prec, label, key, served=True):
    """The scene on both contexts: the exact reference on the new route (run_single), the read-backs after one iteration and the results after
    three equal as arrays, the route counter up by one per call (served) or not at all."""
    N0, M = len(sc["X"]), len(sc["Y0"])
    c0, t0 = scan.prologue_scan_calls(), three.prologue_scan_calls()
    T.run_single(scan, sc, prec, label + "-scan", key=key)
    a = read_backs(scan, N0, M)
    T.run_single(three, sc, prec, label + "-three kernels", key=key)
    b = read_backs(three, N0, M)
    same_arrays(a, b, label + " after one iteration")
    same_arrays(results(scan, sc, prec, 3), results(three, sc, prec, 3), label + " after three iterations")
    assert scan.prologue_scan_calls() == c0 + (2 if served else 0), (label, "route counter", scan.prologue_scan_calls() - c0)
    assert three.prologue_scan_calls() == t0, (label, "TDLO_PROLOGUE_SCAN=0 took the new route")


# ---- 1, 2: the shapes at the edges of the scan ------------------------------------------------------------------------------------------
NB_ALL = [1, 2, 3, 5, 64, 65, 196, 255, 256]
SHAPES = [(nb, k, 50) for nb in NB_ALL for k in (0, 1, 255)] + [(nb, 1, M) for M in (5, 8, 63, 64) for nb in (3, 65)]


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("nb,k,M", SHAPES, ids=[f"nb{nb}-k{k}-M{M}" for nb, k, M in SHAPES])
def test_shapes_at_the_edges_of_the_scan(scan, three, nb, k, M, prec):
    N0 = nb * 256 - k
    assert T.prune_geometry(N0) == (1, nb)
    sc = T.scene_plain(N0, M, 900, outliers=min(7, N0 // 2))
    both_routes(scan, three, sc, prec, f"scan-nb{nb}-k{k}-M{M}-p{prec}", ("plain", N0, M))


# ---- 3: calls the route does not serve ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("N0,M", [(257 * 256, 50), (3000, 65)], ids=["nb257", "M65"])
def test_not_eligible_by_size(scan, three, N0, M, prec):
    sc = T.scene_plain(N0, M, 900, outliers=7)
    both_routes(scan, three, sc, prec, f"scan-not-N{N0}-M{M}-p{prec}", ("plain", N0, M), served=False)


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_not_eligible_split_route(prec):
    """tdlo_split_begin keeps its own three kernels: the counter stays, the stage holds to the reference."""
    from trackdlo_amd import nsplit
    N0, M = 6000, 45
    sc = T.scene_shell(N0, M, cfg=980)
    r = T.reference(sc, ("shell980", N0, M))
    ctx = T.make_ctx(ENV_SCAN, max_points=N0, max_nodes=64)
    try:
        sh = nsplit.HipShard(ctx, sc["X"])
        init = sh.begin(sc["Y0"], 0.0, T.params(prec, max_iter=5), None, None, None)
        try:
            T.check_frame(ctx, 0, sc, r, prec, f"scan-split-p{prec}", n_kept_seen=[init[0]], split=True, pristine_nodes=True)
        finally:
            sh.abort()
        assert ctx.prologue_scan_calls() == 0
    finally:
        ctx.close()


# ---- 6 (and 3): the sort reused by the next call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_sort_reuse_reads_what_the_route_left(prec):
    """The same inputs twice with the reuse on: the second call skips prune and scatter, its set-up kernel reads keep[] as fused_iter0 left it
    (kept count, sum of d2); it is not served by the new route and returns the first call's results."""
    N0, M = 65 * 256 - 1, 50
    sc = T.scene_plain(N0, M, 900, outliers=7)
    ctx = T.make_ctx(ENV_SCAN, max_points=N0, max_nodes=64)
    try:
        ctx.set_sort_reuse(True)
        ctx.set_cloud(0, sc["X"])
        p = T.params(prec, max_iter=3)
        a = ctx.cpd_lle_resident(0, sc["Y0"], 0.0, p)
        assert a["sort_reused"] == 0 and ctx.prologue_scan_calls() == 1
        b = ctx.cpd_lle_resident(0, sc["Y0"], 0.0, p)
        assert b["sort_reused"] == 1 and ctx.prologue_scan_calls() == 1
        for k in ("Y", "sigma2", "iters", "n_kept"):
            assert np.array_equal(T.bits(np.asarray(a[k], dtype=np.float64)), T.bits(np.asarray(b[k], dtype=np.float64))), k
        assert a["n_kept"] > 0 and a["iters"] == 3
    finally:
        ctx.close()


# ---- 4: run structure ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["node0", "even", "blocks", "nonfinite", "empty"])
def test_run_structure(scan, three, kind, prec):
    """Every kept point on node 0; half the nodes without a point; whole blocks pruned away (zero rows in the counts); non-finite coordinates;
    nothing kept (TDLO_E_EMPTY, n_kept == 0, an empty sorted cloud: run_single asserts them)."""
    sc = T.scene_runs(kind)
    both_routes(scan, three, sc, prec, f"scan-runs-{kind}-p{prec}", ("runs", kind))
    if kind == "empty":                                    # ... and the context is usable afterwards
        T.run_single(scan, T.scene_runs("blocks"), prec, f"scan-after-empty-p{prec}", key=("runs", "blocks"))


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_threshold_shell_at_65_blocks(scan, three, prec):
    N0, M = 65 * 256 - 3, 50
    sc = T.scene_shell(N0, M)
    both_routes(scan, three, sc, prec, f"scan-shell-N{N0}-p{prec}", ("shell", N0, M, None))


# ---- 5: a batch of ragged frames ------------------------------------------------------------------------------------------------------------
def _batch(env, scs, M, prec, max_iter):
    from trackdlo_amd import binding as B
    F = len(scs)
    ctx = T.make_ctx(env, max_frames=F, max_points=max(len(sc["X"]) for sc in scs), max_nodes=64)
    ctx.set_sort_reuse(False)
    for f, sc in enumerate(scs):
        ctx.set_cloud(f, sc["X"])
    Yb = np.ascontiguousarray(np.asarray([sc["Y0"] for sc in scs]).transpose(0, 2, 1))
    s2 = np.zeros(F); st = (B.Stats * F)()
    p = T.params(prec, max_iter=max_iter)
    rc = ctx.lib.tdlo_cpd_lle_batch(ctx.h, F, B._ptr(Yb), M, B._ptr(s2), C.byref(p), None, 0, None, 0, None, C.cast(st, C.c_void_p))
    assert rc in (0, B.TDLO_E_EMPTY), rc
    return ctx, Yb, s2, st


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_batch_of_three_ragged_frames(prec):
    """cpd_lle_batch: 20, 3 (nothing kept) and 2 prune workgroups -- the blocks beyond a frame's count fall through, and the node workgroup is
    the launch's last column of workgroups, not a frame's nb-th.  Every frame against the reference and against the three-kernel form."""
    from trackdlo_amd import binding as B
    M = 50
    scs = [T.scene_shell(5000, M, cfg=970), T.scene_runs("empty", 700, M, 972), T.scene_plain(257, M, 974)]
    keys = [("shell970", 5000, M), ("empty972", 700, M), ("plain974", 257, M)]
    a, _, _, st = _batch(ENV_SCAN, scs, M, prec, 1)
    b, _, _, _ = _batch(ENV_THREE, scs, M, prec, 1)
    try:
        assert a.prologue_scan_calls() == 1 and b.prologue_scan_calls() == 0
        for f, sc in enumerate(scs):
            r = T.reference(sc, keys[f])
            T.caps(sc, r)
            if r["n_kept"] == 0:
                assert st[f].status == B.TDLO_E_EMPTY and st[f].n_kept == 0
                assert len(a.debug_read_cloud(len(sc["X"]), f)[0]) == 0 and len(b.debug_read_cloud(len(sc["X"]), f)[0]) == 0
                continue
            assert st[f].status == 0 and st[f].iters == 1, (f, st[f].status)
            T.check_frame(a, f, sc, r, prec, f"scan-batch-frame{f}-p{prec}", n_kept_seen=[st[f].n_kept])
            same_arrays(read_backs(a, len(sc["X"]), M, f), read_backs(b, len(sc["X"]), M, f), f"scan-batch-frame{f}-p{prec}")
    finally:
        a.close(); b.close()
    a, Ya, sa, sta = _batch(ENV_SCAN, scs, M, prec, 3)
    b, Yb, sb, stb = _batch(ENV_THREE, scs, M, prec, 3)
    try:
        assert np.array_equal(T.bits(Ya), T.bits(Yb)) and np.array_equal(T.bits(sa), T.bits(sb))
        assert [(s.iters, s.n_kept, s.status) for s in sta] == [(s.iters, s.n_kept, s.status) for s in stb]
    finally:
        a.close(); b.close()
