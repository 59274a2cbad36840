"""tdlo_visibility_prepass_batch (k_node_min_dist_batch: F slots in one launch) against the exact reference of tests/prepass_ref.py and against
tdlo_visibility_prepass on the same slot: node_dist bit for bit (uint64 views), the index sets exactly, and which route ran (tdlo_debug_route_count 30 / 31).

Every frame of a batch is a scene of its own (another seed), and every frame of three or more points also carries, at its first and last index, the
witness points of its two neighbouring frames moved 0.1 mm towards those frames' nodes: a kernel that reads a neighbour's table entry or stages a
neighbour's nodes returns a smaller minimum for some node.  The reference is computed on the clouds as built."""
import ctypes as C

import numpy as np
import pytest

import prepass_ref as R
from test_prepass_gpu import check, make_ctx

pytestmark = pytest.mark.gpu
NMAX = R.TRIP + 512
SIZES = [1, 37, 64, 65, 256, 257, 30000]          # prepass_ref.SMALL_N
NODES = [1, 2, 45, 64, 65, 300]                   # prepass_ref.SMALL_M without 1024
E_INVALID = -2


@pytest.fixture(scope="module")
def ctx8():
    ctx = make_ctx({"TDLO_DIRECT_UPLOAD": None}, max_frames=8, max_points=NMAX, max_nodes=1024)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def copy_ctx8():
    ctx = make_ctx({"TDLO_DIRECT_UPLOAD": 0}, max_frames=8, max_points=NMAX, max_nodes=1024)
    yield ctx
    ctx.close()


_BUILT = {}


def moved_witness(N, M):
    """Which witness (= which node) of a frame its neighbours carry a moved copy of: the one at index N - 2, which no neighbour's point overwrites -- the
    first one for chains too short to have a node there."""
    idx = R.index_list(N)
    k = idx.index(N - 2) if N - 2 in idx else 0
    return k if k < M else 0


def build(sizes, M, seed0=0, far=False):
    """F scenes (frame i: prepass_ref.scene(sizes[i], M, seed0 + i)) with the neighbours' moved witnesses written in, and the reference squared minima
    of every frame on its cloud as built; computed once per process."""
    key = (tuple(sizes), M, seed0, far)
    if key in _BUILT:
        return _BUILT[key]
    F = len(sizes)
    sc = [R.scene(N, M, seed0 + i, far_nodes=tuple(range(M)) if far else ()) for i, N in enumerate(sizes)]
    Xs = [np.array(s[0], order="F") for s in sc]
    if F > 1:
        for i in range(F):
            if sizes[i] < 3:
                continue
            for where, j in ((0, (i - 1) % F), (sizes[i] - 1, (i + 1) % F)):
                k = moved_witness(sizes[j], M)
                W = np.asarray(sc[j][0])[sc[j][3][k]]               # a witness of neighbour j ...
                y = np.asarray(sc[j][1])[k]                         # ... and the node gathered around it (node m lies at witness m mod K)
                Xs[i][where] = W + 1e-4 * (y - W) / np.linalg.norm(y - W)
    Ys = [np.asarray(s[1]) for s in sc]
    coords = [s[2] for s in sc]
    d2 = [R.min_d2(Xs[i], Ys[i])[0] for i in range(F)]
    _BUILT[key] = (Xs, Ys, coords, d2)
    return _BUILT[key]


def run_batch(ctx, slots, Xs, Ys, coords, d2, thr, d_vis, label, route=0, resident=False):
    """One batch call, held to the reference and to the single call on every slot; asserts counters 30 / 31."""
    F = len(slots)
    if not resident:
        for s, X in zip(slots, Xs):
            ctx.set_cloud(s, X)
    before = ctx.prepass_batch_route_counts(); single = ctx.prepass_route_counts()
    dist, vis, ext = ctx.visibility_prepass_batch(slots, np.stack(Ys), thr, d_vis, np.stack(coords))
    after = ctx.prepass_batch_route_counts()
    if F == 1 and route == 0:        # one slot is passed on to the single call, which takes its own one-launch kernel
        assert [a - b for a, b in zip(after, before)] == [0, 1], (label, before, after)
        assert [a - b for a, b in zip(ctx.prepass_route_counts(), single)] == [1, 0], label
    else:
        assert [a - b for a, b in zip(after, before)] == [1 - route, route], (label, before, after)
        assert [a - b for a, b in zip(ctx.prepass_route_counts(), single)] == [0, route * F], label      # (passed on: the copy route of every single call)
    for i in range(F):
        want = R.threshold_and_fill(d2[i], thr, d_vis, coords[i])
        check((dist[i], vis[i], ext[i]), want, f"{label}: frame {i} (slot {slots[i]}) against the reference")
        check(ctx.visibility_prepass(slots[i], Ys[i], thr, d_vis, coords[i]), want, f"{label}: frame {i}, the single call")
    return dist, vis, ext


def median_thr(d2):
    r = np.sqrt(np.concatenate(d2))
    return float(np.median(r[np.isfinite(r)]))


@pytest.mark.parametrize("M", NODES)
def test_mixed_sizes(ctx8, M):
    """N = 1 .. 30000 in one call: wave and workgroup borders, ragged last waves, one node tile and several; then the first one, two, three of them."""
    Xs, Ys, coords, d2 = build(SIZES, M)
    thr = median_thr(d2)
    run_batch(ctx8, list(range(7)), Xs, Ys, coords, d2, thr, 0.06, f"M{M}-F7")
    for F in (1, 2, 3):
        Xf, Yf, cf, df = build(SIZES[:F], M)
        run_batch(ctx8, list(range(F)), Xf, Yf, cf, df, thr, 0.06, f"M{M}-F{F}")


def test_passed_on_where_the_single_call_takes_the_copies(copy_ctx8):
    """TDLO_DIRECT_UPLOAD=0: the call loops over tdlo_visibility_prepass (counter 31), the same bits."""
    Xs, Ys, coords, d2 = build(SIZES, 45)
    run_batch(copy_ctx8, list(range(7)), Xs, Ys, coords, d2, median_thr(d2), 0.06, "copies", route=1)


def test_second_trip_inside_a_batch(ctx8):
    """A frame of TRIP + 321 points between two frames of one point: the grid-stride loop's second trip happens in a frame's own workgroup range."""
    Xs, Ys, coords, d2 = build([1, R.TRIP + 321, 1], 8)
    run_batch(ctx8, [0, 1, 2], Xs, Ys, coords, d2, median_thr(d2[1:2]), 0.06, "second trip")


def test_slots_out_of_order(ctx8):
    Xs, Ys, coords, d2 = build([257, 65, 30000], 45, seed0=3)
    run_batch(ctx8, [5, 0, 3], Xs, Ys, coords, d2, median_thr(d2), 0.06, "slots 5, 0, 3")


def test_neighbours_witnesses_decide_nothing(ctx8):
    """Frames of one size and node count that differ only in their seed: the moved witnesses of the neighbours lie in every cloud, and every row is its own
    frame's.  (The moved witness IS closer to its node than that node's own witness: a mix-up would show.)"""
    sizes = [257] * 5
    Xs, Ys, coords, d2 = build(sizes, 45, seed0=20)
    for i in range(5):
        for j in ((i - 1) % 5, (i + 1) % 5):
            k = moved_witness(257, 45)
            own = float(((Ys[j][k] - Xs[j][R.index_list(257)[k]]) ** 2).sum())
            assert R.min_d2(Xs[i], Ys[j][k:k + 1])[0][0] < own, "the construction: frame i's cloud holds a point closer to a node of neighbour j than that node's own witness"
    run_batch(ctx8, [0, 1, 2, 3, 4], Xs, Ys, coords, d2, median_thr(d2), 0.06, "witnesses")


def test_rearmed_between_calls_of_different_shape():
    """32 x 300 (near witnesses), 2 x 45 (every node more than 4 cm away), 32 x 300 again, the single call, a ride in the cloud kernel: stale minima or a stale
    ticket of any of them would show in the next."""
    from trackdlo_amd import synth
    ctx = make_ctx({"TDLO_DIRECT_UPLOAD": None}, max_frames=32, max_points=1 << 16, max_nodes=1024)
    try:
        big = build([257] * 32, 300, seed0=40)
        small = build([257, 64], 45, seed0=80, far=True)
        assert np.sqrt(np.concatenate(small[3])).min() > 0.04 and np.sqrt(np.concatenate(big[3])).min() <= 0.02
        for k, (b, F) in enumerate(((big, 32), (small, 2), (big, 32))):
            Xs, Ys, coords, d2 = b
            run_batch(ctx, list(range(F)), Xs, Ys, coords, d2, 0.0655, 0.06, f"call {k}")
        X, Y, coord, idx, r, (d2s, _) = R.case_ref(30000, 300)
        ctx.set_cloud(0, X)
        check(ctx.visibility_prepass(0, Y, 0.0655, 0.06, coord), R.threshold_and_fill(d2s, 0.0655, 0.06, coord), "the single call behind the batches")
        depth, mask, cam, Y0 = synth.depth_scene(30, config=9, frame=2)
        gc = synth.geodesic_coord(Y0)
        d, m = ctx.image_buffers(*depth.shape)
        d[:] = depth; m[:] = mask
        rides = ctx.cloud_vis_rides()
        dist, vis, ext, n, _ = ctx.depth_to_cloud_visibility(0, d, m, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.008, Y0, 0.008, 0.06, gc)
        assert ctx.cloud_vis_rides() == rides + 1
        check((dist, vis, ext), R.prepass(ctx.get_cloud(0), Y0, 0.008, 0.06, gc), "the ride behind the batches")
        Xs, Ys, coords, d2 = small
        run_batch(ctx, [0, 1], Xs, Ys, coords, d2, 0.0655, 0.06, "a batch behind the ride")
    finally:
        ctx.close()


def test_non_finite_points(ctx8):
    """One frame with NaN / inf points at the index list, one frame without a finite point at all (distance 100000, nothing visible), a clean one between."""
    X, Y, coord, idx, r, (d2, _) = R.case_ref(257, 45, seed=8)
    X2, bad = R.with_non_finite(X)
    Xc, Yc, cc, _, _, (d2c, _) = R.case_ref(256, 45, seed=9)
    Xs = [X2, Xc, X2[bad]]
    Ys = [np.asarray(Y), np.asarray(Yc), np.asarray(Y)]
    coords = [coord, cc, coord]
    d2s = [d2, d2c, np.full(45, np.inf)]
    thr = float(np.median(r))
    dist, vis, ext = run_batch(ctx8, [0, 1, 2], Xs, Ys, coords, d2s, thr, 0.06, "non-finite")
    assert (dist[2] == 100000.0).all() and len(vis[2]) == 0 and len(ext[2]) == 0 and 0 < len(vis[0]) < 45 and len(vis[1]) > 0


def raw_batch(ctx, F, slots, M, Y=None, coord=None):
    sl = np.ascontiguousarray(slots, dtype=np.int32)
    n = max(F, 1) * max(M, 1)
    Y = np.zeros(3 * n) if Y is None else Y
    coord = np.zeros(n) if coord is None else coord
    dist = np.zeros(n); vis = np.zeros(n, dtype=np.int32); ext = np.zeros(n, dtype=np.int32)
    nv = np.zeros(max(F, 1), dtype=np.int32); ne = np.zeros(max(F, 1), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return ctx.lib.tdlo_visibility_prepass_batch(ctx.h, F, p(sl), p(Y), M, 0.01, 0.06, p(coord), p(dist), p(vis), p(nv), p(ext), p(ne))


def test_refusals(ctx8):
    """A duplicate slot, a slot without a cloud, F = 0, F > max_frames, M < 1: TDLO_E_INVALID each, counters untouched, and the next call is right."""
    Xs, Ys, coords, d2 = build([257, 65, 64], 45, seed0=60)
    thr = median_thr(d2)
    run_batch(ctx8, [0, 1, 2], Xs, Ys, coords, d2, thr, 0.06, "before")
    assert len(ctx8.get_cloud(7)) == 0, "slot 7 holds no cloud in this module"
    before = ctx8.prepass_batch_route_counts()
    assert raw_batch(ctx8, 3, [0, 1, 0], 45) == E_INVALID
    assert raw_batch(ctx8, 3, [0, 7, 1], 45) == E_INVALID
    assert raw_batch(ctx8, 0, [0], 45) == E_INVALID
    assert raw_batch(ctx8, 9, list(range(9)), 45) == E_INVALID
    assert raw_batch(ctx8, 3, [0, 1, 2], 0) == E_INVALID
    assert raw_batch(ctx8, 3, [0, 1, 8], 45) == E_INVALID
    assert ctx8.prepass_batch_route_counts() == before
    run_batch(ctx8, [0, 1, 2], Xs, Ys, coords, d2, thr, 0.06, "after the refusals", resident=True)
