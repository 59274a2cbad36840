"""GPU suite of the batched start: tdlo_reg_batch (k_reg_estep_batch / k_reg_mstep_batch, csrc/tdlo_reg_batch.hip), tdlo_sort_pts_batch (k_sort_pts_batch,
csrc/tdlo_init.hip) and tdlo_tracker_initialize_from_cloud_batch against the single calls -- bit for bit, frame by frame: border cloud sizes in one batch,
every node count at which a path changes, every frame count at which the route changes, a failing frame among good ones, every refusal, clouds born on
the device, the single calls after a batch, the environment switches, and one frame held to reg's own extended-precision gate (tests/reg_ref.py).
The ordering is held to the numpy statement of tests/init_ref.py as tests/test_init_gpu.py holds the single call."""
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
CLOUDS = [(300, 8), (3000, 40)]                       # (points, nodes) of the composed call, as tests/test_init_gpu.py
BORDER = [255, 256, 257, 1, 3000, 70001]              # one point: reg_ref.nan_cloud(); 70 001: beyond 256 workgroups, the grid-stride loop runs
SLOTS = 32


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    return binding


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(device=0, max_frames=SLOTS, max_points=1 << 17, timing=False)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _tracker(B, ctx, M, slot=0, precision=None):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    return B.trackdlo(M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"],
                      P["lambda_pre_proc"], P["lle_weight"], ctx=ctx, slot=slot, precision=B.PREC_F64 if precision is None else precision)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _table(trackers):
    return C.cast((C.c_void_p * len(trackers))(*[t.h if t is not None else None for t in trackers]), C.c_void_p)


def _cloud(N, seed):
    return reg_ref.nan_cloud() if N == 1 else R.rope_cloud(N, seed=seed)


def _counts(ctx):
    return ctx.init_route_counts() + ctx.init_batch_route_counts()


def _state(t):
    return (t.get_tracking_result(), t.get_guide_nodes(), t.get_sigma2())


def _same_state(a, b):
    return _same(a[0], b[0]) and _same(a[1], b[1]) and _same([a[2]], [b[2]])


def _step(trk, X, M, hidden=0):
    """One tracking_step with the last `hidden` nodes hidden (their priors come from the chain coordinate): (nodes, sigma2), or the error's code."""
    v = np.arange(M - hidden, dtype=np.int32); ve = np.arange(M, dtype=np.int32)
    try:
        trk.tracking_step(X, v, ve)
    except Exception as e:          # TdloError: the twin must end the same way
        return ("refused", getattr(e, "code", None))
    return trk.get_tracking_result(), trk.get_sigma2()


def _same_step(a, b):
    if isinstance(a[0], str) or isinstance(b[0], str):
        return a == b
    return _same(a[0], b[0]) and _same([a[1]], [b[1]])


# ---- reg ---------------------------------------------------------------------------------------------------------------------------------------
def test_border_sizes_in_one_batch(ctx):
    """Slots in reversed order, clouds on both sides of a workgroup, one point (NaN centroids from the third iteration on), and a cloud of more than
    256 x 256 points."""
    M, it = 8, 5
    slots = list(range(len(BORDER)))[::-1]
    for s, N in zip(slots, BORDER):
        ctx.set_cloud(s, _cloud(N, seed=N))
    single = [ctx.reg(None, M, MU, it, slot=s) for s in slots]
    before = _counts(ctx)
    Y, s2 = ctx.reg_batch(slots, M, MU, it)
    assert _counts(ctx) == [before[0], before[1], before[2] + len(slots), before[3]]
    for f, (Ys, ss) in enumerate(single):
        assert _same(Y[f], Ys) and _same([s2[f]], [ss]), (f, BORDER[f])
    k = BORDER.index(1)
    assert np.isnan(Y[k]).all() and np.isnan(s2[k])                          # NaN in the same places (bits compared above) ...
    assert all(np.isfinite(Y[f]).all() and np.isfinite(s2[f]) for f in range(len(BORDER)) if f != k)      # ... and nobody else's


@pytest.mark.parametrize("it", [3, 0])
@pytest.mark.parametrize("M", [4, 5, 64, 65, 356, 890])
def test_node_counts(ctx, M, it):
    """5: 3 M is odd, the state blocks are padded to 16 bytes; 64 | 65: the two forms of the ordering are not reg's business, but the partials' rows are
    5 M + 1 doubles; 356: the first M whose E-step asks for more than 64 KB of LDS (hipFuncSetAttribute for the batch kernel); 890: reg's limit."""
    slots = [2, 0, 1]
    for s in slots:
        ctx.set_cloud(s, R.rope_cloud(300 + s, seed=M + s))
    Y, s2 = ctx.reg_batch(slots, M, MU, it)
    for f, s in enumerate(slots):
        Ys, ss = ctx.reg(None, M, MU, it, slot=s)
        assert _same(Y[f], Ys) and _same([s2[f]], [ss]), (M, it, f)
    assert not _same(Y[0], Y[1]) or it == 0                                  # (distinct clouds: distinct frames)


@pytest.mark.parametrize("F", [1, 2, 3, 32])
def test_frame_counts_and_routes(ctx, B, F):
    """Default TDLO_INIT_BATCH_MIN = 1 (profiles/init_batch_ab.txt): every frame count takes the batch launches (counter 36), one frame included; 25 / 26 / 37
    do not move.  (The other route: test_environment_switches_give_the_same_bits.)"""
    M, it = 8, 3
    slots = list(range(F))
    X = [R.rope_cloud(300 + 7 * f, seed=50 + f) for f in range(F)]
    for s in slots:
        ctx.set_cloud(s, X[s])
    single = [ctx.reg(None, M, MU, it, slot=s) for s in slots]
    c0 = _counts(ctx)
    Y, s2 = ctx.reg_batch(slots, M, MU, it)
    assert _counts(ctx) == [c0[0], c0[1], c0[2] + F, c0[3]]
    for f in range(F):
        assert _same(Y[f], single[f][0]) and _same([s2[f]], [single[f][1]]), f
    # the composed call on the same clouds
    twins = [_tracker(B, ctx, M, slot=s) for s in slots]
    ts2 = [t.initialize_from_cloud(None, MU, it) for t in twins]
    trk = [_tracker(B, ctx, M, slot=s) for s in slots]
    c0 = _counts(ctx)
    codes, bs2 = B.initialize_from_cloud_batch(trk, MU, it)
    assert _counts(ctx) == [c0[0], c0[1], c0[2] + F, c0[3]]
    assert codes == [0] * F and _same(bs2, ts2)
    for a, b in zip(trk, twins):
        assert _same_state(_state(a), _state(b))
    # the ordering alone
    Yn = np.stack([single[f][0] for f in range(F)])
    c0 = _counts(ctx)
    Yo, perm, coord, codes = ctx.sort_pts_batch(Yn)
    assert _counts(ctx) == [c0[0], c0[1], c0[2] + F, c0[3]]
    for f in range(F):
        assert codes[f] == 0 and _same(Yo[f], twins[f].get_tracking_result()) and np.array_equal(Yo[f], Yn[f][perm[f]])


def test_one_frame_of_a_batch_inside_regs_own_gate(ctx):
    """The gate tests/test_reg_gpu.py holds tdlo_reg to (the longdouble reference with its propagated bound), on the middle frame of a batch."""
    N, M = CLOUDS[0]
    X = R.rope_cloud(N, seed=N + M)
    for s, Xs in enumerate((R.rope_cloud(2000, seed=1), X, R.rope_cloud(77, seed=2))):
        ctx.set_cloud(s, Xs)
    Y, s2 = ctx.reg_batch([0, 1, 2], M, MU, ITERS)
    qy, qs = reg_ref.ratio(Y[1], float(s2[1]), reg_ref.propagated(X, M, MU, ITERS))
    print(f"ratio to the gate: Y {qy:.3g}, sigma2 {qs:.3g}")
    assert qy <= 1.0 and qs <= 1.0, (qy, qs)


# ---- the ordering ------------------------------------------------------------------------------------------------------------------------------
_GROUPS = {}


def _groups():
    """The scenes of init_ref.scenes() by node count, each group with one more set of its own -- its first scene's rows rolled by one -- so that every
    group is a batch of at least two DIFFERENT frames: M -> [(nodes, statement)]."""
    if not _GROUPS:
        for name, Y in R.scenes().items():
            _GROUPS.setdefault(len(Y), []).append((Y, R.ref(name)))
        for M, g in _GROUPS.items():
            Yr = np.ascontiguousarray(np.roll(g[0][0], -1, axis=0))
            st = R.statement(Yr)
            assert st["status"] == 0
            g.append((Yr, st))
    return _GROUPS


@pytest.mark.parametrize("M", sorted({len(Y) for Y in R.scenes().values()}))
def test_ordering_of_a_batch_equals_the_statement(ctx, M):
    """M <= 64: the one-wave form, M >= 65: the workgroup form, one workgroup per frame (63 | 64 | 65, 256 | 257, 890, 1024 are among the groups)."""
    g = _groups()[M]
    before = _counts(ctx)
    Ys, perm, coord, codes = ctx.sort_pts_batch(np.stack([Y for Y, _ in g]))
    assert _counts(ctx) == [before[0], before[1], before[2] + len(g), before[3]] and codes == [0] * len(g)
    for f, (_, ref) in enumerate(g):
        assert np.array_equal(perm[f], ref["perm"]), f
        assert _same(Ys[f], ref["Y"]) and _same(coord[f], ref["coord"]), f


@pytest.mark.parametrize("name", ["nan", "dup", "big_dup", "tiny", "huge"])
def test_a_refused_node_set_in_the_middle_of_a_batch(ctx, B, name):
    """Its rc_each is TDLO_E_NUMERIC and its outputs keep their canary values; its neighbours are right; the call returns that code and names the frame."""
    bad, st = R.error_inputs()[name]
    M = len(bad)
    rng = np.random.default_rng(M)
    good = [np.ascontiguousarray(rng.standard_normal((M, 3))) for _ in range(2)]
    refs = [R.statement(Y) for Y in good]
    Yin = np.ascontiguousarray(np.stack([good[0], bad, good[1]]).transpose(0, 2, 1))
    Ys = np.full((3, 3, M), 7.0); perm = np.full((3, M), -7, dtype=np.int32); coord = np.full((3, M), 7.0); rcs = np.full(3, -7, dtype=np.int32)
    rc = ctx.lib.tdlo_sort_pts_batch(ctx.h, _p(Yin), 3, M, _p(Ys), _p(perm), _p(coord), _p(rcs))
    msg = ctx.lib.tdlo_last_error(ctx.h).decode()
    assert rc == B.TDLO_E_NUMERIC and rcs.tolist() == [0, B.TDLO_E_NUMERIC, 0]
    assert "frame 1" in msg and ("non-finite", "coincide", "no edge")[st - 1] in msg, msg
    assert (Ys[1] == 7.0).all() and (perm[1] == -7).all() and (coord[1] == 7.0).all()
    for f, ref in ((0, refs[0]), (2, refs[1])):
        assert ref["status"] == 0 and np.array_equal(perm[f], ref["perm"]) and _same(Ys[f].T, ref["Y"]) and _same(coord[f], ref["coord"]), f
    # every output is optional
    assert ctx.lib.tdlo_sort_pts_batch(ctx.h, _p(Yin), 3, M, None, None, None, None) == B.TDLO_E_NUMERIC


# ---- the composed call -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", CLOUDS)
def test_trackers_started_together_are_the_single_calls_trackers(B, N, M):
    """Nodes, guide nodes, reg's sigma2 and the first tracking_steps (every node visible, then the last quarter hidden: the chain coordinate at work)
    against twins started one by one on another context; the trackers' own sigma2 untouched, a coordinate already there replaced."""
    F = 3
    a = B.Context(device=0, max_frames=F, timing=False); b = B.Context(device=0, max_frames=F, timing=False)
    try:
        X = [R.rope_cloud(N + 11 * f, seed=N + M + f) for f in range(F)]
        ta = [_tracker(B, a, M, slot=f) for f in range(F)]; tb = [_tracker(B, b, M, slot=f) for f in range(F)]
        for f in range(F):
            a.set_cloud(f, X[f])
            ta[f].initialize_geodesic_coord(np.arange(3.0))                  # what was there is replaced, not appended to
            ta[f].set_sigma2(0.125)
        codes, s2a = B.initialize_from_cloud_batch(ta, MU, ITERS)
        s2b = [tb[f].initialize_from_cloud(X[f], MU, ITERS) for f in range(F)]
        assert codes == [0] * F and _same(s2a, s2b)
        for f in range(F):
            assert ta[f].get_sigma2() == 0.125 and tb[f].get_sigma2() == 0.0
            assert _same(ta[f].get_tracking_result(), tb[f].get_tracking_result()) and _same(ta[f].get_guide_nodes(), tb[f].get_guide_nodes())
            assert np.isfinite(ta[f].get_tracking_result()).all()
            ta[f].set_sigma2(s2a[f]); tb[f].set_sigma2(s2b[f])
            X2 = np.asfortranarray(X[f] + np.array([0.0, 0.004, 0.0]))
            for Xk, hidden in ((X2, 0), (X[f], M // 4)):
                ra = _step(ta[f], Xk, M, hidden); rb = _step(tb[f], Xk, M, hidden)
                assert _same_step(ra, rb), (f, hidden, ra, rb)
                assert hidden or not isinstance(ra[0], str), ra
        # a second batch on the same trackers REPLACES again
        codes, s2c = B.initialize_from_cloud_batch(ta, MU, ITERS)
        assert codes == [0] * F and _same(s2c, s2a)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("it,word", [(3, "non-finite"), (1, "coincide")])
def test_a_failing_frame_among_good_ones(B, it, word):
    """reg_ref.nan_cloud() with M = 8: NaN centroids after three iterations, coinciding ones after one (tests/test_init_gpu.py proves both on reg_ref's
    restatement).  That tracker equals an untouched twin, the others their single-call twins, the call returns the first non-zero code."""
    M, F = 8, 3
    a = B.Context(device=0, max_frames=F, timing=False); b = B.Context(device=0, max_frames=F, timing=False)
    try:
        X = [R.rope_cloud(300, seed=3), reg_ref.nan_cloud(), R.rope_cloud(400, seed=4)]
        Xr = R.rope_cloud(300, seed=5)
        Y0 = R.statement(b.reg(Xr, M, MU, ITERS)[0])
        ta = [_tracker(B, a, M, slot=f) for f in range(F)]; tb = [_tracker(B, b, M, slot=f) for f in range(F)]
        for t in ta + tb:
            t.initialize_nodes(Y0["Y"]); t.initialize_geodesic_coord(Y0["coord"]); t.set_sigma2(1e-4)
        for f in range(F):
            a.set_cloud(f, X[f])
        s2 = np.full(F, -1.0); rcs = np.full(F, -7, dtype=np.int32)
        c0 = _counts(a)
        rc = a.lib.tdlo_tracker_initialize_from_cloud_batch(_table(ta), F, MU, it, _p(s2), _p(rcs))
        msg = a.lib.tdlo_last_error(a.h).decode()
        assert rc == B.TDLO_E_NUMERIC and rcs.tolist() == [0, B.TDLO_E_NUMERIC, 0]
        assert "frame 1" in msg and word in msg, msg
        assert _counts(a) == [c0[0], c0[1], c0[2] + F, c0[3]]
        assert s2[1] == -1.0 and _same_state(_state(ta[1]), _state(tb[1]))       # untouched, outputs included
        for f in (0, 2):
            sb = tb[f].initialize_from_cloud(X[f], MU, it)
            assert _same([s2[f]], [sb]) and _same_state(_state(ta[f]), _state(tb[f])), f
        # with the binding: codes, and sigma2 NaN for the tracker that was refused
        codes, s2b = B.initialize_from_cloud_batch(ta, MU, it, check=False)
        assert codes == [0, B.TDLO_E_NUMERIC, 0] and np.isnan(s2b[1]) and _same(s2b[[0, 2]], s2[[0, 2]])
        with pytest.raises(B.TdloError):
            B.initialize_from_cloud_batch(ta, MU, it)
        # the untouched tracker steps like its twin, whose context has seen none of this (the step puts its own cloud into the slot: last)
        X2 = np.asfortranarray(Xr + np.array([0.0, 0.004, 0.0]))
        assert _same_step(_step(ta[1], X2, M), _step(tb[1], X2, M))
    finally:
        a.close(); b.close()


def test_every_refusal_leaves_everything_as_it_was(B):
    M, F = 8, 3
    a = B.Context(device=0, max_frames=4, timing=False); other = B.Context(device=0, max_frames=4, timing=False)
    try:
        lib = a.lib
        X = [R.rope_cloud(300 + f, seed=20 + f) for f in range(F)]
        for f in range(F):
            a.set_cloud(f, X[f]); other.set_cloud(f, X[f])                   # (slot 3 of both stays empty)
        Y0 = R.statement(a.reg(None, M, MU, ITERS, slot=0)[0])
        mk = lambda c, m, s: _tracker(B, c, m, slot=s)
        t = [mk(a, M, f) for f in range(F)]
        for x in t:
            x.initialize_nodes(Y0["Y"]); x.initialize_geodesic_coord(Y0["coord"]); x.set_sigma2(1e-4)
        held = [_state(x) for x in t]
        clouds = [a.get_cloud(f) for f in range(F)]
        c0 = _counts(a)
        s2 = np.full(F, -1.0); rcs = np.full(F, -7, dtype=np.int32)
        start = lambda trk, mu=MU, it=ITERS, n=None: lib.tdlo_tracker_initialize_from_cloud_batch(_table(trk), len(trk) if n is None else n, mu, it, _p(s2), _p(rcs))
        refused = [
            (lambda: start(t, n=0), None),
            (lambda: start(t, n=-2), None),
            (lambda: lib.tdlo_tracker_initialize_from_cloud_batch(None, F, MU, ITERS, _p(s2), _p(rcs)), None),
            (lambda: start([t[0], None, t[2]]), "null"),
            (lambda: start([t[0], mk(other, M, 1), t[2]]), "one context"),
            (lambda: start([t[0], t[1], mk(a, M, 1)]), "named twice"),
            (lambda: start([t[0], t[1], mk(a, M, 3)]), "no cloud"),
            (lambda: start([t[0], mk(a, M + 1, 1), t[2]]), "num_of_nodes"),
            (lambda: start([mk(a, 3, f) for f in range(F)]), "at least 4"),
            (lambda: start([mk(a, 891, f) for f in range(F)]), "at most 890"),
            (lambda: start(t, mu=1.0), "bad reg"),
            (lambda: start(t, mu=-0.1), "bad reg"),
            (lambda: start(t, mu=float("nan")), "bad reg"),
            (lambda: start(t, it=-1), "bad reg"),
        ]
        Yb = np.full((F, 3, M), 7.0); sb = np.full(F, 7.0)
        sl = lambda *s: _p(np.array(s, dtype=np.int32))
        regb = lambda slots, n, M_=M, mu=MU, it=ITERS, Y=Yb, s=sb: lib.tdlo_reg_batch(a.h, slots, n, _p(Y) if Y is not None else None, _p(s) if s is not None else None, M_, mu, it)
        refused += [
            (lambda: regb(sl(0, 1, 2), 0), "bad reg"),
            (lambda: regb(None, 3), "bad reg"),
            (lambda: regb(sl(0, 1, 2), 3, Y=None), "bad reg"),
            (lambda: regb(sl(0, 1, 2), 3, s=None), "bad reg"),
            (lambda: regb(sl(0, 1, 2), 3, M_=0), "bad reg"),
            (lambda: regb(sl(0, 1, 2), 3, M_=891), "890"),
            (lambda: regb(sl(0, 1, 2), 3, mu=1.0), "bad reg"),
            (lambda: regb(sl(0, 1, 2), 3, it=-1), "bad reg"),
            (lambda: regb(sl(0, -1, 2), 3), "out of range"),
            (lambda: regb(sl(0, 4, 2), 3), "out of range"),
            (lambda: regb(sl(0, 1, 0), 3), "named twice"),
            (lambda: regb(sl(0, 3, 2), 3), "no cloud"),
        ]
        Yn = np.ascontiguousarray(np.stack([Y0["Y"]] * 2).transpose(0, 2, 1)); Yo = np.full(Yn.shape, 7.0)
        refused += [
            (lambda: lib.tdlo_sort_pts_batch(a.h, _p(Yn), 0, M, _p(Yo), None, None, None), "no node sets"),
            (lambda: lib.tdlo_sort_pts_batch(a.h, None, 2, M, _p(Yo), None, None, None), "no node sets"),
            (lambda: lib.tdlo_sort_pts_batch(a.h, _p(Yn), 2, 1, _p(Yo), None, None, None), "1024"),
            (lambda: lib.tdlo_sort_pts_batch(a.h, _p(Yn), 2, 1025, _p(Yo), None, None, None), "1024"),
        ]
        for k, (call, word) in enumerate(refused):
            assert call() == B.TDLO_E_INVALID, k
            if word is not None:
                assert word in lib.tdlo_last_error(a.h).decode(), (k, word, lib.tdlo_last_error(a.h).decode())
            assert (s2 == -1.0).all() and (rcs == -7).all() and (Yb == 7.0).all() and (sb == 7.0).all() and (Yo == 7.0).all(), k
            assert _counts(a) == c0, k
            assert all(_same_state(_state(x), h) for x, h in zip(t, held)), k
        assert all(_same(a.get_cloud(f), clouds[f]) for f in range(F))
        # a good call on the same context is still right
        codes, bs2 = B.initialize_from_cloud_batch(t, MU, ITERS)
        for f in range(F):
            tw = mk(other, M, f)
            assert codes[f] == 0 and _same([tw.initialize_from_cloud(None, MU, ITERS)], [bs2[f]]) and _same_state(_state(t[f])[:2] + (0.0,), _state(tw))
    finally:
        a.close(); other.close()


def _depth_image(shift):
    """A small constructed frame (tests/test_init_gpu.py's): a sine stripe three pixels thick, 0.55 .. 0.65 m away; `shift` moves it."""
    rows, cols = 48, 64
    depth = np.zeros((rows, cols), dtype=np.uint16); mask = np.zeros((rows, cols), dtype=np.uint8)
    for u in range(2, cols - 2):
        v = int(round(24 + (12 - shift) * np.sin((u + 3 * shift) / 9.0)))
        mask[v - 1:v + 2, u] = 255
        depth[v - 1:v + 2, u] = 600 + 10 * shift + int(round(50 * np.cos(u / 7.0)))
    return dict(depth=depth, mask=mask, cam=(80.0, 80.0, 32.0, 24.0))


def test_clouds_born_on_the_device_become_trackers_together(ctx, B):
    M, F = 8, 3
    n, _, codes = ctx.depth_to_cloud_batch([_depth_image(k) for k in range(F)], [(2, 0, None), (0, 1, None), (1, 2, None)], 0.008)
    assert codes == [0] * F and min(n) > 60
    slots = [2, 0, 1]
    assert len({ctx.get_cloud(s).tobytes() for s in slots}) == F            # three different clouds, where the kernels left them
    trk = [_tracker(B, ctx, M, slot=s) for s in slots]
    codes, s2 = B.initialize_from_cloud_batch(trk, MU, ITERS)
    assert codes == [0] * F
    for f, s in enumerate(slots):
        tw = _tracker(B, ctx, M, slot=s)
        assert _same([tw.initialize_from_cloud(None, MU, ITERS)], [s2[f]]) and _same_state(_state(trk[f]), _state(tw)), f


def test_single_calls_after_a_batch_give_their_earlier_bits(B):
    """The batch grows and re-carves the workspace the single calls share: they must not notice.  Counters 25 / 26 move for them only."""
    N, M = CLOUDS[1]
    c = B.Context(device=0, max_frames=3, timing=False)
    try:
        X = R.rope_cloud(N, seed=N + M)
        Yn = R.scenes()["rope257"]
        def singles():
            Yr, s2 = c.reg(X, M, MU, ITERS)
            So = c.sort_pts(Yn)
            t = _tracker(B, c, M)
            return Yr, s2, So, t.initialize_from_cloud(None, MU, ITERS), t.get_tracking_result()
        first = singles()
        c1 = _counts(c)
        assert c1[:2] == [2, 0] and c1[2:] == [0, 0]
        for s in range(3):
            c.set_cloud(s, R.rope_cloud(5000 + s, seed=s))
        c.reg_batch([0, 1, 2], 356, MU, 1)                                   # (more than 64 KB of LDS, a larger workspace)
        c.sort_pts_batch(np.stack([R.scenes()["rope1024"]] * 2))
        trk = [_tracker(B, c, M, slot=s) for s in range(3)]
        B.initialize_from_cloud_batch(trk, MU, 2)
        assert _counts(c) == [c1[0], c1[1], 3 + 2 + 3, 0]
        again = singles()
        assert _same(again[0], first[0]) and _same([again[1]], [first[1]]) and _same([again[3]], [first[3]]) and _same(again[4], first[4])
        assert np.array_equal(again[2][1], first[2][1]) and _same(again[2][0], first[2][0]) and _same(again[2][2], first[2][2])
        assert _counts(c) == [c1[0] + 2, c1[1], 8, 0]
    finally:
        c.close()


_ENV_CHILD = textwrap.dedent("""
    import os, sys
    sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
    import numpy as np
    import init_ref as R
    import test_init_batch_gpu as T
    from trackdlo_amd import binding as B
    N, M = T.CLOUDS[0]
    ctx = B.Context(device=0, max_frames=3, timing=False)
    X = [R.rope_cloud(N + f, seed=N + M + f) for f in range(3)] + [T.reg_ref.nan_cloud()]
    out = {}
    for tag, clouds in (("good", X[:3]), ("bad", [X[0], X[3], X[2]])):
        for s, x in enumerate(clouds):
            ctx.set_cloud(s, x)
        trk = [T._tracker(B, ctx, M, slot=s) for s in range(3)]
        codes, s2 = B.initialize_from_cloud_batch(trk, T.MU, 3 if tag == "bad" else T.ITERS, check=False)
        out[tag + "_codes"] = np.array(codes); out[tag + "_s2"] = s2
        out[tag + "_Y"] = np.stack([t.get_tracking_result() for t in trk])
        if tag == "good":
            out["reg_Y"], out["reg_s2"] = ctx.reg_batch([0, 1, 2], M, T.MU, 3)
    out["routes"] = np.array(T._counts(ctx))
    np.savez(sys.argv[2], **out)
    print("OK")
""")


@pytest.mark.parametrize("env,routes", [(dict(TDLO_INIT_BATCH_MIN="4"), [6, 0, 0, 9]), (dict(TDLO_INIT_SORT="host"), [0, 0, 9, 0])])
def test_environment_switches_give_the_same_bits(ctx, B, tmp_path, env, routes):
    """Both are read when the context is made: a fresh child process each.  TDLO_INIT_BATCH_MIN=4: three frames go to the single calls (37; 25 counts their
    six orderings); TDLO_INIT_SORT=host: the three centroid sets are read back once and ordered by the host twin -- the batch's frames (36), no single call."""
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", _ENV_CHILD, ROOT, out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    z = np.load(out)
    N, M = CLOUDS[0]
    assert z["routes"].tolist() == routes
    X = [R.rope_cloud(N + f, seed=N + M + f) for f in range(3)]
    assert z["good_codes"].tolist() == [0, 0, 0] and z["bad_codes"].tolist() == [0, B.TDLO_E_NUMERIC, 0]
    assert np.isnan(z["bad_s2"][1]) and not z["bad_Y"][1].any()             # the refused tracker keeps the zeros it was made with
    for f in range(3):
        ctx.set_cloud(f, X[f])
    trk = [_tracker(B, ctx, M, slot=f) for f in range(3)]
    codes, s2 = B.initialize_from_cloud_batch(trk, MU, ITERS)
    assert _same(z["good_s2"], s2)
    for f in range(3):
        assert _same(z["good_Y"][f], trk[f].get_tracking_result()), f
    Yr, s2r = ctx.reg_batch([0, 1, 2], M, MU, 3)
    assert _same(z["reg_Y"], Yr) and _same(z["reg_s2"], s2r)
    for f in (0, 2):
        tw = _tracker(B, ctx, M, slot=f)
        assert _same([tw.initialize_from_cloud(None, MU, 3)], [z["bad_s2"][f]]) and _same(tw.get_tracking_result(), z["bad_Y"][f]), f
