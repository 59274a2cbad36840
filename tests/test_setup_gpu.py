"""The set-up stage -- k_prune_pass1 / k_setup / k_prune_scatter, their one-launch form k_prologue, setup_body and chain_link -- against the
exact reference of tests/setup_ref.py: which points are kept, in which order, around which origin and in which precision they are stored,
the sum behind sigma2_0, the chain coordinate, the links and H Y0.

Every case runs ONE registration with the smallest iteration count its route allows (one; none on the split route) and reads the stage's
outputs back through tdlo_debug_read_cloud / tdlo_debug_read_setup.  Per frame (u = 2^-53; every count is from the source, written out where
it is used; no gate comes from what a kernel returned):

  1. kept count: stats.n_kept, keep[0] (the state's N on the split route, with split_begin's init[0] and the E-step sums' N_kept) and the length
     of the cloud read back are equal, and equal the reference's count of pinned kept points plus at most the unpinned ones.
  2. the cloud read back is the reference's sequence: the bits of fl_T(fl64(x_n - ctr)) in (nearest node, original index) order; unpinned
     points are removed from both sequences first (they exist only in the razor-band case).
  3. ctr within (ceil(M / 64) + 6) u mean|y| of the longdouble centroid per coordinate (setup_body: lane l adds the nodes l, l + 64, ... --
     ceil(M / 64) - 1 additions --, wave_sum's six butterfly steps, one division), and the centred nodes equal fl64(y - ctr) -- and
     fl_T(fl64(y - ctr)) in the E-step's node block where no M-step has run (split route) -- exactly.
  4. sum of d2 within (M + 22 + tiles + per) u relative (all terms positive.  One d2: three differences at u each -> 2 u in the squares, a
     product, two additions: 5 u.  M - 1 sequential additions per point; block_sum: six butterfly steps and three additions; one addition
     per tile of the workgroup (tiles = prune_tiles); k_setup: per = ceil(nb / 256) sequential additions per thread, six butterfly steps,
     three additions: 5 + M - 1 + 9 + tiles + per + 9); sigma2_0 = sum / (3 M N): the product is an integer, one division more.
  5. coord: bit-equal to estep_ref.chain_coord when the nodes are grid values; otherwise within (i + 4) u coord_i of the exact running sum
     (a segment: 5 u in the sum of squares -> 2.5 u + the root's u <= 4 u; i - 1 additions at u of the partial sum each).
  6. links within the gates of setup_ref.link_gates (counted there entry by entry) of the longdouble links AT THE GAP THE DEVICE USED,
     h = fl64(coord_i - coord_{i-1}) of the coord read back (held by 5); h = 0 gives exactly Phi = I, Q = 0; row 0 within setup_ref.ROW0_GATE;
     H Y0 within 14 u of its mass (13 products, 12 additions).
Each case names its route: the switch that forces it (TDLO_DIRECT_UPLOAD=0: three kernels), the size limits of the fused prologue with the
fall-back counter at zero, the batch / split / tracker entry point, the route counters of tracking_step."""
import ctypes as C
import os

import numpy as np
import pytest

import estep_ref as R
import setup_ref as S

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = S.U
G26 = 2.0 ** -26
WORST = {}


def note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


# ---- scenes (seeds fixed; every builder returns dict(X, Y0, exact, razor, claim)) ---------------------------------------------------
def _synth(N0, M, cfg, outliers=5):
    from trackdlo_amd import synth
    X, Y0, _ = synth.scene(N0, M, config=cfg, outliers=min(outliers, N0))
    return np.array(X, dtype=np.float64), np.array(Y0, dtype=np.float64)


def _perp(Y0, m, rng):
    M = len(Y0)
    tau = Y0[min(m + 1, M - 1)] - Y0[max(m - 1, 0)]
    v = np.cross(tau, rng.normal(size=3))
    return v / np.linalg.norm(v)


def scene_plain(N0, M, cfg=900, off=None, outliers=5):
    X, Y0 = _synth(N0, M, cfg + M, outliers)
    if off is not None:          # away from the origin, full fp64 mantissas (synth's cloud is fp32 values)
        rng = np.random.default_rng(cfg)
        X = X + np.asarray(off) + rng.uniform(-1e-7, 1e-7, X.shape); Y0 = Y0 + np.asarray(off) + rng.uniform(-1e-7, 1e-7, Y0.shape)
    return dict(X=np.asfortranarray(X), Y0=Y0, exact=False, razor=False, claim=None)


SHELL_REL = [1e-3, 1e-6, 1e-9, 1e-12]


def scene_shell(N0, M, cfg=910, nshell=384, off=None):
    """On top of a synth scene: nshell points at 0.02 .. 0.3 m from a node (perpendicular to the chain there), two thirds of them at
    0.1 (1 +- 1e-3, 1e-6, 1e-9, 1e-12), at indices spread over the whole cloud (every prune workgroup) and over all nodes, both ends included."""
    sc = scene_plain(N0, M, cfg, off)
    X, Y0 = sc["X"], sc["Y0"]
    rng = np.random.default_rng(cfg + 1)
    idx = np.unique(np.linspace(0, N0 - 1, nshell).astype(np.int64))
    for j, n in enumerate(idx):
        m = (0, M - 1)[j % 2] if j % 16 < 2 else j % M
        if j % 3 < 2:
            r = 0.1 * (1.0 + (1 if (j // 3) % 2 else -1) * SHELL_REL[(j // 6) % 4])
        else:
            r = (0.02, 0.05, 0.09, 0.11, 0.2, 0.3)[(j // 3) % 6]
        X[n] = Y0[m] + r * _perp(Y0, m, rng)
    return dict(sc, claim="threshold")


def _three_squares_near(n, want, step):
    """Representations n' = a^2 + b^2 + c^2 with c close to sqrt(n') and a, b small (the point then sits almost straight above its node),
    for n' = n, n + step, n + 2 step ... until `want` are found.  Returns [(n', a, b, c)]."""
    from math import isqrt
    out = []
    while len(out) < want:
        c0 = isqrt(n)
        for c in range(c0, c0 - 6, -1):
            r = n - c * c
            a = isqrt(r)
            while a >= 0 and 2 * a * a >= r:
                b2 = r - a * a
                b = isqrt(b2)
                if b * b == b2:
                    out.append((n, a, b, c)); break
                a -= 1
            if out and out[-1][0] == n:
                break
        n += step
    return out


N_KEPT_MAX = 45035996273704          # d2 = n 2^-52 on the 2^-26 m grid: the largest n with sqrt(n 2^-52) < 0.1 ...
N_PRUNED_MIN = 45035996273705        # ... and the smallest one that is pruned (tests/test_setup_ref.py checks both against setup_ref.T_KEEP)


def scene_grid(M, cfg=920):
    """Nodes and points on the 2^-26 m grid inside +-0.25 m: every difference (< 2^25 steps), square (< 2^50) and sum of three (< 2^53) in a
    d2 is an integer that fp64 holds exactly, fused or not.  A zigzag chain with 2^20 steps (1.6 cm) between nodes; points exactly
    equidistant from nodes (a, a + 1) for every a and from (a, a + 1, a + 2) for every a; points whose d2 to their node are integers either side
    of the threshold; ordinary points; pruned points 0.125 m above the chain."""
    assert M <= 14
    rng = np.random.default_rng(cfg + M)
    Sg = 1 << 20
    x0 = -((M - 1) * Sg) // 2
    Yi = np.array([[x0 + m * Sg, (m % 2) * Sg, 0] for m in range(M)], dtype=np.int64)
    pts = []
    for a in range(M - 1):                                   # two-node ties: d2 = 10/16 S^2 (+ z^2) from a and a + 1, 26/16 S^2 or more from the others
        pa = a % 2
        for j in range(6):
            pts.append(Yi[a] + np.array([Sg // 4, (3 * Sg // 4) if pa == 0 else -(3 * Sg // 4), (j - 3) * 1024 + a]))
    for a in range(M - 2):                                   # three-node ties: the circumcentre of a zigzag triangle, d2 = S^2 (+ z^2) from all three
        pa = a % 2
        for j in range(4):
            pts.append(Yi[a] + np.array([Sg, 0, (j - 2) * 2048 + a]))
    ties = len(pts)
    kept_reps = _three_squares_near(N_KEPT_MAX, 6, -1); prun_reps = _three_squares_near(N_PRUNED_MIN, 6, 1)
    edge = []
    for reps in (kept_reps, prun_reps):
        for j, (n, a, b, c) in enumerate(reps):
            for k, (sa, sb, sc_) in enumerate(((1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, 1))):
                m = (j * 4 + k) % M
                edge.append(Yi[m] + np.array([sa * a, sb * b, sc_ * c]))
    pts += edge
    n_rand = 1500
    m = rng.integers(0, M, n_rand)
    pts += list(Yi[m] + rng.integers(-(1 << 19), 1 << 19, (n_rand, 3)))
    pts += list(Yi[rng.integers(0, M, 300)] + np.array([0, 0, 1 << 23]) + rng.integers(-(1 << 19), 1 << 19, (300, 3)))      # 0.125 m away: pruned
    P = np.array(pts, dtype=np.int64)
    P = P[rng.permutation(len(P))]
    assert np.abs(P).max() < (1 << 24) and np.abs(Yi).max() < (1 << 24)
    return dict(X=np.asfortranarray(P.astype(np.float64) * G26), Y0=Yi.astype(np.float64) * G26, exact=True, razor=False, claim="grid",
                n_ties=ties, edge_n=([r[0] for r in kept_reps], [r[0] for r in prun_reps]))


def scene_razor(N0=6000, M=45, cfg=930, n_thr=24, n_tie=24):
    """Points moved, one ulp of one coordinate at a time, until the longdouble margin to the threshold (n_thr of them) or to a tie between two
    consecutive nodes (n_tie) is below 8 u: the unpinned ones."""
    sc = scene_plain(N0, M, cfg)
    X, Y0 = sc["X"], sc["Y0"]
    rng = np.random.default_rng(cfg + 2)
    tL = LD(S.T_KEEP)
    idx = np.linspace(10, N0 - 10, n_thr + n_tie).astype(np.int64)
    made = 0
    for j, n in enumerate(idx):
        for attempt in range(40):
            m = int(rng.integers(3, M - 3))
            if j < n_thr:
                v = _perp(Y0, m, rng)
                p = Y0[m] + 0.1 * v
                k = int(np.argmin(np.abs(Y0[m] - p) + (np.abs(Y0[m] - p) < 1e-4)))       # the coordinate with the smallest (not tiny) difference: the finest steps
                for _ in range(6):
                    d = (Y0[m] - p).astype(LD)
                    miss = tL - (d * d).sum()
                    stp = LD(2) * d[k] * LD(np.spacing(p[k]))
                    p[k] -= float(np.round(miss / stp)) * np.spacing(p[k])
                ok = abs(float(((Y0[m] - p).astype(LD) ** 2).sum() / tL - 1)) < S.PIN / 2
            else:
                v = _perp(Y0, m, rng)
                p = 0.5 * (Y0[m] + Y0[m + 1]) + 0.09 * v
                w = Y0[m + 1] - Y0[m]
                k = int(np.argmin(np.abs(w) + (np.abs(w) < 1e-4)))
                for _ in range(6):
                    da = ((Y0[m] - p).astype(LD) ** 2).sum(); db = ((Y0[m + 1] - p).astype(LD) ** 2).sum()
                    # d(da - db)/dp_k = -2 (y_a - p)_k + 2 (y_b - p)_k = 2 w_k
                    stp = LD(2) * LD(w[k]) * LD(np.spacing(p[k]))
                    p[k] -= float(np.round((da - db) / stp)) * np.spacing(p[k])
                da = ((Y0[m] - p).astype(LD) ** 2).sum(); db = ((Y0[m + 1] - p).astype(LD) ** 2).sum()
                ok = abs(float((da - db) / max(da, db))) < S.PIN / 2 and float(max(da, db)) < 0.0095
            if ok:
                X[n] = p; made += 1
                break
    return dict(sc, razor=True, claim="razor", made=made)


def scene_runs(kind, N0=3000, M=50, cfg=940):
    sc = scene_plain(N0, M, cfg)
    X, Y0 = sc["X"], sc["Y0"]
    rng = np.random.default_rng(cfg + 3)
    if kind == "node0":                 # every point nearest to node 0: output order = input order
        X[:] = Y0[0] + rng.normal(0, 0.002, X.shape)
    elif kind == "even":                # half the nodes without any point
        X[:] = Y0[2 * rng.integers(0, M // 2, N0)] + rng.normal(0, 0.001, X.shape)
    elif kind == "blocks":              # whole prune workgroups whose points are all pruned (the first, one inside, the last)
        for b in (0, 5, (N0 - 1) // 256):
            X[256 * b:256 * (b + 1)] += (0.0, 0.0, 5.0)
    elif kind == "empty":
        X[:] += (0.0, 0.0, 5.0)
    elif kind == "nonfinite":           # NaN, +-inf and 1e200 coordinates between good points
        bad = [np.nan, np.inf, -np.inf, 1e200, -1e200]
        for j, n in enumerate(range(3, N0, 7)):
            X[n, j % 3] = bad[j % 5]
    return dict(sc, X=np.asfortranarray(X))


# ---- the reference of a scene (cached) ------------------------------------------------------------------------------------------
_REF = {}


def sum_d2_centred(X, Y0):
    """sum over points and nodes of |x - y|^2 = M sum|x'|^2 - 2 sum x' . sum y' + N sum|y'|^2 around the nodes' centroid, in longdouble: O(N + M).
    Around the centroid the three terms are within a factor ~10 of the result (cancellation of three bits out of longdouble's 64);
    tests/test_setup_ref.py holds it to 2^-58 of estep_ref.sum_d2 on the small scenes."""
    Xl = np.asarray(X, dtype=np.float64).astype(LD); Yl = np.asarray(Y0, dtype=np.float64).astype(LD)
    c = Yl.sum(axis=0) / LD(len(Yl))
    Xl = Xl - c; Yl = Yl - c
    return LD(len(Yl)) * (Xl * Xl).sum() - LD(2) * (Xl.sum(axis=0) * Yl.sum(axis=0)).sum() + LD(len(Xl)) * (Yl * Yl).sum()


def reference(sc, key=None):
    if key is not None and key in _REF:
        return _REF[key]
    X, Y0 = sc["X"], sc["Y0"]
    M = len(Y0)
    d = S.decide(X, Y0, exact=sc["exact"])
    kp = d["kept"] & d["pinned"]
    order, starts = S.sorted_order(kp, d["nearest"], M)
    n = int(np.count_nonzero(d["kept"]))
    sd = sum_d2_centred(X[d["kept"]], Y0) if n else LD(0)
    r = dict(d=d, order=order, starts=starts, n_kept=n, n_pinned_kept=int(kp.sum()), unpinned=np.nonzero(~d["pinned"])[0], sum_d2=sd,
             sigma2_0=(sd / LD(3 * M * n)) if n else LD(0), ctr=S.centroid(Y0), coord64=R.chain_coord(Y0), coordL=S.chain_exact(Y0))
    if key is not None:
        _REF[key] = r
    return r


def caps(sc, r):
    """The conditions of the scenes, on the reference alone (also run on the CPU by tests/test_setup_ref.py)."""
    d = r["d"]; N0 = len(sc["X"])
    nun = len(r["unpinned"])
    if sc["razor"]:
        assert 16 <= nun <= 64 and nun <= 0.01 * N0, nun
    else:
        assert nun == 0, (nun, "unpinned decisions outside the razor band")
    if sc["claim"] in ("threshold", "grid"):
        rel = np.abs(np.sqrt(d["dmin"]) / 0.1 - 1.0)
        near = np.isfinite(d["dmin"]) & (rel <= 1.001e-3)
        assert int((near & d["kept"]).sum()) >= 16 and int((near & ~d["kept"]).sum()) >= 16, (int((near & d["kept"]).sum()), int((near & ~d["kept"]).sum()))
    if sc["claim"] == "grid":
        assert int(d["ties"].sum()) >= 8 and int(d["ties"].sum()) >= sc["n_ties"]


# ---- driving the library ----------------------------------------------------------------------------------------------------------
def make_ctx(env=None, **kw):
    from trackdlo_amd import binding as B
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = str(v)
        return B.Context(device=0, timing=False, **kw)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def params(prec, max_iter=1, lle=False, beta=None):
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    if lle:
        return B.make_params(P["beta_pre_proc"] if beta is None else beta, P["lambda_pre_proc"], P["lle_weight"], P["mu"], max_iter, 0.0, True, 0.0, 0.0,
                             P["visibility_threshold"], prec)
    return B.make_params(P["beta"] if beta is None else beta, P["lambda_"], P["lle_weight"], P["mu"], max_iter, 0.0, False, 0.0, 0.0, P["visibility_threshold"], prec)


def prune_geometry(N0):
    """prepare_frame: 256-point tiles per prune workgroup (doubling beyond 1024 workgroups) and the workgroups."""
    tiles = 1
    while -(-N0 // (256 * tiles)) > 1024:
        tiles *= 2
    return tiles, -(-N0 // (256 * tiles))


def fused_prologue_serves(N0, M):
    """prologue_pair_ok: at most 64 point workgroups of one tile each and 256 nodes."""
    tiles, nb = prune_geometry(N0)
    return nb <= 64 and tiles == 1 and M <= 256


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def check_frame(ctx, frame, sc, r, prec, label, n_kept_seen=(), split=False, beta=None, pristine_nodes=False, links=True):
    """Assertions 1 - 6 on frame `frame` of the last call."""
    X, Y0 = sc["X"], sc["Y0"]
    N0, M = len(X), len(Y0)
    d = r["d"]
    cloud, ctr = ctx.debug_read_cloud(N0, frame)
    keep = ctx.debug_read_setup("keep", M, frame)
    # 1. the kept count, everywhere the same
    n = len(cloud)
    counts = [int(keep[2])] + ([] if split else [int(keep[0])]) + [int(v) for v in n_kept_seen]
    assert all(c == n for c in counts), (label, n, counts)
    assert r["n_pinned_kept"] <= n <= r["n_pinned_kept"] + len(r["unpinned"]), (label, n, r["n_pinned_kept"], len(r["unpinned"]))
    if not len(r["unpinned"]):
        assert n == r["n_kept"], (label, n, r["n_kept"])
    # 3. the centring offset and the centred nodes
    mean_abs = np.abs(Y0).mean(axis=0)
    g_ctr = (-(-M // 64) + 6) * U * mean_abs
    e_ctr = np.abs((ctr.astype(LD) - r["ctr"]).astype(np.float64))
    assert (e_ctr <= g_ctr).all(), (label, "ctr", e_ctr, g_ctr)
    note("ctr", (e_ctr / np.maximum(g_ctr, 1e-300)).max())
    Yc = ctx.debug_read_setup("Y0", M, frame)
    assert np.array_equal(bits(Yc), bits(S.stored(Y0, ctr, False))), (label, "centred nodes (fp64)")
    nodes = ctx.debug_read_setup("nodes", M, frame)
    if pristine_nodes:
        assert np.array_equal(bits(nodes[:, :3]), bits(S.stored(Y0, ctr, prec == 0))), (label, "node block")
    # 2. the sorted cloud, bit for bit
    ref_seq = S.stored(X[r["order"]], ctr, prec == 0)
    got = cloud
    if len(r["unpinned"]):
        unp = S.stored(X[r["unpinned"]], ctr, prec == 0)
        uset = {row.tobytes() for row in np.ascontiguousarray(unp)}
        assert not any(row.tobytes() in uset for row in np.ascontiguousarray(ref_seq)), (label, "an unpinned point shares its coordinates with a pinned one")
        sel = np.array([row.tobytes() not in uset for row in np.ascontiguousarray(got)], dtype=bool)
        got = got[sel]
    assert got.shape == ref_seq.shape, (label, got.shape, ref_seq.shape)
    same = (bits(got) == bits(ref_seq)).all(axis=1) if len(got) else np.zeros(0, dtype=bool)
    assert same.all(), (label, "sorted cloud: first difference at position", int(np.argmin(same)), "of", len(got), got[int(np.argmin(same))], ref_seq[int(np.argmin(same))])
    # 4. sum of d2 (and sigma2_0 from it)
    tiles, nb = prune_geometry(N0)
    per = -(-nb // 256)
    if n and not len(r["unpinned"]):
        g_sum = (M + 22 + tiles + per) * U
        sd = float(keep[3])
        e = abs(float((LD(sd) - r["sum_d2"]) / r["sum_d2"]))
        assert e <= g_sum, (label, "sum d2", sd, float(r["sum_d2"]), e / g_sum)
        note("sum_d2", e / g_sum)
        if not split:
            assert keep[1] == keep[3], (label, keep)
        s20 = sd / (3.0 * M * n)
        e = abs(float((LD(s20) - r["sigma2_0"]) / r["sigma2_0"]))
        assert e <= g_sum + U, (label, "sigma2_0", e)
    # 5. the chain coordinate
    coord = ctx.debug_read_setup("coord", M, frame)
    if sc["exact"]:
        assert np.array_equal(bits(coord), bits(r["coord64"])), (label, "coord on grid nodes")
    else:
        cl = r["coordL"]
        g_c = (np.arange(M) + 4) * U * cl.astype(np.float64)
        e_c = np.abs((coord.astype(LD) - cl).astype(np.float64))
        assert (e_c <= g_c).all(), (label, "coord", int(np.argmax(e_c - g_c)))
        note("coord", (e_c[1:] / g_c[1:]).max())
    want_w = coord.astype(np.float32).astype(np.float64) if prec == 0 else coord
    assert np.array_equal(bits(nodes[:, 3]), bits(want_w)), (label, "the node block's chain coordinate")
    # 6. the links
    if links:
        check_links(ctx, frame, coord, M, params_beta(beta), label)
    return n


def params_beta(beta):
    from trackdlo_amd import synth
    return synth.LAUNCH_PARAMS["beta"] if beta is None else beta


LINK_NAMES = ["Phi11", "Phi12", "Phi21", "Phi22", "Q11", "Q12", "Q22"]


def check_links(ctx, frame, coord, M, beta, label):
    chain = ctx.debug_read_setup("chain", M, frame)
    r0 = S.row0(beta)
    e0 = np.abs((chain[0, :4].astype(LD) - r0) / r0).astype(np.float64)
    assert (e0 <= S.ROW0_GATE).all() and not chain[0, 4:].any(), (label, "row 0", e0 / S.ROW0_GATE)
    note("row0", (e0 / S.ROW0_GATE).max())
    assert np.isfinite(chain).all(), (label, "a non-finite link")
    for i in range(1, M):
        h = coord[i] - coord[i - 1]
        got = chain[i]
        assert got[7] == 0.0
        if h == 0.0:
            assert list(got[:7]) == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0] and not np.signbit(got[4:7]).any(), (label, i, got)
            continue
        v, g = S.link_gates(h, beta)
        e = np.abs((got[:7].astype(LD) - v).astype(np.float64))
        q = e / g
        assert (q <= 1.0).all(), f"{label}: link {i} (h = {h!r}, x = {np.sqrt(2.0) / beta * h!r}) {LINK_NAMES[int(q.argmax())]} off by {q.max():.3g} gates: {got[:7]!r} against {v.astype(np.float64)!r}"
        for k in range(7):
            note(LINK_NAMES[k], q[k])


def run_single(ctx, sc, prec, label, key=None, **kw):
    r = reference(sc, key)
    caps(sc, r)
    g = ctx.cpd_lle(sc["X"], sc["Y0"], 0.0, params(prec), check=False)
    if r["n_kept"] == 0 and not len(r["unpinned"]):
        from trackdlo_amd import binding as B
        assert g["rc"] == B.TDLO_E_EMPTY and g["n_kept"] == 0, (label, g["rc"])
        cloud, _ = ctx.debug_read_cloud(len(sc["X"]), 0)
        assert len(cloud) == 0
        return g, r
    assert g["rc"] == 0 and g["iters"] == 1, (label, g["rc"], g["iters"])
    check_frame(ctx, 0, sc, r, prec, label, n_kept_seen=[g["n_kept"]], **kw)
    return g, r


@pytest.fixture(scope="module")
def fused():
    """Default switches: clouds of up to 16 384 points and 256 nodes take the fused prologue (k_prologue), larger ones the three kernels."""
    ctx = make_ctx({"TDLO_DIRECT_UPLOAD": None}, max_points=1100000, max_nodes=1024)
    ctx.set_sort_reuse(False)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def classic():
    """TDLO_DIRECT_UPLOAD=0: k_prune_pass1 / k_setup / k_prune_scatter behind a host-to-device copy, whatever the size."""
    ctx = make_ctx({"TDLO_DIRECT_UPLOAD": 0}, max_points=20000, max_nodes=1024)
    ctx.set_sort_reuse(False)
    yield ctx
    ctx.close()


def route_of(ctx_name, N0, M):
    return "k_prologue" if ctx_name == "fused" and fused_prologue_serves(N0, M) else "three kernels"


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
N_ALL = [1, 63, 255, 256, 257, 16384, 16385, 262144, 262145, 524289, 1100000]
M_ALL = [4, 5, 6, 7, 63, 64, 65, 256, 257, 512, 513, 1024]
SHAPES = [(N0, 50) for N0 in N_ALL] + [(N0, M) for M in M_ALL for N0 in (3000, 16385)]


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("N0,M", SHAPES, ids=[f"N{n}-M{m}" for n, m in SHAPES])
def test_shapes(fused, classic, N0, M, prec):
    """Every N0 at M = 50 (the fused prologue's limit, one, two and three doublings of prune_tiles), every M at N0 = 3000 (fused prologue up to 256
    nodes) and 16 385 (three kernels: the scan's four instantiations)."""
    sc = scene_plain(N0, M, 900, outliers=min(7, N0 // 2))
    fb = fused.route_counts()[5]
    run_single(fused, sc, prec, f"shape-N{N0}-M{M}-p{prec}-{route_of('fused', N0, M)}", key=("plain", N0, M))
    assert fused.route_counts()[5] == fb                 # no fall-back from the fused prologue: the route is the one the sizes name
    if N0 <= 20000 and fused_prologue_serves(N0, M):     # the same scene through the three kernels
        run_single(classic, sc, prec, f"shape-N{N0}-M{M}-p{prec}-three kernels", key=("plain", N0, M))


# ---- decisions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("N0,M,off", [(6000, 45, None), (16385, 50, None), (6000, 64, (0.6, -0.3, 0.2)), (300000, 33, None)],
                         ids=["N6000-M45", "N16385-M50", "N6000-M64-offset", "N300000-M33-two-tiles"])
def test_threshold_shell(fused, classic, N0, M, off, prec):
    sc = scene_shell(N0, M, off=off)
    run_single(fused, sc, prec, f"shell-N{N0}-M{M}-p{prec}-{route_of('fused', N0, M)}", key=("shell", N0, M, off))
    if N0 <= 20000:
        run_single(classic, sc, prec, f"shell-N{N0}-M{M}-p{prec}-three kernels", key=("shell", N0, M, off))


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("M", [5, 6, 7, 8, 9, 12])
def test_exact_grid_ties_and_threshold_integers(fused, classic, M, prec):
    """Ties between every pair (a, a + 1) -- (3, 4) across the unrolled loop's group boundary from M = 5 on, the tail m0 + k for M mod 4 = 1, 2, 3 --
    and every triple; the first index wins.  Integer d2 either side of the threshold."""
    sc = scene_grid(M)
    _, r = run_single(fused, sc, prec, f"grid-M{M}-p{prec}-k_prologue", key=("grid", M))
    run_single(classic, sc, prec, f"grid-M{M}-p{prec}-three kernels", key=("grid", M))
    t = r["d"]["ties"]
    assert t.sum() >= sc["n_ties"]


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_razor_band(fused, classic, prec):
    """Unpinned points only: the counts agree with each other and with the cloud, the pinned points are the reference's sequence.  Prints how many
    unpinned threshold points the device kept against the oracle's fp64 formula."""
    sc = scene_razor()
    for name, ctx in (("k_prologue", fused), ("three kernels", classic)):
        g, r = run_single(ctx, sc, prec, f"razor-p{prec}-{name}", key=("razor",))
        d = r["d"]
        un = r["unpinned"]
        thr = un[d["m_thr"][un] <= S.PIN]
        extra = g["n_kept"] - r["n_pinned_kept"] - int((d["m_thr"][un] > S.PIN).sum())
        print(f"razor band ({name}, prec {prec}): {len(un)} unpinned ({len(thr)} at the threshold, {len(un) - len(thr)} at a tie); the oracle's fp64 formula keeps "
              f"{int(d['kept'][thr].sum())} of the threshold points, the device {extra}")


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("off", [(0.6, -0.45, 0.3), (12.0, -7.0, 3.0)], ids=["0.6m", "12m"])
def test_centroid_away_from_the_origin(fused, classic, off, prec):
    for M, N0 in ((45, 5000), (257, 9000)):
        sc = scene_shell(N0, M, cfg=950, off=off)
        run_single(fused, sc, prec, f"offset{off[0]}-M{M}-p{prec}-{route_of('fused', N0, M)}", key=("off", off, M))
        run_single(classic, sc, prec, f"offset{off[0]}-M{M}-p{prec}-three kernels", key=("off", off, M))


# ---- run structure, non-finite points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["node0", "even", "blocks", "nonfinite", "empty"])
def test_run_structure(fused, classic, kind, prec):
    sc = scene_runs(kind)
    for name, ctx in (("k_prologue", fused), ("three kernels", classic)):
        g, r = run_single(ctx, sc, prec, f"runs-{kind}-p{prec}-{name}", key=("runs", kind))
        if kind == "node0":
            assert (r["order"] == np.arange(len(sc["X"]))).all()
        if kind == "even":
            assert (np.diff(r["starts"])[1::2] == 0).all()
        if kind == "nonfinite":
            assert not r["d"]["kept"][~np.isfinite(sc["X"]).all(axis=1) | (np.abs(sc["X"]) > 1e100).any(axis=1)].any()
        if kind == "empty":                                # ... and the context is usable afterwards
            run_single(ctx, scene_runs("blocks"), prec, f"after-empty-p{prec}-{name}", key=("runs", "blocks"))


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_more_nodes_than_points(fused, classic, prec):
    sc = scene_plain(20, 50, 960, outliers=2)
    run_single(fused, sc, prec, f"M>N0-p{prec}-k_prologue")
    run_single(classic, sc, prec, f"M>N0-p{prec}-three kernels")


# ---- the other entry points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_batch_with_ragged_frames(prec):
    """cpd_lle_batch: frames indexed by blockIdx.y with their own nprune_blocks -- 5000, 1 (kept), 700 (all pruned), 16 385, 257 and 9000 points; every
    frame is read back (tdlo_debug_read_cloud / _read_setup by frame of the last call)."""
    from trackdlo_amd import binding as B
    M = 50
    scs = [scene_shell(5000, M, cfg=970), scene_plain(1, M, 971, outliers=0), scene_runs("empty", 700, M, 972), scene_shell(16385, M, cfg=973),
           scene_plain(257, M, 974), scene_runs("nonfinite", 9000, M, 975)]
    F = len(scs)
    ctx = make_ctx(max_frames=F, max_points=16385, max_nodes=64)
    try:
        for f, sc in enumerate(scs):
            ctx.set_cloud(f, sc["X"])
        Yb = np.ascontiguousarray(np.asarray([sc["Y0"] for sc in scs]).transpose(0, 2, 1))
        s2 = np.zeros(F); st = (B.Stats * F)()
        p = params(prec)
        rc = ctx.lib.tdlo_cpd_lle_batch(ctx.h, F, B._ptr(Yb), M, B._ptr(s2), C.byref(p), None, 0, None, 0, None, C.cast(st, C.c_void_p))
        assert rc in (0, B.TDLO_E_EMPTY), rc
        for f, sc in enumerate(scs):
            r = reference(sc)
            caps(sc, r)
            if r["n_kept"] == 0:
                assert st[f].status == B.TDLO_E_EMPTY and st[f].n_kept == 0
                assert len(ctx.debug_read_cloud(len(sc["X"]), f)[0]) == 0
                continue
            assert st[f].status == 0 and st[f].iters == 1, (f, st[f].status)
            check_frame(ctx, f, sc, r, prec, f"batch-frame{f}-p{prec}", n_kept_seen=[st[f].n_kept])
        with pytest.raises(B.TdloError):
            ctx.debug_read_cloud(10, F)                    # beyond the last call's frames
        with pytest.raises(B.TdloError):
            ctx.debug_read_setup("coord", M, F)
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("N0,M", [(6000, 45), (16385, 50), (300000, 20), (3000, 513)])
def test_split_route(N0, M, prec):
    """tdlo_split_begin (split_mode: its own three kernels, no iteration has run): init[], the state, the node block before any M-step, the
    iteration-0 sigma2 after tdlo_split_set_global, and the E-step sums' N_kept."""
    from trackdlo_amd import nsplit
    sc = scene_shell(N0, M, cfg=980)
    r = reference(sc)
    caps(sc, r)
    ctx = make_ctx(max_points=N0, max_nodes=max(64, M))
    try:
        sh = nsplit.HipShard(ctx, sc["X"])
        init = sh.begin(sc["Y0"], 0.0, params(prec, max_iter=5), None, None, None)
        try:
            check_frame(ctx, 0, sc, r, prec, f"split-N{N0}-M{M}-p{prec}", n_kept_seen=[init[0]], split=True, pristine_nodes=True)
            keep = ctx.debug_read_setup("keep", M, 0)
            assert init[1] == keep[3]
            sh.set_global(init[0], init[1])
            s2 = ctx.debug_read_setup("sigma2", M, 0)
            tiles, nb = prune_geometry(N0)
            g = (M + 22 + tiles + -(-nb // 256) + 1) * U
            e = abs(float((LD(s2) - r["sigma2_0"]) / r["sigma2_0"]))
            assert e <= g, ("sigma2_0", s2, float(r["sigma2_0"]), e / g)
            note("sigma2_0", e / g)
            sums = sh.estep(None)
            assert sums[4 * M + 1] == r["n_kept"]
        finally:
            sh.abort()
    finally:
        ctx.close()


def _tracker(ctx, M, Y0, prec):
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 1, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    trk = B.trackdlo(*args, ctx=ctx, precision=B.PREC_F64 if prec else B.PREC_F32)
    trk.initialize_nodes(Y0); trk.initialize_geodesic_coord(synth.geodesic_coord(Y0))
    return trk


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("hidden", [False, True], ids=["all-visible-paired", "hidden-nodes"])
def test_tracking_step(prec, hidden):
    """tracking_step (max_iter 1): with every node visible the cloud is read from pinned host memory by the fused prologue and the main registration's
    set-up rides in the pre-processing registration's launch (route counter 0); with hidden nodes the main registration has a prologue of its own.
    The last call's frame is the MAIN registration: its cloud, offset, nodes, coordinate and links (beta of the main registration) are held."""
    M, N0 = 45, 5000
    sc = scene_shell(N0, M, cfg=990)
    r = reference(sc)
    caps(sc, r)
    ctx = make_ctx(max_points=N0, max_nodes=64)
    try:
        trk = _tracker(ctx, M, sc["Y0"], prec)
        vis = np.arange(M, dtype=np.int32) if not hidden else np.r_[0:18, 27:M].astype(np.int32)
        before = ctx.route_counts()
        trk.tracking_step(sc["X"], vis, vis, None, 0, 0)
        after = ctx.route_counts()
        if not hidden:
            assert after[0] == before[0] + 1, (before, after)           # the paired set-up was taken up
        else:
            assert after[0] == before[0], (before, after)
        st = trk.last_stats
        assert all(s["status"] == 0 for s in st), st
        check_frame(ctx, 0, sc, r, prec, f"tracking_step-{'hidden' if hidden else 'paired'}-p{prec}", n_kept_seen=[s["n_kept"] for s in (st[1:] if hidden else st)])      # (hidden nodes: the pre-processing registration runs on the visible nodes only)
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
def test_cloud_born_on_the_device(prec):
    """tdlo_depth_to_cloud leaves the cloud resident in the slot; the registration that follows prunes and sorts it there."""
    from trackdlo_amd import synth
    M = 30
    depth, mask, cam, Y0 = synth.depth_scene(M, config=9, frame=2)
    ctx = make_ctx(max_points=65536, max_nodes=64)
    try:
        X, n, _ = ctx.depth_to_cloud(0, depth, mask, cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.008)
        sc = dict(X=np.asfortranarray(X), Y0=np.array(Y0, dtype=np.float64), exact=False, razor=False, claim=None)
        r = reference(sc)
        caps(sc, r)
        g = ctx.cpd_lle_resident(0, sc["Y0"], 0.0, params(prec))
        assert g["rc"] == 0 and g["iters"] == 1 and n == len(X)
        check_frame(ctx, 0, sc, r, prec, f"depth-cloud-p{prec}", n_kept_seen=[g["n_kept"]])
    finally:
        ctx.close()


# ---- the links ------------------------------------------------------------------------------------------------------------------------------
BETAS = [0.1, 0.35, 5.0]
X_TARGETS = [0.5, 1 - 1e-3, "1-", "1", "1+", 1 + 1e-3, 2.0, 20.0, 720.0, 800.0]


def gap_for(beta, target):
    """A gap h whose x = fl(fl(sqrt2 / beta) h) is the target: '1-' the largest x below 1, '1' exactly 1 if some h gives it (else the smallest
    x >= 1), '1+' the smallest x above 1."""
    s = np.sqrt(2.0) / np.float64(beta)
    if isinstance(target, float):
        return float(np.float64(target) / s)
    h = np.float64(1.0) / s
    cand = [h]
    for _ in range(8):
        cand.append(np.nextafter(cand[-1], 0.0))
    h = np.float64(1.0) / s
    for _ in range(8):
        h = np.nextafter(h, 10.0); cand.append(h)
    cand = sorted(cand); xs = [s * c for c in cand]
    if target == "1-":
        return float(max((c for c, x in zip(cand, xs) if x < 1.0)))
    if target == "1":
        return float(min((c for c, x in zip(cand, xs) if x >= 1.0)))
    return float(min((c for c, x in zip(cand, xs) if x > 1.0)))


def link_chain(beta, first_gap, sweep):
    """A straight chain along x from the origin: the first gap is `first_gap` (sqrt(h h) = h and 0 + h = h: the device's gap is h to the bit), then the
    gaps of `sweep`; a small cloud around node 0."""
    gaps = [first_gap] + list(sweep)
    xs = np.concatenate([[0.0], np.cumsum(gaps)])
    Y0 = np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], axis=1)
    rng = np.random.default_rng(7)
    X = Y0[0] + rng.normal(0, 0.003, (300, 3))
    return dict(X=np.asfortranarray(X), Y0=Y0, exact=False, razor=False, claim=None)


SWEEP = [0.0, 1e-9, 1e-6, 1e-3, 0.02, 0.0, 0.3, 3.0]


@pytest.mark.parametrize("beta", BETAS)
def test_links_over_gaps_and_beta(beta):
    """Split route (set-up only).  x = s h at 0.5, 1 -+ 1e-3, the last x below 1, 1, the first above, 2, 20, 720 (e^-x subnormal) and 800 (e^-x = 0:
    Phi and Q12 go to 0 and Q to Pinf, nothing is NaN) -- prepare_frame accepts every one of these chains; gaps 0 (coincident nodes: Phi = I, Q = 0),
    1e-9, 1e-6, 1e-3 m ... 3 m."""
    from trackdlo_amd import nsplit
    ctx = make_ctx(max_points=1024, max_nodes=64)
    try:
        for tg in X_TARGETS:
            h = gap_for(beta, tg)
            x64 = np.sqrt(2.0) / np.float64(beta) * np.float64(h)
            if tg == "1-": assert x64 < 1.0 and x64 >= 1.0 - 2.0 ** -50
            if tg in ("1", "1+"): assert 1.0 <= x64 <= 1.0 + 2.0 ** -50
            sc = link_chain(beta, h, SWEEP)
            M = len(sc["Y0"])
            sh = nsplit.HipShard(ctx, sc["X"])
            sh.begin(sc["Y0"], 0.0, params(1, max_iter=3, beta=beta), None, None, None)
            try:
                coord = ctx.debug_read_setup("coord", M, 0)
                assert coord[1] == h, (coord[1], h)                  # the device's first gap is h to the bit
                check_links(ctx, 0, coord, M, beta, f"links-beta{beta}-x{tg}")
                chain = ctx.debug_read_setup("chain", M, 0)
                if tg == 800.0:
                    p = S.row0(beta).astype(np.float64)
                    assert list(chain[1, :4]) == [0.0, 0.0, -0.0, 0.0] or not chain[1, :4].any()
                    assert chain[1, 5] == 0.0 and abs(chain[1, 4] / p[0] - 1) <= 8 * U and abs(chain[1, 6] / p[1] - 1) <= 16 * U
            finally:
                sh.abort()
    finally:
        ctx.close()


def lle_H(Y0, shifted):
    from oracle import ref_cpu
    M = len(Y0)
    L = ref_cpu.calc_lle_weights(Y0, 6)
    H = (np.eye(M) - L).T @ (np.eye(M) - L)
    H = 0.5 * (H + H.T)
    far = np.abs(np.subtract.outer(np.arange(M), np.arange(M))) > 6
    H[far] = 0.0
    if shifted:
        H = H + 0.05 * np.eye(M) + 0.01 * (np.eye(M, k=1) + np.eye(M, k=-1))      # rows no longer sum to zero (still banded and symmetric)
    return H


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("M,shifted,dense", [(45, False, False), (45, True, False), (257, True, False), (45, True, True)],
                         ids=["M45-band", "M45-band-shifted", "M257-band-shifted", "M45-dense-shifted"])
def test_hy0_and_links_with_the_lle_term(M, shifted, dense, prec):
    """Registrations with the LLE term: H Y0 from the 13 diagonals (band route, k_mstep_band) or from the banded dense matrix (the dense pivoted
    route), on a scene 0.6 m from the origin whose H rows do not sum to zero; links at beta_pre_proc."""
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    N0 = 4000
    sc = scene_plain(N0, M, 995, off=(0.6, -0.3, 0.2) if shifted else None)
    r = reference(sc)
    H = lle_H(sc["Y0"], shifted)
    ref, mass = S.hy0(S.band_of(H), sc["Y0"])
    ctx = make_ctx(max_points=N0, max_nodes=max(64, M))
    B.mstep_lle_dense(dense)
    try:
        g = ctx.cpd_lle(sc["X"], sc["Y0"], 2e-5, params(prec, lle=True), H=H, check=False)
        name = ctx.profile_iteration(1)[3]
        assert g["rc"] == 0 and g["iters"] == 1
        assert (name == "k_mstep_band") == (not dense), name
        check_frame(ctx, 0, sc, r, prec, f"lle-M{M}-{'dense' if dense else 'band'}-p{prec}", n_kept_seen=[g["n_kept"]], beta=P["beta_pre_proc"])
        got = ctx.debug_read_setup("HY0", M, 0)
        e = np.abs((got.astype(LD) - ref).astype(np.float64)); gt = 14 * U * mass.astype(np.float64)
        assert (e <= gt).all(), ("H Y0", float((e / gt).max()))
        note("HY0", (e / gt).max())
    finally:
        B.mstep_lle_dense(False)
        ctx.close()


def test_zz_report_worst_ratios():
    """Prints the worst observed ratio to its gate per quantity over the whole file (DESIGN.md 4 quotes them)."""
    assert WORST, "runs last in the file: the cases above fill the table"
    for k, v in WORST.items():
        assert v <= 1.0, (k, v)
    print("set-up stage, worst observed error / gate: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def all_scenes():
    """(label, builder) of every scene this file registers: tests/test_setup_ref.py checks their conditions (caps) where no GPU is needed."""
    out = []
    for N0, M in SHAPES:
        out.append((f"plain-N{N0}-M{M}", lambda N0=N0, M=M: scene_plain(N0, M, 900, outliers=min(7, N0 // 2))))
    for N0, M, off in [(6000, 45, None), (16385, 50, None), (6000, 64, (0.6, -0.3, 0.2)), (300000, 33, None)]:
        out.append((f"shell-N{N0}-M{M}", lambda N0=N0, M=M, off=off: scene_shell(N0, M, off=off)))
    for M in (5, 6, 7, 8, 9, 12):
        out.append((f"grid-M{M}", lambda M=M: scene_grid(M)))
    out.append(("razor", scene_razor))
    for off in [(0.6, -0.45, 0.3), (12.0, -7.0, 3.0)]:
        for M, N0 in ((45, 5000), (257, 9000)):
            out.append((f"offset{off[0]}-M{M}", lambda M=M, N0=N0, off=off: scene_shell(N0, M, cfg=950, off=off)))
    for kind in ("node0", "even", "blocks", "nonfinite", "empty"):
        out.append((f"runs-{kind}", lambda kind=kind: scene_runs(kind)))
    out.append(("M>N0", lambda: scene_plain(20, 50, 960, outliers=2)))
    out += [("batch0", lambda: scene_shell(5000, 50, cfg=970)), ("batch1", lambda: scene_plain(1, 50, 971, outliers=0)), ("batch2", lambda: scene_runs("empty", 700, 50, 972)),
            ("batch3", lambda: scene_shell(16385, 50, cfg=973)), ("batch4", lambda: scene_plain(257, 50, 974)), ("batch5", lambda: scene_runs("nonfinite", 9000, 50, 975))]
    for N0, M in [(6000, 45), (16385, 50), (300000, 20), (3000, 513)]:
        out.append((f"split-N{N0}-M{M}", lambda N0=N0, M=M: scene_shell(N0, M, cfg=980)))
    out.append(("tracking", lambda: scene_shell(5000, 45, cfg=990)))
    for M, sh in ((45, False), (45, True), (257, True)):
        out.append((f"lle-M{M}-{sh}", lambda M=M, sh=sh: scene_plain(4000, M, 995, off=(0.6, -0.3, 0.2) if sh else None)))
    return out
