"""Depth images with a PRESCRIBED run structure for the one-launch depth -> cloud kernels (k_cloud_team, k_cloud_fused; trackdlo_amd/csrc/tdlo_cloud.hip):
every scene puts the sorted points where one of the kernels' borders lies -- a team member's slice, the staging window, a trip of 1024, a word-layout
limit.  Written from the header's contract and the constants below, not from the kernels; what a scene claims is asserted in
tests/test_cloud_scenes_ref.py on voxel_ref.structure alone, and a CPU test reads the constants out of the kernels' source, so that a retune moves the scenes.

The recipe: a long-lens camera (fx = fy = 1e8, cx = cy = -0.5) makes every x and y a small positive float with a full mantissa inside cell 0; with
leaf = 2 mm a point of depth 2 c + 1 mm lies in the middle of z-cell c.  The masked pixels are a sorted random subset of the allowed pixels and the cells are
dealt to them by a random permutation: a cell's points lie scattered in pixel order, and the stable order decides the float sums.  Mask bytes are drawn from
1 .. 255, unmasked depth is random."""
import functools

import numpy as np

# ---- the kernels' constants (tdlo_cloud.hip; held to its text by test_cloud_scenes_ref.py)
kFNmax, kFT, kFPix, kFTmax, kTK, kTCh, kTVcap = 32704, 1024, 4096, 4095, 8, 64, 6144
CONSTANTS = dict(kFNmax=kFNmax, kFT=kFT, kFPix=kFPix, kFTmax=kFTmax, kTK=kTK, kTCh=kTCh, kTVcap=kTVcap)

LEAF = 0.002
N_FULL = kFNmax


def tiles(P):
    return (P + kFPix - 1) // kFPix


def team_slices(n, T):
    """The slice rule of k_cloud_team: K = min(8, T), per = roundup64(ceil(n / K)), s_k = min(k per, n).  Returns (K, per, [s_0 .. s_K])."""
    K = min(kTK, T)
    per = ((n + K - 1) // K + 63) & ~63
    return K, per, [min(k * per, n) for k in range(K + 1)]


def fused_R(n):
    """The thread rule of k_cloud_fused: thread t takes the sorted positions [t R, t R + R)."""
    return (n + kFT - 1) // kFT


class Scene:
    """depth [rows x cols] uint16, mask [rows x cols] uint8, cam = (fx, fy, cx, cy), leaf; route: what the one-launch kernels do with the frame --
    "taken", "passed" (on to the multi-launch form) or "untouched" (the host does not launch them)."""

    def __init__(self, name, depth, mask, cam, leaf=LEAF, route="taken", runs=None, note=None):
        self.name, self.depth, self.mask, self.cam, self.leaf, self.route, self.runs, self.note = name, depth, mask, cam, leaf, route, runs, note or {}

    @property
    def P(self):
        return self.depth.size

    @property
    def T(self):
        return tiles(self.P)

    def points(self):
        import voxel_ref as V
        return V.backproject(self.depth, self.mask, *self.cam)

    @functools.cached_property
    def ref(self):
        """(X, n_raw) of the reference; computed once, never written to."""
        import voxel_ref as V
        X, n_raw = V.voxel_ref(self.points(), None, self.leaf)
        X.setflags(write=False)
        return X, n_raw

    @functools.cached_property
    def structure(self):
        import voxel_ref as V
        return V.structure(self.points(), None, self.leaf)


def cell_scene(name, rows, cols, runs, seed, *, pixels=None, cell_depth=None, leaf=LEAF, fx=1e8, route="taken", force_pixels=(), note=None):
    """runs[c] masked pixels in the c-th occupied cell (ascending key).  pixels: the pixel numbers a masked pixel may have (default: all);
    force_pixels are masked whatever the draw; cell_depth[c]: the depth in mm of cell c's points (default 2 c + 1: mid-cell at leaf 2 mm)."""
    rng = np.random.default_rng(seed)
    runs = np.asarray(runs, dtype=np.int64)
    n, P = int(runs.sum()), rows * cols
    pool = np.arange(P) if pixels is None else np.asarray(pixels)
    force = np.asarray(sorted(force_pixels), dtype=np.int64)
    free = np.setdiff1d(pool, force)
    pix = np.sort(np.concatenate([force, rng.choice(free, n - len(force), replace=False)]))
    cell = rng.permutation(np.repeat(np.arange(len(runs)), runs))
    cd = 2 * np.arange(len(runs)) + 1 if cell_depth is None else np.asarray(cell_depth)
    assert cd.min() >= 1 and cd.max() <= 65535
    depth = rng.integers(1, 60000, P).astype(np.uint16)
    mask = np.zeros(P, np.uint8)
    depth[pix] = cd[cell].astype(np.uint16)
    mask[pix] = rng.integers(1, 256, n)
    return Scene(name, depth.reshape(rows, cols), mask.reshape(rows, cols), (fx, fx, -0.5, -0.5), leaf, route, runs, note)


def fill_runs(n, solid, seed, lo=1, hi=40):
    """Run lengths that sum to n: the half-open position intervals in `solid` are runs of their own (a head at each start, none inside), the rest is cut
    into runs of lo .. hi points."""
    rng = np.random.default_rng(seed)
    solid = sorted(solid)
    runs, p, i = [], 0, 0
    while p < n:
        if i < len(solid) and p == solid[i][0]:
            runs.append(solid[i][1] - p); p = solid[i][1]; i += 1
            continue
        stop = solid[i][0] if i < len(solid) else n
        L = min(int(rng.integers(lo, hi + 1)), stop - p)
        runs.append(L); p += L
    assert p == n and min(runs) >= 1
    return runs


ROWS, COLS = 192, 256            # 12 tiles: K = 8, room for kFNmax points


def heads_of(runs):
    """Sorted positions at which a run starts."""
    return np.concatenate([[0], np.cumsum(runs)[:-1]]).astype(np.int64)


# ---- A: slice borders -------------------------------------------------------------------------------------------------------------------------
def scene_A():
    _, per, s = team_slices(N_FULL, tiles(ROWS * COLS))
    solid = [(s[1], s[1] + 7), (s[2], s[2] + 1), (s[3], s[3] + 33), (s[4] - 1, s[4] + 1), (s[5] - 1, s[5] + 1), (s[6] - 1, s[6]), (s[6], s[6] + 12),
             (s[7] - 40, s[7] + 25)]
    return cell_scene("A", ROWS, COLS, fill_runs(N_FULL, solid, 101), 102, note=dict(solid=solid))


# ---- B: long runs -----------------------------------------------------------------------------------------------------------------------------
B_SOLID = {"B_ii": [(4000, 11000)], "B_iii": [(8186, 14386)], "B_iv_at": [(4000, kTVcap)], "B_iv_past": [(4000, kTVcap + 1)]}


def scene_B(which):
    if which == "B_i":
        return cell_scene(which, ROWS, COLS, [N_FULL], 110)
    if which == "B_v":
        return cell_scene(which, ROWS, COLS, [100, 9000, 23604], 111)
    solid = B_SOLID[which]
    return cell_scene(which, ROWS, COLS, fill_runs(N_FULL, solid, 112), 113 + sorted(B_SOLID).index(which), note=dict(solid=solid))


# ---- C: sizes ---------------------------------------------------------------------------------------------------------------------------------
C_SIZES = [1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 10901, 10902, 16384, 16385, 31744, 31745, 32703, 32704]


def scene_C(n):
    return cell_scene("C_%d" % n, ROWS, COLS, fill_runs(n, [], 200 + n), 300 + n, route="taken" if n <= kFNmax else "passed")


def scene_C_distinct():
    return cell_scene("C_distinct", ROWS, COLS, [1] * N_FULL, 120)


# ---- D: team size and tiles -------------------------------------------------------------------------------------------------------------------
D_IMAGES = {1: (63, 65), 2: (90, 91), 7: (149, 191), 8: (181, 181), 9: (192, 192)}          # T: rows x cols; P % 4 = 3, 2, 3, 1, 0
D_PLACES = ("first", "last", "alternate")


def scene_D(T, place):
    rows, cols = D_IMAGES[T]
    P = rows * cols
    assert tiles(P) == T
    tile = np.arange(P) // kFPix
    if place == "first":
        pool, force = np.nonzero(tile == 0)[0], ()
    elif place == "last":
        pool, force = np.nonzero(tile == T - 1)[0], (P - 1,)
    else:
        pool, force = np.nonzero(tile % 2 == 0)[0], (P - 1,)
    n = min(3000, len(pool) - 5)
    return cell_scene("D_%d_%s" % (T, place), rows, cols, fill_runs(n, [], 400 + T), 410 + 3 * T + D_PLACES.index(place), pixels=pool, force_pixels=force)


# ---- E: many tiles ----------------------------------------------------------------------------------------------------------------------------
def scene_E(which):
    if which == "E_1026":
        rows, cols, tl, route = 2048, 2051, (0, 1023, 1024, 1025), "taken"
    elif which == "E_max":
        rows, cols, tl, route = kFTmax, kFPix, (0, 1, kFTmax - 1), "taken"
    else:                                                                                    # one pixel more than 4095 tiles hold
        rows, cols, tl, route = 1, kFTmax * kFPix + 1, (0, 1, kFTmax), "untouched"
    P = rows * cols
    pool = np.concatenate([np.arange(t * kFPix, min((t + 1) * kFPix, P)) for t in tl])
    n = min(6000, len(pool) - 1)
    s = cell_scene(which, rows, cols, fill_runs(n, [], 500, lo=100, hi=900), 501 + len(which), pixels=pool, fx=1e10, route=route, note=dict(tiles=tl))
    assert s.T == (kFTmax + 1 if route == "untouched" else tiles(P))
    return s


# ---- F: word layout ---------------------------------------------------------------------------------------------------------------------------
F_CELLS = {1: 2, 4: 16, 5: 17, 8: 256, 9: 257}          # kb: z-cells at leaf 2 mm


def scene_F(kb):
    """kb up to 9: that many z-cells at leaf 2 mm, every one occupied.  kb = 16, 17: leaf 0.5 mm (fx = 1e9), where every depth value is a cell of its own and
    the grid's extent is twice the depth span."""
    n = 20000
    if kb in F_CELLS:
        ncell = F_CELLS[kb]
        cuts = np.sort(np.random.default_rng(600 + kb).choice(np.arange(1, n), ncell - 1, replace=False))
        runs = np.diff(np.concatenate([[0], cuts, [n]]))
        return cell_scene("F_kb%d" % kb, ROWS, COLS, runs, 610 + kb)
    return layout_scene("F_kb%d" % kb, n, {16: 20000, 17: 40000}[kb], 0.0005, 620 + kb)


def layout_scene(name, n, span, leaf, seed, route="taken"):
    """n points in cells of one depth value each, the depth values spread over [1000, 1000 + span] mm with both ends occupied."""
    runs = fill_runs(n, [], seed, lo=1, hi=9)
    rng = np.random.default_rng(seed + 1)
    cd = 1000 + np.sort(np.concatenate([[0, span], rng.choice(np.arange(1, span), len(runs) - 2, replace=False)]))
    return cell_scene(name, ROWS, COLS, runs, seed + 2, cell_depth=cd, leaf=leaf, fx=1e9, route=route)


@functools.lru_cache(maxsize=None)
def scene_F_pair():
    """The first two depth spans (a search on the reference's structure alone) at which rb + kb is 32 (taken) and 33 (passed on); leaf 0.25 mm."""
    found = {}
    for span in range(24000, 64001, 8000):
        for want, route in ((32, "taken"), (33, "passed")):
            if want not in found:
                s = layout_scene("F_rbkb%d" % want, 20000, span, 0.00025, 640, route)
                if s.structure["rb"] + s.structure["kb"] == want:
                    found[want] = s
    return found[32], found[33]


# ---- G: values --------------------------------------------------------------------------------------------------------------------------------
def _wall(seed, rows=480, cols=640):
    from trackdlo_amd import synth
    cam = synth.CAMERA
    assert (cam["rows"], cam["cols"]) == (rows, cols)
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:rows, 0:cols]
    depth = (600.0 + 0.35 * j + 0.2 * i + 3.0 * rng.random((rows, cols))).astype(np.uint16)          # a flat wall, slanted: cells in all three directions
    mask = ((rng.random((rows, cols)) < 0.06) * rng.integers(1, 256, (rows, cols))).astype(np.uint8)
    return depth, mask, (cam["fx"], cam["fy"], cam["cx"], cam["cy"])


def scene_G(which):
    depth, mask, cam = _wall(700)
    if which == "G_wall":
        return Scene(which, depth, mask, cam, 0.02)
    if which == "G_far":                                                                         # the wall at the far end of the depth format: 65 532 .. 65 535
        depth = (65535 - depth % 4).astype(np.uint16)
        return Scene(which, depth, mask, cam, 0.5)
    # masked zero-depth pixels left of and above the principal point only: x = y = -0.0f, z = 0.0f, alone in their cell (the wall is 0.6 m away)
    zero = np.zeros(mask.shape, dtype=bool)
    zero[10:200:7, 5:300:11] = True
    assert zero[:, 320:].sum() == 0 and zero[240:].sum() == 0
    depth[zero] = 0
    mask[zero] = 255
    if which == "G_zero":
        return Scene(which, depth, mask, cam, 0.02, note=dict(zero=zero))
    keep = zero.copy(); keep[300:330, 400:440] = True                                            # ... at a leaf that triggers the pass-through: fewer points
    mask[~keep] = 0
    return Scene("G_zero_pass", depth, mask, cam, 1e-6, route="passed", note=dict(zero=zero))


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------------
def _makers():
    m = {"A": scene_A, "C_distinct": scene_C_distinct}
    for w in ("B_i", "B_ii", "B_iii", "B_iv_at", "B_iv_past", "B_v"):
        m[w] = functools.partial(scene_B, w)
    for n in C_SIZES + [kFNmax + 1]:
        m["C_%d" % n] = functools.partial(scene_C, n)
    for T in D_IMAGES:
        for place in D_PLACES:
            m["D_%d_%s" % (T, place)] = functools.partial(scene_D, T, place)
    for w in ("E_1026", "E_max", "E_over"):
        m[w] = functools.partial(scene_E, w)
    for kb in (1, 4, 5, 8, 9, 16, 17):
        m["F_kb%d" % kb] = functools.partial(scene_F, kb)
    m["F_rbkb32"] = lambda: scene_F_pair()[0]
    m["F_rbkb33"] = lambda: scene_F_pair()[1]
    for w in ("G_wall", "G_far", "G_zero", "G_zero_pass"):
        m[w] = functools.partial(scene_G, w)
    return m


MAKERS = _makers()
NAMES = list(MAKERS)
LARGE = ("E_1026", "E_max", "E_over")          # the only large images


@functools.lru_cache(maxsize=None)
def get(name):
    s = MAKERS[name]()
    s.depth.setflags(write=False); s.mask.setflags(write=False)
    return s


def route_rule(st, T):
    """What the one-launch kernels do with a frame of T tiles whose reference structure is st (the header's rule for the one-launch form)."""
    if T > kFTmax:
        return "untouched"
    if st["n_raw"] == 0:
        return "taken"                                             # (the kernel itself reports an empty cloud)
    return "passed" if st["n_raw"] > kFNmax or st["nodown"] or st["rb"] + st["kb"] > 32 else "taken"


def family(name):
    return name[0]


# ---- a scene as a colour frame ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _colour_pools():
    """BGR colours by where tests/colour_ref.py's HSV of them lies against the launch file's range: inside it, or exactly one unit outside in H (both
    sides), S or V."""
    import colour_ref
    rng = np.random.default_rng(77)
    (lo,), (hi,) = colour_ref.LAUNCH_RANGE
    def blue(n, b):
        b = np.broadcast_to(b, n).astype(np.int64)
        return np.stack([b, (rng.random(n) * (b + 1)).astype(np.int64), (rng.random(n) * (b + 1)).astype(np.int64)], axis=1)
    g = rng.integers(30, 256, 100000)
    green = np.stack([g - rng.integers(0, 6, 100000), g, (rng.random(100000) * g * 0.5).astype(np.int64)], axis=1)      # hue just below the blue side
    cand = np.clip(np.concatenate([blue(300000, rng.integers(30, 256, 300000)), blue(50000, lo[2] - 1), green]), 0, 255).astype(np.uint8)
    hsv = colour_ref.bgr_to_hsv(cand).astype(np.int64)
    inside = ((hsv >= lo) & (hsv <= hi)).all(axis=1)
    pools = {"in": cand[inside]}
    for c, v, tag in ((0, lo[0] - 1, "h_lo"), (0, hi[0] + 1, "h_hi"), (1, lo[1] - 1, "s_lo"), (2, lo[2] - 1, "v_lo")):
        rest = [k for k in range(3) if k != c]
        sel = (hsv[:, c] == v) & ((hsv[:, rest] >= np.asarray(lo)[rest]) & (hsv[:, rest] <= np.asarray(hi)[rest])).all(axis=1)
        pools[tag] = cand[sel]
    assert all(len(p) >= 10 for p in pools.values()), {k: len(p) for k, p in pools.items()}
    return pools


def paint(s, seed):
    """(colour [rows x cols x 3] BGR, occluder [rows x cols], lower, upper): the scene's masked pixels painted with colours inside the launch file's range, the
    others with colours one unit outside it in H, S or V -- except a few, painted inside the range behind an occluder byte of 0."""
    import colour_ref
    rng = np.random.default_rng(seed)
    pools = _colour_pools()
    want = np.asarray(s.mask).reshape(-1) != 0
    P = want.size
    colour = np.zeros((P, 3), np.uint8)
    colour[want] = pools["in"][rng.integers(0, len(pools["in"]), int(want.sum()))]
    other = np.nonzero(~want)[0]
    tag = rng.integers(0, 4, len(other))
    for k, name in enumerate(("h_lo", "h_hi", "s_lo", "v_lo")):
        idx = other[tag == k]
        colour[idx] = pools[name][rng.integers(0, len(pools[name]), len(idx))]
    occ = rng.integers(1, 256, P).astype(np.uint8)
    hidden = rng.choice(other, min(200, len(other) // 4), replace=False)
    colour[hidden] = pools["in"][rng.integers(0, len(pools["in"]), len(hidden))]
    occ[hidden] = 0
    lower, upper = colour_ref.LAUNCH_RANGE
    return colour.reshape(s.depth.shape + (3,)), occ.reshape(s.depth.shape), lower, upper
