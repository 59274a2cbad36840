"""Constructed scenes for the painter test over a cell of ropes.  A scene is a cell -- ropes [(Y [M x 3], node_dist, threshold)] in the rig frame, a rig
(intrinsics + rig_to_cam matrices), an image size and a width -- with ONE stated property; `check` asserts it on the reference's own structure
(tests/cell_painter_ref.py), on the CPU.  Coordinates are exact binary fractions where a scene says that keys tie.  The reference's verdict of every scene is
computed once (scenes()) and shared by the CPU and GPU tests."""
import functools

import numpy as np

import cell_painter_ref as CR
import rig_painter_ref as PR
import rig_painter_scenes as PS

CAM, ROWS, COLS, BEHIND = PS.CAM, PS.ROWS, PS.COLS, PS.BEHIND


class Cell:
    def __init__(self, name, Ys, cams, mats, rows=ROWS, cols=COLS, w=10, dists=None, thrs=None, check=None):
        Ys = [np.asarray(Y, dtype=np.float64).reshape(-1, 3) for Y in Ys]
        dists = [np.zeros(len(Y)) for Y in Ys] if dists is None else [np.asarray(d, dtype=np.float64) for d in dists]
        thrs = [0.008] * len(Ys) if thrs is None else list(thrs)
        self.name, self.ropes, self.cams, self.mats, self.rows, self.cols, self.w, self.check = name, list(zip(Ys, dists, thrs)), list(cams), mats, rows, cols, w, check
        self.F, self.K, self.Ms = len(Ys), len(self.cams), [len(Y) for Y in Ys]
        self.N = sum(self.Ms)
        self.off = np.concatenate(([0], np.cumsum(self.Ms))).astype(int)

    def ref(self, variant=None):
        return CR.cell_verdict(self.ropes, self.cams, self.mats, self.rows, self.cols, self.w, variant)

    def cell(self):
        """The scene as Context.cell_occlusion_batch takes a cell."""
        return (self.ropes, self.cams, self.mats, self.w)

    def permuted(self, order, name=None):
        Ys, ds, ts = zip(*[self.ropes[f] for f in order])
        return Cell(name or self.name + " permuted", Ys, self.cams, self.mats, self.rows, self.cols, self.w, ds, ts)


def hidden_set(per):
    return {n for n, h in enumerate(per["hidden"]) if h}


def hiders(c, n, w):
    """The painted edges that stand strictly before first(n) and cover node n's pixel, from the reference's structure of one camera."""
    return sorted(e for e, r in c["rank"].items() if r < c["first"][n] and PR.covers(c["px"][n], c["px"][e], c["px"][e + 1], w))


def line_x(z, y=0.0, n=9, half=0.25):
    return [(half * (2 * i - (n - 1)) / (n - 1), y, z) for i in range(n)]


def line_y(z, x=0.0, n=9, half=0.25):
    return [(x, half * ((n - 1) - 2 * i) / (n - 1), z) for i in range(n)]


# ---- two ropes cross at different depths: the lower one loses exactly the node under the crossing; swapping the depths swaps the victims ----------------
def scene_crossing(swap):
    za, zb = (1.0625, 1.0) if swap else (1.0, 1.0625)

    def check(s, vis, seen, hidden, per):
        assert hidden_set(per[0]) == ({4} if swap else {9 + 4})
        assert all(per[0]["seen"])
        assert [list(v) for v in vis] == ([[0, 1, 2, 3, 5, 6, 7, 8], list(range(9))] if swap else [list(range(9)), [0, 1, 2, 3, 5, 6, 7, 8]])
    return Cell("crossing" + (", depths swapped" if swap else ""), [line_x(za), line_y(zb)], [CAM], None, check=check)


# ---- mirror tie: the crossing edges of both ropes have exactly equal keys, the flat index decides; permuting the ropes moves the hidden node ------------
def mirror_ropes():
    A = [(-0.5, -0.5, 1.0), (-0.375, -0.375, 1.0), (-0.25, -0.25, 1.0), (-0.125, -0.125, 1.0), (0.0, 0.0, 1.0), (0.125, 0.125, 1.0)]      # crossing edges: local 3, 4
    B = [(0.125, -0.125, 1.0), (0.0, 0.0, 1.0), (-0.125, 0.125, 1.0)]                                                                    # crossing edges: local 0, 1
    return A, B


def scene_mirror(permute):
    A, B = mirror_ropes()

    def check(s, vis, seen, hidden, per):
        c = per[0]
        ea, eb = (3 + 3, 0) if permute else (3, 6)                                   # flat index of A's and B's first crossing edge
        assert c["keys"][ea] == c["keys"][ea + 1] == c["keys"][eb] == c["keys"][eb + 1]
        later_mid = (3 + 4) if permute else (6 + 1)                                  # the middle node of the rope that stands second
        assert hidden_set(c) == {later_mid}
    return Cell("mirror tie" + (", permuted" if permute else ""), [B, A] if permute else [A, B], [CAM], None, w=6, check=check)


# ---- block boundaries: the covering edge and the covered node on either side of flat indices 63|64, 255|256, 511|512 ----------------------------------
BOUNDARY_MS = (63, 1, 192, 256, 45)
BOUNDARY_PAIRS = ((63, 64 + 90), (64, 30), (255, 256 + 100), (256, 64 + 120), (511, 512 + 20), (512, 256 + 150))      # (victim node, covering edge), flat


def scene_boundaries():
    Ys = []
    for f, M in enumerate(BOUNDARY_MS):
        Ys.append(np.array([(-0.3 + 0.6 * (i + 0.5) / M, -0.2 + 0.1 * f, 1.0 + f / 16.0) for i in range(M)]))
    flat = np.concatenate(Ys)
    off = np.concatenate(([0], np.cumsum(BOUNDARY_MS)))
    for v, e in BOUNDARY_PAIRS:                                                      # the victim goes behind the middle of its edge, on the same ray
        mid = (flat[e] + flat[e + 1]) / 2
        f = int(np.searchsorted(off, v, side="right") - 1)
        Ys[f][v - off[f]] = mid * (1.5 / mid[2])

    def check(s, vis, seen, hidden, per):
        c = per[0]
        for v, e in BOUNDARY_PAIRS:
            b = 64 if v in (63, 64) else 256 if v in (255, 256) else 512
            h = hiders(c, v, s.w)
            assert c["hidden"][v] and e in h and all((x < b) != (v < b) for x in h), (v, e, h)
        assert c["first"][63] == c["n_painted"]                                      # the rope of one node has no edge
    return Cell("block boundaries", Ys, [CAM], None, w=6, check=check)


# ---- tiny ropes: M = 1 has no edge, M = 2 has both nodes sharing one incident edge ------------------------------------------------------------------
def scene_tiny():
    Ys = [line_x(1.0), [(0.0, 0.0, 1.0625)], [(-0.125, 0.0, 1.125), (-0.0625, 0.0, 1.125)], [(0.0, 0.125, 0.5)]]

    def check(s, vis, seen, hidden, per):
        c = per[0]
        assert c["first"][9] == c["n_painted"] == c["first"][12] and c["first"][10] == c["first"][11] == c["rank"][10]
        assert hidden_set(c) == {9, 10, 11} and [list(v) for v in vis[1:]] == [[], [], [0]]
    return Cell("tiny ropes", Ys, [CAM], None, check=check)


# ---- no phantom edge: the segment from the last node of rope 0 to the first node of rope 1 would cover rope 2's middle node -----------------------------
def scene_no_phantom():
    Ys = [[(-0.25, -0.25, 1.0), (-0.25, -0.125, 1.0), (-0.25, 0.0, 1.0)], [(0.25, 0.0, 1.0), (0.25, 0.125, 1.0), (0.25, 0.25, 1.0)],
          [(0.0, -0.125, 1.25), (0.0, 0.0, 1.25), (0.0, 0.125, 1.25)]]

    def check(s, vis, seen, hidden, per):
        c = per[0]
        assert c["drawable"][2] and c["drawable"][3] and 2 not in c["painted"] and abs(c["px"][2][0] - c["px"][3][0]) == 250
        assert PR.covers(c["px"][7], c["px"][2], c["px"][3], s.w) and not hidden_set(c)
    return Cell("no phantom edge", Ys, [CAM], None, check=check)


# ---- undrawable parts: one rope wholly behind the camera, another with one undrawable node in the middle -----------------------------------------------
def scene_undrawable():
    behind = [(x, 0.0, -1.0) for x in (-0.1, 0.0, 0.1, 0.2)]
    broken = [(-0.125, 0.0, 1.0625), (-0.0625, 0.0, 1.0625), (0.0, 0.0, -1.0), (0.0625, 0.0, 1.0625), (0.125, 0.0, 1.0625)]
    over = line_y(1.0, x=0.0625 / 1.0625, n=5, half=0.125)

    def check(s, vis, seen, hidden, per):
        c = per[0]
        assert not any(c["drawable"][:4]) and not any(c["painted"][e] for e in range(3))
        assert [c["painted"][e] for e in range(4, 8)] == [True, False, False, True]
        assert c["first"][5] == c["rank"][4] and c["first"][7] == c["rank"][7] and not c["drawable"][6] and not c["hidden"][6]
        assert hidden_set(c) == {7} and list(vis[0]) == [] and list(vis[1]) == [0, 1, 4]
    return Cell("undrawable parts", [behind, broken, over], [CAM], None, check=check)


# ---- a node outside the image that is hidden but not seen ---------------------------------------------------------------------------------------------
def scene_off_image():
    Ys = [[(0.5 + 0.05 * i, 0.0, 1.0) for i in range(9)], line_y(1.0625, x=0.7 * 1.0625, n=9, half=0.25)]

    def check(s, vis, seen, hidden, per):
        c = per[0]
        assert c["px"][9 + 4][0] >= COLS and c["drawable"][9 + 4] and c["hidden"][9 + 4] and not c["seen"][9 + 4] and 4 not in vis[1]
    return Cell("off-image node", Ys, [CAM], None, check=check)


def scene_one_node():
    def check(s, vis, seen, hidden, per):
        assert [list(v) for v in vis] == [[0]] and seen.tolist() == [[1]] and hidden.tolist() == [[0]]
    return Cell("one node", [[(0.0, 0.0, 1.0)]], [CAM], None, check=check)


def scene_many_cameras():
    rng = np.random.default_rng(91)
    cams, mats = PS.random_rig(rng, 64)
    mats = [None if k % 7 == 3 else m for k, m in enumerate(mats)]

    def check(s, vis, seen, hidden, per):
        assert s.K == 64 and sum(m is None for m in s.mats) >= 9 and any(hidden_set(c) for c in per)
    return Cell("many cameras", [PS.rope(rng, M) for M in (33, 20, 45)], cams, mats, w=12, check=check)


# ---- a node hidden in camera 0 is seen and not hidden in camera 1: it stays visible ---------------------------------------------------------------------
def scene_second_camera():
    def check(s, vis, seen, hidden, per):
        assert hidden_set(per[0]) == {9 + 4} and per[1]["seen"][9 + 4] and not per[1]["hidden"][9 + 4] and hidden_set(per[1]) == {4}
        assert [list(v) for v in vis] == [list(range(9)), list(range(9))]
    return Cell("second camera saves a node", [line_x(1.0), line_y(1.0625)], [CAM, CAM], [None, BEHIND], check=check)


# ---- the largest cell: 14 parallel lines at staggered depths and two ropes that cross them all, 16 ropes of 1024 nodes ---------------------------------
def scene_largest():
    """The nodes of a rope lie more than w / 2 pixels apart (a 4096 x 4096 image), so a straight rope does not hide itself and only the crossings hide."""
    M = 1024
    cam = (4000.0, 4000.0, 2048.0, 2048.0)
    Ys = [np.array([(-0.5 + 1.0 * i / (M - 1), -0.21 + 0.03 * f, 1.0 + f / 64.0) for i in range(M)]) for f in range(14)]      # at least 3.2 pixels a step
    Ys.append(np.array([(-0.1, -0.45 + 0.9 * i / (M - 1), 0.9) for i in range(M)]))              # in front of every line
    Ys.append(np.array([(0.1, -0.6 + 1.2 * i / (M - 1), 1.5) for i in range(M)]))                # behind every line

    def check(s, vis, seen, hidden, per):
        c = per[0]
        assert s.N == 16384 and c["survivors"] < 10 ** 6 and all(c["seen"])
        h = hidden_set(c)
        assert all(1 <= sum(f * M <= n < (f + 1) * M for n in h) <= 4 for f in range(14))         # the front rope hides a node or two of every line, no more
        assert 14 <= sum(15 * M <= n for n in h) <= 56 and not any(14 * M <= n < 15 * M for n in h)      # the back rope loses nodes under every line
    return Cell("largest cell", Ys, [cam], None, rows=4096, cols=4096, w=4, check=check)


def random_cell(rng, F=None, K=None, name="random", Mmax=40):
    F = int(rng.integers(1, 6)) if F is None else F
    K = int(rng.integers(1, 5)) if K is None else K
    cams, mats = PS.random_rig(rng, K)
    Ms = [int(rng.integers(1, Mmax + 1)) for _ in range(F)]
    return Cell(name, [PS.rope(rng, M) for M in Ms], cams, mats, w=int(rng.integers(1, 40)), dists=[rng.uniform(0, 0.016, M) for M in Ms],
                thrs=[float(rng.uniform(0.004, 0.012)) for _ in Ms])


@functools.lru_cache(maxsize=None)
def scenes():
    """Every constructed scene with the reference's verdict: [(scene, vis, seen_words, hidden_words, per_camera)]."""
    made = [scene_crossing(False), scene_crossing(True), scene_mirror(False), scene_mirror(True), scene_boundaries(), scene_tiny(), scene_no_phantom(),
            scene_undrawable(), scene_off_image(), scene_one_node(), scene_many_cameras(), scene_second_camera()]
    return [(s, ) + tuple(s.ref()) for s in made]


@functools.lru_cache(maxsize=None)
def largest():
    s = scene_largest()
    return (s, ) + tuple(s.ref())


@functools.lru_cache(maxsize=None)
def batches():
    """C = 1, 2 and 33 cells of unequal F, N and K; the tests run every batch in both orders."""
    rng = np.random.default_rng(92)
    all_ = scenes()
    many = []
    for i in range(33):
        s = random_cell(rng, K=1 if i in (0, 32) else None, name=f"batch cell {i}")
        many.append((s, ) + tuple(s.ref()))
    return {"C=1": [all_[0]], "C=2": [all_[5], all_[11]], "C=33": many}
