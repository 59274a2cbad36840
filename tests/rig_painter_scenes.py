"""Constructed scenes for the self-occlusion test under a rig.  A scene is nodes Y [M x 3] in the rig frame, a rig (intrinsics + rig_to_cam matrices), an image
size, a width, distances and a threshold; `check` asserts the scene's own property on the reference (tests/rig_painter_ref.py), on the CPU.  The reference's
verdict of every scene is computed once (scenes()) and shared by the CPU and GPU tests."""
import functools
from fractions import Fraction

import numpy as np

import rig_painter_ref as PR

CAM = (500.0, 500.0, 320.0, 240.0)
ROWS, COLS = 480, 640
BEHIND = np.array([[-1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, -1.0, 2.05]])      # a camera on the other side of the crossing, looking back at the first
IDENT = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


class Scene:
    def __init__(self, name, Y, cams, mats, rows=ROWS, cols=COLS, w=10, dist=None, thr=0.008, check=None):
        self.name, self.Y, self.cams, self.mats, self.rows, self.cols, self.w = name, np.asarray(Y, dtype=np.float64), list(cams), mats, rows, cols, w
        self.dist = np.zeros(len(self.Y)) if dist is None else np.asarray(dist, dtype=np.float64)
        self.thr, self.check = thr, check
        self.M, self.K = len(self.Y), len(self.cams)

    def ref(self, variant=None):
        return PR.rig_verdict(self.Y, self.cams, self.mats, self.rows, self.cols, self.w, self.dist, self.thr, variant)

    def frame(self):
        """The scene as Context.rig_self_occlusion_batch takes a frame."""
        return (self.Y, self.cams, self.mats, self.w, self.dist, self.thr)


def hidden_set(per):
    return {m for m, h in enumerate(per["hidden"]) if h}


# ---- the crossing: strand A along x at z = 1.00, strand B along y at z = 1.05, both with a node on the optical axis ----------------------------------
def crossing():
    A = [(x, 0.0, 1.0) for x in np.linspace(-0.2, 0.2, 9)]                       # node 4 = (0, 0, 1)
    link = [(0.3, 0.1, 1.02), (0.3, 0.3, 1.03), (0.1, 0.3, 1.04)]
    Bs = [(0.0, y, 1.05) for y in np.linspace(0.2, -0.2, 9)]                      # node 12 + 4 = 16 = (0, 0, 1.05)
    return np.array(A + link + Bs), 4, 16


def scene_a():
    Y, a_mid, b_mid = crossing()

    def check(s, vis, seen, hidden, per):
        assert hidden_set(per[0]) == {b_mid} and hidden_set(per[1]) == {a_mid}      # each camera alone hides a different strand's node
        assert all(all(c["seen"]) for c in per)
        assert list(vis) == list(range(s.M))                                        # the rig hides none
    return Scene("a crossing, opposite sides", Y, [CAM, CAM], [None, BEHIND], check=check)


def scene_b():
    Y, a_mid, b_mid = crossing()
    beside = IDENT.copy(); beside[0, 3] = -0.02

    def check(s, vis, seen, hidden, per):
        assert b_mid in hidden_set(per[0]) and b_mid in hidden_set(per[1]) and b_mid not in vis and a_mid in vis
    return Scene("b crossing, one side", Y, [CAM, CAM], [None, beside], check=check)


def scene_c(inside):
    """(b) with a third camera behind the crossing whose principal point puts the hidden node's pixel at column COLS (one outside) or COLS - 1."""
    Y, a_mid, b_mid = crossing()
    beside = IDENT.copy(); beside[0, 3] = -0.02
    third = (500.0, 500.0, float(COLS - 1 if inside else COLS), 240.0)

    def check(s, vis, seen, hidden, per):
        assert per[2]["px"][b_mid][0] == (COLS - 1 if inside else COLS) and per[2]["drawable"][b_mid] and not per[2]["hidden"][b_mid]
        assert per[2]["seen"][b_mid] == inside and (b_mid in vis) == inside
    return Scene("c third camera, one column " + ("in" if inside else "out"), Y, [CAM, CAM, third], [None, beside, BEHIND], check=check)


def scene_d():
    """Node 0 has z_c < 0 and node 1 has z_c exactly 0 in camera 1 (its matrix takes node 1's z away)."""
    Y = np.array([(0.05 * m - 0.1, 0.01 * m, 0.8 + 0.1 * m) for m in range(6)] + [(-0.16, -0.07, 1.4)])
    # (node 6's pixel in camera 1 is (160, 170) to a pixel, half way from pixel (0, 0) to node 2's (320, 340): a reading that ranks and paints the edges that are NOT
    # painted, from the pixel (0, 0) a node that cannot be drawn is left with, hides it there)
    T = IDENT.copy(); T[2, 3] = -Y[1, 2]

    def check(s, vis, seen, hidden, per):
        c = per[1]
        q = [PR.cam_node(T, y) for y in s.Y]
        assert q[0][2] < 0 and q[1][2] == 0.0 and q[2][2] > 0
        assert c["drawable"][:3] == [False, False, True] and c["painted"][:3] == [False, False, True]
        assert c["n_painted"] == 4 and c["first"][1] == 4 and c["first"][0] == 4 and c["first"][2] == c["rank"][2]
        assert not c["seen"][0] and not c["hidden"][0] and not c["hidden"][1]
        assert c["px"][2] == (320, 340) and max(abs(c["px"][6][0] - 160), abs(c["px"][6][1] - 170)) <= 1 and not c["hidden"][6]
    return Scene("d z_c zero and negative", Y, [CAM, CAM], [None, T], check=check)


def scene_e():
    """Edges 0 and 2 lie on one line in the image; their squared mid-point distances differ by one ulp (edge 0's is the larger) and the roots are equal, so the
    index decides: edge 0 is painted first and covers nodes 2 and 3.  A sort on the squares would paint edge 2 first and hide neither."""
    d, y, z, x0 = 0.02, 0.1, 1.0, 0.001
    n0, n1 = (x0 - d, y, z), (x0 + d, y, z)
    k0, s0 = PR.edge_key([np.float64(v) for v in n0], [np.float64(v) for v in n1], True)
    for k in range(1, 20000):
        x1 = x0 - k * 2e-14
        n2, n3 = (d - x1, y, z), (-x1 - d, y, z)
        k2, s2 = PR.edge_key([np.float64(v) for v in n2], [np.float64(v) for v in n3], True)
        if s0 == np.nextafter(s2, np.inf) and k0 == k2:
            break
    else:
        raise AssertionError("no pair of edges one ulp apart")
    Y = np.array([n0, n1, n2, n3])

    def check(s, vis, seen, hidden, per):
        c = per[0]
        a, sa = PR.edge_key(list(s.Y[0]), list(s.Y[1]), True); b, sb = PR.edge_key(list(s.Y[2]), list(s.Y[3]), True)
        assert a == b and sa != sb and sa == np.nextafter(sb, np.inf)               # the keys are equal, the squares are not
        assert c["rank"][0] < c["rank"][2] and hidden_set(c) == {2, 3} and list(vis) == [0, 1]
    return Scene("e equal roots, index decides", Y, [CAM], None, w=5, check=check)


def scene_f():
    Y, a_mid, b_mid = crossing()
    Y = np.repeat(Y, 2, axis=0)                                                     # every node twice: every other edge has length zero

    def check(s, vis, seen, hidden, per):
        assert {2 * b_mid, 2 * b_mid + 1} & hidden_set(per[0]) and not ({2 * b_mid, 2 * b_mid + 1} & hidden_set(per[1]))
    return Scene("f coincident nodes", Y, [CAM, CAM], [None, BEHIND], check=check)


def scene_g(w):
    Y, a_mid, b_mid = crossing()

    def check(s, vis, seen, hidden, per):
        assert b_mid in hidden_set(per[0])
        if w == 255:
            assert len(hidden_set(per[0])) > 5                                       # a quarter of the image under every line
    return Scene(f"g width {w}", Y, [CAM, CAM], [None, BEHIND], w=w, check=check)


def scene_h():
    """fx = 1, cx = 0, z = 1: the column is the truncated x.  Pixels at -8192 and 8191 are drawable, at -8193 and 8192 they are not."""
    xs = [-8193.0, -8192.5, -4000.25, 0.5, 4000.25, 8191.5, 8192.0, 8191.999, 100.0, -8192.999]
    Y = np.array([(x, 0.25 * (m % 3), 1.0) for m, x in enumerate(xs)])
    cam = (1.0, 1.0, 0.0, 0.0)

    def check(s, vis, seen, hidden, per):
        c = per[0]
        assert c["drawable"] == [False, True, True, True, True, True, False, True, True, True]
        assert c["px"][1][0] == -8192 and c["px"][5][0] == 8191 and c["px"][7][0] == 8191 and c["px"][9][0] == -8192
        assert c["seen"] == [False, False, False, True, True, True, False, True, True, False]
    return Scene("h pixels at the rule's ends", Y, [cam], None, rows=8192, cols=8192, w=255, check=check)


def scene_i():
    Y, a_mid, b_mid = crossing()
    dist = np.full(len(Y), 0.001); dist[2] = np.nan; dist[3] = 0.0081; dist[5] = 0.008

    def check(s, vis, seen, hidden, per):
        assert 2 not in vis and 3 not in vis and 5 in vis and b_mid not in vis
    return Scene("i NaN and far distances", Y, [CAM], None, dist=dist, check=check)


def scene_fused():
    """Camera-frame x of node 3 is ((1 x + b y) + 0 z) + 0 with x = -rn(b y): 0 when every product is rounded, the negative rounding residue when the second
    product is fused into its sum.  With cx = 1 the column is 1 against 0; a one-pixel-wide vertical edge at column 1, nearer to the camera, hides the node in
    the first case only."""
    b = 0.1
    for k in range(1, 4000):
        y = 0.5 + k * 2.0 ** -20
        p = float(np.float64(b) * np.float64(y))
        res = Fraction(b) * Fraction(y) - Fraction(p)
        if res < 0 and float(res) * 500.0 < -1e-15:
            break
    else:
        raise AssertionError("no product with a negative rounding residue")
    T = np.array([[1.0, b, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]])
    Y = np.array([(0.0, 0.0, -0.01), (0.0, 0.0, 0.01), (0.3, y, 0.2), (-p, y, 0.0), (-0.3, y, -0.2)])
    cam = (500.0, 500.0, 1.0, 5.0)

    def check(s, vis, seen, hidden, per):
        c = per[0]
        assert PR.cam_node(T, s.Y[3])[0] == 0.0 and PR.cam_node(T, s.Y[3], fused=True)[0] < 0
        assert c["px"][0] == (1, 0) and c["px"][1] == (1, 10) and c["px"][3] == (1, 5) and c["seen"][3]
        assert hidden_set(c) == {3} and 3 not in vis
    return Scene("k fused boundary", Y, [cam], [T], rows=16, cols=640, w=1, check=check)


def rope(rng, M):
    """A rope that crosses itself in the image (the generator of tests/test_abi.py's self-occlusion test)."""
    t = np.linspace(0, 1, M); a = rng.uniform(0.5, 3, 3); ph = rng.uniform(0, 2 * np.pi, 3)
    return np.stack([0.25 * np.sin(2 * np.pi * a[0] * t + ph[0]), 0.2 * np.sin(2 * np.pi * a[1] * t + ph[1]), 0.6 + 0.15 * np.sin(2 * np.pi * a[2] * t + ph[2])], axis=1)


def random_rig(rng, K):
    """K cameras around the rope: rotations about the y axis through (0, 0, 0.6), small shifts, the first camera without a matrix now and then."""
    cams, mats = [], []
    for k in range(K):
        cams.append((float(rng.uniform(400, 700)), float(rng.uniform(400, 700)), float(rng.uniform(250, 390)), float(rng.uniform(180, 300))))
        th = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        c = np.array([0.0, 0.0, 0.6])
        t = -R @ c + np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(0.5, 0.9)])
        mats.append(None if (k == 0 and rng.random() < 0.5) else np.hstack([R, t[:, None]]))
    return cams, (None if all(m is None for m in mats) else mats)


def random_scene(rng, M=None, K=None, name="random"):
    M = int(rng.integers(2, 60)) if M is None else M
    K = int(rng.integers(1, 5)) if K is None else K
    cams, mats = random_rig(rng, K)
    return Scene(name, rope(rng, M), cams, mats, w=int(rng.integers(1, 40)), dist=rng.uniform(0, 0.016, M))


def border_scenes():
    """(j): the wave and block borders of the kernel in M, and K = 1, 2, 64."""
    rng = np.random.default_rng(77)
    out = [random_scene(rng, M, K, f"j M={M} K={K}") for M, K in ((1, 1), (2, 2), (3, 64), (64, 2), (65, 1), (256, 2), (257, 1), (1024, 1))]
    return out


@functools.lru_cache(maxsize=None)
def scenes():
    """Every constructed scene with the reference's verdict: [(scene, vis, seen_words, hidden_words, per_camera)]."""
    made = [scene_a(), scene_b(), scene_c(False), scene_c(True), scene_d(), scene_e(), scene_f(), scene_g(1), scene_g(255), scene_h(), scene_i(), scene_fused()]
    made += border_scenes()
    return [(s, ) + s.ref() for s in made]


@functools.lru_cache(maxsize=None)
def batches():
    """(j) in batches: F = 1, 2 and 33 frames with unequal K_f and unequal M; the frame with the fewest cameras stands first and last."""
    rng = np.random.default_rng(78)
    all_ = scenes()
    one = [all_[0]]
    two = [all_[5], all_[0]]                                                        # K = 1 first ... K = 2
    many = []
    for f in range(33):
        K = 1 if f in (0, 32) else int(rng.integers(2, 5))
        s = random_scene(rng, int(rng.integers(1, 80)), K, f"batch frame {f}")
        many.append((s, ) + s.ref())
    return {"F=1": one, "F=2": two, "F=33": many}
