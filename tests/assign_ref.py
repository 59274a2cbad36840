"""The statement of "one cloud dealt out among F ropes" (include/trackdlo_hip.h, "ropes of one colour") in numpy + exact arithmetic, and its scenes.

D(i, f) = min_m node_point_d2(Y_f[m], X_i) in the fused form of prepass_ref.d2_fused (one right bit pattern), g(i) = min_f D(i, f), owner(i) = the lowest f that
attains g(i) if g(i) is finite and g(i) <= fl(d_max d_max), else -1.  As prepass_ref.min_d2 does, a vectorised pass with plain products narrows every (point,
rope) pair to the nodes within 1e-12 relative of the smallest, and only those are evaluated in the fused form.  The fused multiply-add of that evaluation is the
C library's fma() (correctly rounded, like float(Fraction)): test_assign_ref.py holds it to prepass_ref.fma, the Fraction form, on random operands and on every
point that decides a scene -- a cloud of 70 001 points is beyond Fractions in a test of seconds."""
import ctypes
import ctypes.util
from fractions import Fraction

import numpy as np

import prepass_ref as PR

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
TILE = 512                 # nodes of the kernel's LDS tile (csrc/tdlo_assign_lane.h: kAssignTile)
G = 2.0 ** -26             # the lattice of the exact scenes


def fma(a, b, c):
    return _libm.fma(a, b, c)


def d2_fused(y, x):
    dx, dy, dz = float(y[0]) - float(x[0]), float(y[1]) - float(x[1]), float(y[2]) - float(x[2])
    return fma(dz, dz, fma(dy, dy, dx * dx))


def d2_plain(y, x):
    dx, dy, dz = float(y[0]) - float(x[0]), float(y[1]) - float(x[1]), float(y[2]) - float(x[2])
    return dx * dx + dy * dy + dz * dz


def rope_min(X, Y, d2=d2_fused):
    """D(., f) for one rope: per point the bits of min_m d2(Y[m], X_i); +inf where no term is finite."""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    out = np.full(len(X), np.inf)
    for a in range(0, len(X), 4096):
        Xc = X[a:a + 4096]
        with np.errstate(invalid="ignore", over="ignore"):
            d = Y[None, :, :] - Xc[:, None, :]
            P = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        P = np.where(np.isnan(P), np.inf, P)
        lo = P.min(axis=1)
        for i in np.nonzero(np.isfinite(lo))[0]:
            out[a + i] = min(d2(Y[m], Xc[i]) for m in np.nonzero(P[i] <= lo[i] * (1.0 + 1e-12))[0])
    return out


def assign(X, ropes, d_max, d2=d2_fused, tie="lowest", gate="<="):
    """The statement: (owner [n] int32, owner_d2 [n], n_each [F], n_unowned).  d2 / tie / gate: the wrong readings test_assign_ref.py tells from it."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    g = np.full(len(X), np.inf); owner = np.full(len(X), -1, dtype=np.int32)
    for f, Y in enumerate(ropes):
        D = rope_min(X, Y, d2)
        better = D < g if tie == "lowest" else (D <= g) & np.isfinite(D)
        g[better] = D[better]; owner[better] = f
    dmax2 = float(d_max) * float(d_max)
    ok = np.isfinite(g) & ((g <= dmax2) if gate == "<=" else (g < dmax2))
    owner[~ok] = -1
    return owner, g, [int((owner == f).sum()) for f in range(len(ropes))], int((owner < 0).sum())


def split(X, owner, F):
    """The destination clouds: the points of every rope in ascending source order (column-major, as tdlo_get_cloud returns them)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    return [np.asfortranarray(X[owner == f]) for f in range(F)]


def visibility(Xf, Y, visibility_threshold, d_vis, coord):
    """tdlo_visibility_prepass of one destination (a rope that owns nothing: 100000 everywhere, no visible node)."""
    return PR.threshold_and_fill(PR.min_d2(Xf, Y)[0], visibility_threshold, d_vis, coord)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------------
def rope(M, k, rng, spacing=0.012):
    """Rope k: M nodes along a wavy line at height 0.05 k, and its chain coordinate."""
    s = np.arange(M) * spacing
    Y = np.stack([0.1 + s, 0.2 + 0.05 * k + 0.01 * np.sin(7.0 * s + k), 0.6 + 0.01 * np.cos(5.0 * s + 2 * k)], axis=1) + rng.normal(0, 2e-4, (M, 3))
    coord = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(Y, axis=0), axis=1))]) if M > 1 else np.zeros(1)
    return np.asfortranarray(Y), coord


def cloud_scene(n, Ms, seed=0, far=0.1):
    """(X [n x 3], ropes, coords): point i lies within 4 mm of a random node of rope i mod F -- the ropes interleaved point by point, so every rope's run
    crosses every block border -- except a share `far` of the points, which lie 3 cm and more from every rope."""
    rng = np.random.default_rng(4100 + 17 * seed + n % 9973 + 3 * len(Ms))
    rc = [rope(M, k, rng) for k, M in enumerate(Ms)]
    ropes = [r[0] for r in rc]; F = len(Ms)
    X = np.empty((n, 3))
    for i in range(n):
        Y = ropes[i % F]
        X[i] = Y[rng.integers(len(Y))] + rng.normal(0, 1.5e-3, 3)
    out = rng.random(n) < far
    X[out, 2] += 0.03 + 0.05 * rng.random(int(out.sum()))
    return np.asfortranarray(X), ropes, [r[1] for r in rc]


def lattice(v):
    return np.round(np.asarray(v, dtype=np.float64) / G) * G


def tie_scene():
    """Three ropes of 300, 300 and 45 nodes (645 > TILE: the list has two tiles) on the 2^-26 lattice.  Point 0 is equidistant -- exactly: every difference,
    square and sum is exact -- from node 7 of rope 0 (tile 0) and node 40 of rope 2 (flat index 640: tile 1), and farther from everything else; the rest of
    the cloud is ordinary.  Returns (X, ropes, d_max, the tied point's index)."""
    rng = np.random.default_rng(4242)
    ropes = [np.array(lattice(rope(M, k, rng)[0]), order="F") for k, M in enumerate((300, 300, 45))]
    p = lattice([2.0, 0.3, 0.9])                               # far from the ropes' run
    ropes[0][7] = p + np.array([30001.0, -20003.0, 10007.0]) * G
    ropes[2][40] = p + np.array([-20003.0, 10007.0, 30001.0]) * G
    ropes[1][150] = p + np.array([30001.0, 20003.0, 10008.0]) * G   # rope 1: a little farther
    X, _, _ = cloud_scene(300, (300, 300, 45), seed=5)
    X = np.array(X, order="F"); X[0] = p
    return X, ropes, np.inf, 0


def gate_scene():
    """Two single-node ropes and d_max = 5 s 2^-26 (s = 60 000: 4.47 mm) on the lattice: point 0 has g = fl(d_max^2) EXACTLY (offset (3 s, 4 s, 0)), point 1 has
    g one ulp above it (offset (2^-34, 5 s, 0): g = d_max^2 + 2^-68), point 2 lies well inside, point 3 well outside.  Returns (X, ropes, d_max)."""
    s = 60000.0
    y0 = lattice([0.3, 0.3, 0.6]); y1 = y0 + np.array([0.0, 0.5, 0.0])
    d_max = 5.0 * s * G
    X = np.array([y0 + np.array([3 * s, 4 * s, 0.0]) * G, y0 + np.array([2.0 ** -34, 5 * s * G, 0.0]), y1 + np.array([1000.0, 0.0, 0.0]) * G,
                  y0 + np.array([0.0, 0.1, 0.0])], order="F")
    return X, [np.asfortranarray(y0[None, :]), np.asfortranarray(y1[None, :])], d_max


_FLIP = []


def fused_flip_scene():
    """Found by search (seed fixed): a point and two single-node ropes for which the fused distances and the plain-product distances order the ropes
    differently.  Returns (X [1 x 3], ropes)."""
    if not _FLIP:
        rng = np.random.default_rng(20260)
        for _ in range(200000):
            p = rng.uniform(0.2, 0.9, 3); o = rng.uniform(-0.01, 0.01, 3)
            a, b = p + o, p + o[[2, 0, 1]] * rng.choice([-1.0, 1.0], 3)
            fa, fb, pa, pb = d2_fused(a, p), d2_fused(b, p), d2_plain(a, p), d2_plain(b, p)
            if (fa < fb and pb < pa) or (fb < fa and pa < pb):
                _FLIP.append((np.asfortranarray(p[None, :]), [np.asfortranarray(a[None, :]), np.asfortranarray(b[None, :])]))
                break
    return _FLIP[0]


def with_specials(X, seed=0):
    """X with points that have NaN / infinite coordinates (never owned) and signed zeros inserted at the front, the middle and the end.  Returns (cloud, the
    indices of the non-finite points)."""
    X = np.array(X, order="F")
    n = len(X)
    bad = sorted({0, min(63, n - 1), n // 2, n - 1})
    pat = [(np.nan, 0.3, 0.6), (0.3, np.inf, 0.6), (-np.inf, 0.3, 0.6), (np.nan, np.nan, np.nan)]
    for k, i in enumerate(bad):
        X[i] = pat[k % len(pat)]
    return X, bad


def zero_scene():
    """A rope through the origin and points with -0.0 and +0.0 coordinates next to it: the sign of a zero must survive the copy."""
    Y = np.asfortranarray(np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]]))
    X = np.asfortranarray(np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.001], [0.002, -0.0, -0.0], [-0.0, -0.0, -0.0]]))
    return X, [Y, np.asfortranarray(np.array([[0.0, 0.5, 0.0]]))]


def crossing_ropes(M=45, frames=10, n=1500, seed=3):
    """Two ropes of M nodes that cross in the image plane 3 cm apart in depth, drifting over `frames` frames: (Y0 [2], coords [2], [cloud per frame])."""
    rng = np.random.default_rng(900 + seed)
    s = np.arange(M) * 0.012
    base = [np.stack([0.1 + s, 0.2 + 0.3 * s, 0.60 + 0 * s], axis=1), np.stack([0.1 + s, 0.36 - 0.3 * s, 0.63 + 0 * s], axis=1)]
    coords = [np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(b, axis=0), axis=1))]) for b in base]
    clouds = []
    for fr in range(frames):
        pts = []
        for k, b in enumerate(base):
            t = rng.uniform(0, M - 1, n // 2); i0 = np.floor(t).astype(int); w = (t - i0)[:, None]
            c = b[i0] * (1 - w) + b[np.minimum(i0 + 1, M - 1)] * w
            pts.append(c + np.array([0.0005 * fr, 0.0003 * fr * (1 - 2 * k), 0.0]) + rng.normal(0, 8e-4, c.shape))
        X = np.concatenate(pts); X = X[rng.permutation(len(X))]
        clouds.append(np.asfortranarray(X))
    return [np.asfortranarray(b) for b in base], coords, clouds
