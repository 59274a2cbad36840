"""Exact reference of the visibility pre-pass (trackdlo_node.cpp:257-277, :316, :345-360) as the library computes it, and the scenes it is tested on.

The kernels (k_node_min_dist, k_node_min_dist_direct, the ride-along in k_cloud_team) form a node's squared distance to a point as
node_point_d2: dx = fl(y - x) per coordinate, then fma(dz, dz, fma(dy, dy, fl(dx dx))), take the minimum over the cloud (fmin: a NaN never wins)
and the host takes sqrt, caps at the reference's starting value 100000 (:261), thresholds (<=, :316) and fills the gaps (:345-360).  Every step is
correctly rounded, so the result has ONE right bit pattern; `min_d2` gives it: a vectorised fp64 pass with plain products finds, per node, the points
whose distance lies within 1e-12 relative of the smallest (the fused and the plain value differ by less than 4 u), and only those are evaluated
exactly -- a fused multiply-add as float(Fraction(a) Fraction(b) + Fraction(c)), which Python rounds correctly.

Scenes (`scene`): every point that decides a result is known.  A far field lies at least 5 cm from every node; the nodes are gathered around a few
WITNESS points, node m at a distance r_m of its own (distinct, 1 mm .. 2 cm) from witness m mod K, and the K witnesses sit at the cloud indices where
a kernel goes wrong (`index_list`): the first and last lanes of waves and workgroups, the ragged last wave, both sides of the 262 144-point border
behind which the grid-stride loop takes its second trip."""
from fractions import Fraction

import numpy as np

START = 100000.0          # trackdlo_node.cpp:261
TRIP = 1024 * 256         # points of one trip of the pre-pass kernels' grid-stride loop (launch_node_min_dist*: at most 1024 workgroups of 256)


def fma(a, b, c):
    """fl(a b + c) for finite doubles, one rounding."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def d2_fused(y, x):
    """node_point_d2 for one finite node / point pair."""
    dx, dy, dz = float(y[0]) - float(x[0]), float(y[1]) - float(x[1]), float(y[2]) - float(x[2])
    return fma(dz, dz, fma(dy, dy, dx * dx))


def _plain_d2(X, y):
    with np.errstate(invalid="ignore", over="ignore"):
        dx = y[0] - X[:, 0]; dy = y[1] - X[:, 1]; dz = y[2] - X[:, 2]
        d2 = dx * dx + dy * dy + dz * dz
    return np.where(np.isnan(d2), np.inf, d2)


def min_d2(X, Y):
    """Per node the bits of min_n node_point_d2 (+inf for a cloud without a point at a finite distance), and the index of the first point that attains it (-1)."""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    out = np.full(len(Y), np.inf); arg = np.full(len(Y), -1, dtype=np.int64)
    for m, y in enumerate(Y):
        d2 = _plain_d2(X, y)
        lo = d2.min() if len(d2) else np.inf
        if not np.isfinite(lo):
            continue
        for n in np.nonzero(d2 <= lo * (1.0 + 1e-12))[0]:
            v = d2_fused(y, X[n])
            if v < out[m]:
                out[m] = v; arg[m] = n
    return out, arg


def fill_gaps(vis, coord, d_vis):
    """trackdlo_node.cpp:348-360."""
    ext = []
    for i in range(len(vis) - 1):
        ext.append(int(vis[i]))
        if abs(coord[vis[i + 1]] - coord[vis[i]]) <= d_vis:
            ext.extend(range(int(vis[i]) + 1, int(vis[i + 1])))
    if len(vis):
        ext.append(int(vis[-1]))
    return np.asarray(ext, dtype=np.int32)


def threshold_and_fill(d2, visibility_threshold, d_vis, coord):
    dist = np.minimum(np.sqrt(d2), START)
    vis = np.nonzero(dist <= visibility_threshold)[0].astype(np.int32)
    return dist, vis, fill_gaps(vis, np.asarray(coord, dtype=np.float64), d_vis)


def prepass(X, Y, visibility_threshold, d_vis, coord):
    """(node_dist, visible_nodes, visible_nodes_extended) of tdlo_visibility_prepass, bit for bit."""
    return threshold_and_fill(min_d2(X, Y)[0], visibility_threshold, d_vis, coord)


def nearest_two(X, Y):
    """Per node the index of its nearest point and the distances to it and to the nearest of all OTHER points (plain fp64: for margins of centimetres)."""
    X = np.asarray(X, dtype=np.float64)
    arg = np.zeros(len(Y), dtype=np.int64); d1 = np.zeros(len(Y)); d2nd = np.zeros(len(Y))
    for m, y in enumerate(np.asarray(Y, dtype=np.float64)):
        d2 = _plain_d2(X, y)
        n = int(d2.argmin())
        arg[m] = n; d1[m] = min(np.sqrt(d2[n]), START)
        d2[n] = np.inf
        d2nd[m] = min(np.sqrt(d2.min()), START) if len(d2) > 1 else START
    return arg, d1, d2nd


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def index_list(N):
    """Where witnesses are written: first / last lanes of the first waves and workgroups, the ragged last wave, the border of the second trip and
    the first lane of the second trip's last wave."""
    cand = [0, 63, 64, 255, 256, N - 1, N - 2]
    if N > TRIP:
        cand += [TRIP - 1, TRIP, TRIP + (N - 1 - TRIP) // 64 * 64]
    out = []
    for i in cand:
        if 0 <= i < N and i not in out:
            out.append(i)
    return out


def scene(N, M, seed=0, far_nodes=()):
    """Returns (X [N x 3, column-major], Y [M x 3], coord [M], idx [K witness indices], r [M]).  Node m lies r[m] from X[idx[m mod K]]; the nodes in
    `far_nodes` lie 6 .. 7 cm from their witness instead of 1 mm .. 2 cm; every other point of the cloud is at least 5 cm from every node."""
    rng = np.random.default_rng(77000 + 131 * seed + 7 * M + N % 9973)
    idx = index_list(N); K = len(idx)
    side = int(np.ceil(np.sqrt(K)))
    W = np.array([[0.25 * (j % side), 0.25 * (j // side), 0.6] for j in range(K)]) + rng.uniform(-0.01, 0.01, (K, 3))
    r = 0.001 + 0.019 * (rng.permutation(M) + 0.5) / M
    for m in far_nodes:
        r[m] = 0.06 + 0.01 * (m + 0.5) / M
    u = rng.normal(size=(M, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    Y = W[np.arange(M) % K] + r[:, None] * u
    X = np.empty((N, 3))
    X[:, 0] = rng.uniform(-0.1, 0.25 * side, N); X[:, 1] = rng.uniform(-0.1, 0.25 * side, N)
    X[:, 2] = 0.6 + rng.choice([-1.0, 1.0], N) * rng.uniform(0.16, 0.5, N)        # nodes: |z - 0.6| <= 0.01 + 0.07
    X[idx] = W
    coord = np.concatenate([[0.0], np.cumsum(rng.uniform(0.015, 0.025, M - 1))]) if M > 1 else np.zeros(1)
    return np.asfortranarray(X), np.asfortranarray(Y), coord, idx, r


SMALL_N = [1, 37, 64, 65, 256, 257, 30000]
SMALL_M = [1, 2, 45, 64, 65, 300, 1024]
LARGE = [(TRIP, 8), (TRIP, 45), (TRIP + 321, 8), (TRIP + 321, 45)]


def cases():
    return [(N, M) for N in SMALL_N for M in SMALL_M] + LARGE


_REF = {}


def case_ref(N, M, seed=0, far_nodes=()):
    """The scene of a case and its reference squared minima, computed once per process."""
    k = (N, M, seed, tuple(far_nodes))
    if k not in _REF:
        s = scene(N, M, seed, far_nodes)
        _REF[k] = s + (min_d2(s[0], s[1]),)
    return _REF[k]


def tie_scene():
    """A scene (N = 257, M = 8) whose node 1 lies on the origin of a 2^-26 m grid and its witness on a grid point: the coordinate differences, their
    squares and the sum are exact, so d^2 has no rounding and d = sqrt(d^2) is the one distance the `<= visibility_threshold` test is tied at.
    Returns (X, Y, coord, d)."""
    X, Y, coord, idx, _ = scene(257, 8, seed=11)
    X = np.array(X, order="F"); Y = np.array(Y, order="F")
    g = 2.0 ** -26
    Y[1] = np.round(Y[1] / g) * g
    off = np.array([300001.0, -200003.0, 100007.0])
    X[idx[1]] = Y[1] + off * g
    d2 = float((off * off).sum()) * g * g
    assert d2_fused(Y[1], X[idx[1]]) == d2 and Fraction(d2) == sum(Fraction(int(o)) ** 2 for o in off) * Fraction(g) ** 2
    return X, Y, coord, float(np.sqrt(d2))


def with_non_finite(X, seed=0):
    """X with ten points that have NaN or +-inf coordinates inserted so that THEY land on index_list of the longer cloud.  Returns (cloud, their indices)."""
    rng = np.random.default_rng(991 + seed)
    pat = [(np.nan, 0.3, 0.6), (0.3, np.inf, 0.6), (-np.inf, 0.3, 0.6), (np.nan, np.nan, np.nan), (np.inf, -np.inf, np.nan),
           (0.3, 0.3, -np.inf), (np.inf, np.inf, np.inf), (0.3, np.nan, 0.6), (-np.nan, 0.3, np.inf), (0.3, 0.3, np.nan)]
    N = len(X)
    K = 10
    idx = index_list(N + K)
    idx += [i for i in range(1, N + K) if i not in idx][:K - len(idx)]      # (where the list names fewer than ten distinct indices)
    out = np.empty((N + K, 3))
    keep = np.ones(N + K, dtype=bool); keep[idx] = False
    out[keep] = np.asarray(X)
    out[idx] = np.array([pat[(j + int(rng.integers(10))) % len(pat)] for j in range(K)])
    return np.asfortranarray(out), idx
