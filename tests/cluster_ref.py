"""The statement of "one cloud clustered into F ropes" (include/trackdlo_hip.h, "starting ropes of one colour") in numpy + exact arithmetic, and its scenes.

link(i, j): i != j, both points finite, node_point_d2(X_i, X_j) <= fl(tol tol) in the fused form of assign_ref.d2_fused (one right bit pattern).  A vectorised
pass with plain products decides every pair that is farther than 2^-40 relative from the gate (the plain and the fused sum differ by a few units of 2^-53
relative); every pair nearer to it is decided by the scalar fused form.  Clusters are the connected components over the finite points, found by a plain
breadth-first sweep from every unvisited point in ascending index -- so a component's root, its smallest index, is where its sweep starts; a cluster is kept
if it has at least min_size members; the kept clusters are numbered in ascending order of their root; owner(i) is the number of i's cluster if that is kept
and below F, else -1.

Every scene asserts, on the reference's own output, the property it is named for: a scene cannot quietly stop exercising it."""
import numpy as np

import assign_ref as AR

TILE = 512                 # points of the kernel's LDS tile (csrc/tdlo_cluster_lane.h: kClusterTile)
G = AR.G                   # the 2^-26 lattice of the exact scenes
NEAR = 2.0 ** -40


def links(X, tol, d2=AR.d2_fused, gate="<="):
    """The link graph as a symmetric boolean matrix (the diagonal False).  d2 / gate: the wrong readings test_cluster_ref.py tells from the statement."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = len(X)
    tol2 = float(tol) * float(tol)
    fin = np.isfinite(X).all(axis=1)
    A = np.zeros((n, n), dtype=bool)
    for a in range(0, n, 256):
        with np.errstate(invalid="ignore", over="ignore"):
            d = X[a:a + 256, None, :] - X[None, :, :]
            P = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            blk = (P <= tol2) if gate == "<=" else (P < tol2)
            near = np.abs(P - tol2) <= NEAR * tol2
        for i, j in zip(*np.nonzero(near)):
            if fin[a + i] and fin[j]:
                v = d2(X[a + i], X[j])
                blk[i, j] = (v <= tol2) if gate == "<=" else (v < tol2)
        A[a:a + 256] = blk
    A &= fin[:, None] & fin[None, :]
    A[np.arange(n), np.arange(n)] = False
    assert np.array_equal(A, A.T)
    return A


def components(A, fin, linkage="single"):
    """root [n] (a point that is not finite: itself).  linkage="first": the wrong reading "linked to the cluster's first point"."""
    n = len(A)
    root = np.arange(n)
    seen = ~fin
    for i in range(n):
        if seen[i]:
            continue
        members = np.zeros(n, dtype=bool); members[i] = True
        front = members.copy()
        while front.any():
            front = A[front].any(axis=0) & ~members & ~seen
            members |= front
            if linkage == "first":
                break
        seen |= members
        root[members] = i
    return root


def cluster(X, F, tol, min_size, d2=AR.d2_fused, gate="<=", numbering="root", keep=">=", linkage="single"):
    """The statement: (owner [n] int32, n_clusters, n_each [F], n_unowned, root [n]).  The keywords select the wrong readings."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = len(X)
    fin = np.isfinite(X).all(axis=1)
    root = components(links(X, tol, d2, gate), fin, linkage)
    size = np.bincount(root[fin], minlength=n) if n else np.zeros(0, dtype=np.int64)
    kept = [r for r in range(n) if fin[r] and root[r] == r and (size[r] >= min_size if keep == ">=" else size[r] > min_size)]
    if numbering == "size":
        kept.sort(key=lambda r: (-size[r], r))
    elif numbering == "largest":
        kept.sort(key=lambda r: int(np.nonzero(root == r)[0].max()))
    number = {r: c for c, r in enumerate(kept)}
    owner = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        c = number.get(int(root[i]), -1) if fin[i] else -1
        owner[i] = c if 0 <= c < F else -1
    return owner, len(kept), [int((owner == f).sum()) for f in range(F)], int((owner < 0).sum()), root


def split(X, owner, F):
    return AR.split(X, owner, F)


bits = AR.bits

# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------------
TOL = 0.02
_PHI = 0.6180339887498949


def ropes(n, F, seed=0, length=0.1, gap=0.05):
    """n points on F parallel ropes `gap` apart, point i on rope i mod F -- interleaved point by point, so every cluster crosses every block border -- at a
    low-discrepancy position along it (the largest hole along a rope stays below TOL from 16 points per rope on) with a millimetre of noise."""
    rng = np.random.default_rng(7700 + 31 * seed + n + 5 * F)
    i = np.arange(n)
    s = ((i // F + 1) * _PHI) % 1.0 * length
    X = np.stack([0.1 + s, 0.2 + gap * (i % F), np.full(n, 0.6)], axis=1) + rng.normal(0, 1e-3, (n, 3))
    return np.asfortranarray(X)


def chain(order):
    """1 025 points 0.9 TOL apart on a line: chain position k links to k +- 1 only.  order[k] = the cloud index of chain position k."""
    n = len(order)
    X = np.zeros((n, 3))
    X[np.asarray(order), 0] = np.arange(n) * 0.9 * TOL
    X[:, 1] = 0.3; X[:, 2] = 0.6
    return np.asfortranarray(X)


def _case(X, F, tol=TOL, min_size=1):
    return dict(X=np.asfortranarray(np.asarray(X, dtype=np.float64).reshape(-1, 3)), F=F, tol=tol, min_size=min_size)


def sc_sizes(n, F):
    def make():
        s = _case(ropes(n, F, seed=1), F, min_size=1 if n < 16 * F else 3)
        owner, C, n_each, un, _ = cluster(**s)
        if n >= 16 * F:
            assert C == F and un == 0 and owner[:F].tolist() == list(range(F)) and max(n_each) - min(n_each) <= 1      # rope k is cluster k, all of it
            for b in range(0, n - F + 1, 64):
                assert set(owner[b:b + F].tolist()) == set(range(F))                                                # every cluster in every wave
        else:
            assert C == min(n, F)
        return s
    return make


def sc_chain(kind):
    def make():
        n = 1025
        k = np.arange(n)
        order = {"identity": k, "reversed": n - 1 - k, "stride": (k * 389) % n}[kind]
        assert sorted(order.tolist()) == list(range(n))
        s = _case(chain(order), 2)
        A = links(s["X"], s["tol"])
        assert A.sum() == 2 * (n - 1) and all(A[order[j], order[j + 1]] for j in range(n - 1))      # k links to k +- 1 only
        owner, C, n_each, un, root = cluster(**s)
        assert C == 1 and n_each == [n, 0] and (root == 0).all()
        return s
    return make


def sc_joined_by_first_and_last():
    """Two chains whose only link is the pair (0, n - 1): a triangular tile visit that skips the first tile leaves two clusters."""
    n, m = 1025, 500
    X = np.zeros((n, 3)); X[:, 1] = 0.3; X[:, 2] = 0.6
    X[:m, 0] = -0.9 * TOL * np.arange(m)                       # A: index k at -0.9 TOL k
    X[n - 1, 0] = 0.9 * TOL                                    # B starts at the last index ...
    X[m:n - 1, 0] = 0.9 * TOL * (2 + np.arange(n - 1 - m))     # ... and goes on at m, m + 1, ...
    s = _case(X, 2)
    A = links(s["X"], s["tol"])
    lo = np.zeros(n, dtype=bool); lo[:m] = True
    assert [tuple(p) for p in np.argwhere(A & lo[:, None] & ~lo[None, :])] == [(0, n - 1)]
    assert cluster(**s)[1] == 1 and (n - 1) // TILE == 2
    return s


def sc_joined_across_a_tile_border():
    """Two scrambled chains whose only link is the pair (TILE - 1, TILE)."""
    n = 2 * TILE + 1
    X = np.zeros((n, 3)); X[:, 1] = 0.3; X[:, 2] = 0.6
    k = np.arange(TILE - 1)
    X[k, 0] = -0.9 * TOL * (1 + (k * 37) % (TILE - 1))
    X[TILE - 1, 0] = 0.0
    X[TILE, 0] = 0.9 * TOL
    j = np.arange(TILE)
    X[TILE + 1 + j, 0] = 0.9 * TOL * (2 + (j * 41) % TILE)
    s = _case(X, 2)
    A = links(s["X"], s["tol"])
    lo = np.arange(n) < TILE
    assert [tuple(p) for p in np.argwhere(A & lo[:, None] & ~lo[None, :])] == [(TILE - 1, TILE)]
    assert cluster(**s)[1] == 1
    return s


def sc_gate():
    """tol = 2^-7 on the lattice: points 0 and 1 are EXACTLY fl(tol^2) apart (linked), points 1 and 2 one ulp more (not linked)."""
    tol = 2.0 ** -7
    p0 = AR.lattice([0.3, 0.3, 0.6])
    p1 = p0 + np.array([tol, 0.0, 0.0])
    p2 = p1 + np.array([tol, 2.0 ** -33, 0.0])
    s = _case([p0, p1, p2], 3, tol=tol)
    t2 = tol * tol
    assert AR.d2_fused(p1, p0) == t2 and AR.d2_fused(p2, p1) == np.nextafter(t2, np.inf) and AR.d2_fused(p1, p2) == AR.d2_fused(p2, p1)
    assert cluster(**s)[0].tolist() == [0, 0, 1] and cluster(gate="<", **s)[0].tolist() == [0, 1, 2]
    return s


_FLIP = []


def sc_fused_against_plain():
    """Found by search (seed fixed): two points whose fused distance and plain-product distance are neighbouring doubles with fl(tol^2) on the lower one, so the
    two forms decide the link differently."""
    if not _FLIP:
        rng = np.random.default_rng(20261)
        for _ in range(400000):
            p = rng.uniform(0.2, 0.9, 3); q = p + rng.uniform(-0.01, 0.01, 3)
            f, pl = AR.d2_fused(q, p), AR.d2_plain(q, p)
            if f != pl:
                tol = float(np.sqrt(min(f, pl)))
                if tol * tol == min(f, pl):
                    _FLIP.append((p, q, tol))
                    break
    p, q, tol = _FLIP[0]
    s = _case([p, q], 2, tol=tol)
    assert (AR.d2_fused(q, p) <= tol * tol) != (AR.d2_plain(q, p) <= tol * tol)
    assert cluster(**s)[1] != cluster(d2=AR.d2_plain, **s)[1]
    return s


def _blob(centre, k, rng):
    return np.asarray(centre) + rng.normal(0, 1e-3, (k, 3))


def sc_noise_around_min_size():
    """min_size = 5: a blob of 4 points (dropped), a blob of 5 (kept, root 1) and a rope of 40 (kept, root 2), interleaved; the blob of 5 is cluster 0 though it
    is the smaller one, and the dropped blob holds index 0."""
    rng = np.random.default_rng(5)
    parts = [_blob([0.1, 0.9, 0.6], 4, rng), _blob([0.5, 0.9, 0.6], 5, rng), ropes(40, 1, seed=2)]
    X = np.concatenate(parts); lab = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    perm = np.argsort(np.concatenate([np.arange(len(p)) * 3 + k for k, p in enumerate(parts)]), kind="stable")      # 0 1 2 0 1 2 ... then the rope's rest
    s = _case(X[perm], 2, min_size=5)
    lab = lab[perm]
    owner, C, n_each, un, _ = cluster(**s)
    assert lab[:3].tolist() == [0, 1, 2] and C == 2 and n_each == [5, 40] and un == 4 and (owner[lab == 0] == -1).all()
    assert cluster(keep=">", **s)[2] == [40, 0] and cluster(numbering="size", **s)[2] == [40, 5]
    return s


def sc_isolated_points_more_clusters_than_destinations():
    """min_size = 1, two ropes and five isolated points of which one is index 0: C = 7 > F = 2; cluster 0 is the isolated point, cluster 1 a rope, the rest -1."""
    rng = np.random.default_rng(6)
    X = ropes(80, 2, seed=3)
    iso = np.array([[1.0 + 0.1 * k, 0.9, 0.6] for k in range(5)])
    X = np.insert(X, [0, 7, 20, 41, 80], iso, axis=0)
    s = _case(X, 2, min_size=1)
    owner, C, n_each, un, _ = cluster(**s)
    assert C == 7 and n_each == [1, 40] and un == 44 and owner[0] == 0
    return s


def sc_fewer_clusters_than_destinations():
    s = _case(ropes(130, 2, seed=4), 4, min_size=2)
    owner, C, n_each, un, _ = cluster(**s)
    assert C == 2 and n_each == [65, 65, 0, 0] and un == 0
    return s


def sc_numbering():
    """Cluster A holds the indices 0 and n - 1, cluster B the index 1 and is the larger one: by root A, B; by size B, A; by largest member B, A."""
    a, b = ropes(20, 1, seed=5), ropes(40, 1, seed=6) + np.array([0.0, 0.3, 0.0])
    X = np.concatenate([a[:1], b, a[1:]])
    s = _case(X, 2, min_size=2)
    assert cluster(**s)[2] == [20, 40] and cluster(numbering="size", **s)[2] == [40, 20] and cluster(numbering="largest", **s)[2] == [40, 20]
    return s


def sc_non_finite():
    """NaN, +inf and -inf coordinates interleaved, index 0 among them: they link nothing and nobody owns them; the ropes stay whole around them."""
    X = np.array(ropes(300, 2, seed=7), order="F")
    bad = [0, 63, 64, 150, 255, 256, 299]
    pat = [(np.nan, 0.3, 0.6), (0.3, np.inf, 0.6), (-np.inf, 0.3, 0.6), (np.nan, np.nan, np.nan), (0.15, 0.2, np.inf), (np.inf, -np.inf, np.nan), (0.15, np.nan, 0.6)]
    for k, i in enumerate(bad):
        X[i] = pat[k]
    s = _case(X, 2, min_size=1)
    owner, C, n_each, un, _ = cluster(**s)
    assert C == 2 and un == len(bad) and (owner[bad] == -1).all() and sum(n_each) == 300 - len(bad) and owner[1] == 0 and owner[2] == 1
    return s


def sc_duplicates():
    X = np.array(ropes(257, 3, seed=8), order="F")
    X[100:160] = X[10:70]
    X[256] = X[0]
    s = _case(X, 3, min_size=3)
    assert cluster(**s)[1] == 3 and len(np.unique(X, axis=0)) < 200
    return s


def sc_signed_zeros():
    """-0.0 against 0.0: the distance is 0, the bits are copied."""
    X = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.0, 0.001], [0.5, 0.0, -0.0]])
    s = _case(X, 2, min_size=1)
    owner, C, n_each, un, _ = cluster(**s)
    assert owner.tolist() == [0, 0, 0, 1] and np.signbit(split(s["X"], owner, 2)[0]).sum() == 5
    return s


def sc_one_destination():
    s = _case(ropes(257, 2, seed=9), 1, min_size=3)
    owner, C, n_each, un, _ = cluster(**s)
    assert C == 2 and n_each == [129] and un == 128
    return s


SIZES = [1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE + 1, 2 * TILE + 1]
SCENES = {}
for _n in SIZES:
    for _F in (2, 3):
        SCENES[f"ropes{_F}_n{_n}"] = sc_sizes(_n, _F)
for _k in ("identity", "reversed", "stride"):
    SCENES[f"chain_{_k}"] = sc_chain(_k)
SCENES.update(first_and_last=sc_joined_by_first_and_last, tile_border=sc_joined_across_a_tile_border, gate=sc_gate, fused=sc_fused_against_plain,
              noise=sc_noise_around_min_size, isolated=sc_isolated_points_more_clusters_than_destinations, few=sc_fewer_clusters_than_destinations,
              numbering=sc_numbering, non_finite=sc_non_finite, duplicates=sc_duplicates, zeros=sc_signed_zeros, one_destination=sc_one_destination)

_DONE = {}


def scene(name):
    """(the scene's arguments, the statement's output), computed once per process and left unchanged."""
    if name not in _DONE:
        s = SCENES[name]()
        _DONE[name] = (s, cluster(**s))
    return _DONE[name]
