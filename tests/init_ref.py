"""The rule of `sort_pts` (trackdlo/src/utils.cpp:95-170) stated in numpy, the chain coordinate behind it, and the scenes the tests hold
k_sort_pts (csrc/tdlo_init.hip) and its host twin (csrc/tdlo_host.cpp, sort_pts_host) to.

The statement keeps the reference's shape: the matrix G of squared distances -- fp64, (dx dx + dy dy) + dz dz, every product and sum rounded --,
the scan of every round over a (selected) ascending, then b (unselected) ascending, with the strict `minimum > G(a, b)` and `G != 0`, and the
list with its reverse / reverse_on / insertion_counter / last_visited_b bookkeeping (:134-157).  `statement_literal` is the triple loop as it
stands (chains of up to a few dozen nodes: it is cubic in python); `statement` replaces the two inner loops of a round by the first minimum, in
row-major order, of the matrix masked to (selected row, unselected column, non-zero) -- the same pair by construction, and
tests/test_init_ref.py holds the two to each other on every scene the literal form can afford.  The reference finds rows in its list BY VALUE;
the scenes' nodes are pairwise distinct, so that is by index (two equal nodes are an error of the library: status 2).

A statement returns dict(status, perm, Y, coord, rounds=[(a, b)], reverse=[value after each round], ties=[pairs attaining the minimum]):
status 0, or 1 a non-finite coordinate, 2 two equal nodes (as values: -0.0 == 0.0), 3 a round without an edge (the reference would take a = b = 0
there and repeat node 0).  coord[0] = 0, coord[i] = coord[i - 1] + sqrt((dx dx + dy dy) + dz dz) of consecutive sorted nodes, added serially
(trackdlo_node.cpp:135-141, tracking_test.py:531-537).

variant (the sharpness tests: each must change the result of some scene): 'largest_parent' ties go to the largest a; 'counter_off' the
insertion counter starts one too far; 'zero_edge' a zero distance is an edge."""
import numpy as np


def dist2_matrix(Y):
    Y = np.asarray(Y, dtype=np.float64)
    with np.errstate(all="ignore"):
        dx = Y[:, 0][:, None] - Y[:, 0][None, :]; dy = Y[:, 1][:, None] - Y[:, 1][None, :]; dz = Y[:, 2][:, None] - Y[:, 2][None, :]
        return (dx * dx + dy * dy) + dz * dz


def chain_coord(Ys):
    d = np.diff(np.asarray(Ys, dtype=np.float64), axis=0)
    seg = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    out = np.zeros(len(Ys)); cur = 0.0
    for i in range(1, len(Ys)):
        cur = cur + seg[i - 1]
        out[i] = cur
    return out


def precheck(Y):
    Y = np.asarray(Y, dtype=np.float64)
    if not np.isfinite(Y).all():
        return 1
    eq = (Y[:, None, :] == Y[None, :, :]).all(axis=2)
    return 2 if (eq.sum() > len(Y)) else 0


class _List:
    """The list of :134-157, as indices into Y_0."""

    def __init__(self, variant):
        self.rows = []; self.reverse = 0; self.reverse_on = 0; self.insertion_counter = 0; self.last_visited_b = 0; self.variant = variant

    def take(self, counter, a, b):
        if counter == 0:
            self.rows.append(a); self.rows.append(b)
        else:
            if self.last_visited_b != a:
                self.reverse += 1; self.reverse_on = a
                self.insertion_counter = 2 if self.variant == "counter_off" else 1
            if self.reverse % 2 == 1:
                self.rows.insert(self.rows.index(a), b)
            elif self.reverse != 0:
                self.rows.insert(self.rows.index(self.reverse_on) + self.insertion_counter, b)
                self.insertion_counter += 1
            else:
                self.rows.append(b)
        self.last_visited_b = b


def _result(Y, status, lst=None, rounds=(), reverse=(), ties=()):
    if status:
        return dict(status=status, perm=None, Y=None, coord=None, rounds=list(rounds), reverse=list(reverse), ties=list(ties))
    perm = np.array(lst.rows, dtype=np.int32)
    Ys = np.asarray(Y, dtype=np.float64)[perm]
    return dict(status=0, perm=perm, Y=Ys, coord=chain_coord(Ys), rounds=list(rounds), reverse=list(reverse), ties=list(ties))


def statement_literal(Y, variant=None):
    Y = np.asarray(Y, dtype=np.float64); N = len(Y)
    st = precheck(Y)
    if st:
        return _result(Y, st)
    G = dist2_matrix(Y).tolist()
    selected = [False] * N; selected[0] = True
    lst = _List(variant); rounds = []; reverse = []
    scan = range(N - 1, -1, -1) if variant == "largest_parent" else range(N)
    counter = 0
    while counter < N - 1:
        minimum = float("inf"); a = 0; b = 0; found = False
        for m in scan:
            if selected[m]:
                for n in range(N):
                    if (not selected[n]) and (G[m][n] != 0.0 or variant == "zero_edge"):
                        if minimum > G[m][n]:
                            minimum = G[m][n]; a = m; b = n; found = True
        if not found:
            return _result(Y, 3, rounds=rounds, reverse=reverse)
        lst.take(counter, a, b)
        rounds.append((a, b)); reverse.append(lst.reverse)
        selected[b] = True
        counter += 1
    return _result(Y, 0, lst, rounds, reverse)


def statement(Y, variant=None):
    Y = np.asarray(Y, dtype=np.float64); N = len(Y)
    st = precheck(Y)
    if st:
        return _result(Y, st)
    G = dist2_matrix(Y)
    inf = np.inf
    edge = np.ones_like(G, dtype=bool) if variant == "zero_edge" else (G != 0.0)
    np.fill_diagonal(edge, False)
    W = np.full((N, N), inf)                                       # W[a, b] = G[a, b] where a is selected, b is not and (a, b) is an edge
    selected = np.zeros(N, dtype=bool)

    def select(a):
        selected[a] = True
        W[:, a] = inf
        W[a, :] = np.where(edge[a] & ~selected, G[a], inf)
    select(0)
    lst = _List(variant); rounds = []; reverse = []; ties = []
    for counter in range(N - 1):
        k = int(np.argmin(W))                                      # the first minimum in row-major order: a ascending, then b ascending
        a, b = divmod(k, N)
        minimum = W[a, b]
        if not minimum < inf:
            return _result(Y, 3, rounds=rounds, reverse=reverse, ties=ties)
        hits = np.flatnonzero(W.ravel() == minimum)
        if variant == "largest_parent":                            # the largest a attaining the minimum, its smallest b
            a = int(hits[-1] // N); b = int(hits[hits // N == a][0] % N)
        lst.take(counter, a, b)
        rounds.append((a, b)); reverse.append(lst.reverse); ties.append(int(hits.size))
        select(b)
    return _result(Y, 0, lst, rounds, reverse, ties)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
def _curve(M, seed, jitter=0.1):
    """M nodes along a gentle helix, about 2 cm apart, each moved along the curve by up to `jitter` of the spacing and off it by a tenth of a millimetre.
    The tree then follows the rope: a scene's chain order is the rope's own order, or its reverse (tests/test_init_ref.py)."""
    rng = np.random.default_rng(seed)
    s = (np.arange(M) + jitter * rng.uniform(-1, 1, M)) * 0.02
    turn = max(M * 0.02 / 3.0, 0.3)                                # three turns at most: the helix's pitch keeps the turns a decimetre or more apart
    r = turn / (2 * np.pi) * 0.8
    Y = np.stack([r * np.cos(2 * np.pi * s / turn), r * np.sin(2 * np.pi * s / turn), 0.6 + 0.6 * s], axis=1)
    return Y + 1e-4 * rng.standard_normal((M, 3))


def _shuffled(Y, first, seed):
    """Rows of Y in a random order with row `first` in front.  Returns (nodes, rank): rank[i] = place along the curve of node i."""
    rng = np.random.default_rng(seed)
    rest = np.array([i for i in range(len(Y)) if i != first])
    rng.shuffle(rest)
    order = np.concatenate([[first], rest]).astype(int)
    return np.ascontiguousarray(Y[order]), order


def rope_end_first(M=24, seed=1):
    return _shuffled(_curve(M, seed), 0, seed + 100)


def rope_middle_first(M=24, seed=2):
    return _shuffled(_curve(M, seed), M // 2, seed + 100)


def u_shape(M=31, seed=3):
    """A U bent until its ends nearly meet: M nodes about 2 cm apart on a circle that closes except for a gap of 1.5 cm between the rope's two ends.  Node 0
    sits a quarter of the way along, and the links grow with their distance from it -- 20.0, 20.4, 20.8 ... mm on one side, 20.2, 20.6 ... mm on the other --
    so the tree's two tips take turns (`reverse` goes up in every round) until the short side reaches the rope's end, crosses the gap and runs on
    along the far end of the other side."""
    k0 = M // 4
    link = np.zeros(M - 1)                                          # link[i] joins nodes i and i + 1 of the rope
    for j in range(M - 1 - k0):
        link[k0 + j] = 0.0200 + 0.0004 * j
    for j in range(k0):
        link[k0 - 1 - j] = 0.0202 + 0.0004 * j
    arc = 0.0075 + np.concatenate([[0.0], np.cumsum(link)])
    R = (arc[-1] + 0.0075) / (2 * np.pi)
    Y = np.stack([R * np.cos(arc / R), R * np.sin(arc / R), np.full(M, 0.5)], axis=1)
    return _shuffled(Y, k0, seed + 100)


def lattice(seed=4):
    g = np.arange(4) * 0.03125                                      # spacings and sums exact in binary: equal distances are EQUAL doubles
    Y = np.array([[x, y, z + 0.5] for x in g for y in g for z in g])
    return _shuffled(Y, 21, seed + 100)


def one_ulp(seed=5):
    Y = _curve(12, seed)
    twin = Y[7].copy(); twin[0] = np.nextafter(twin[0], np.inf)
    return _shuffled(np.concatenate([Y, [twin]]), 3, seed + 100)


def signed_zero(seed=6):
    """Nodes on the plane x = 0, half of them written -0.0: distinct nodes whose x are equal as values and differ as bits."""
    Y = _curve(10, seed); Y[:, 0] = 0.0; Y[::2, 0] = -0.0
    return _shuffled(Y, 0, seed + 100)


def underflow():
    """Distinct nodes with a zero distance between two of them (1e-170 squared is below the smallest double): never an edge, though the smallest."""
    return np.array([[0.0, 0.0, 0.0], [1e-170, 0.0, 0.0], [1.0, 0.0, 0.0], [3.0, 0.0, 0.0]]), np.arange(4)


SIZES = [2, 3, 63, 64, 65, 256, 257, 890, 1024]


def scenes():
    """name -> nodes [M x 3].  Built once per process."""
    if not _SCENES:
        for name, fn in (("end_first", rope_end_first), ("middle_first", rope_middle_first), ("u_shape", u_shape), ("lattice", lattice),
                         ("one_ulp", one_ulp), ("signed_zero", signed_zero), ("underflow", underflow)):
            _SCENES[name] = fn()[0]
        for M in SIZES:
            _SCENES[f"rope{M}"] = _shuffled(_curve(M, 40 + M), (M * 5) // 7 if M > 3 else 0, 200 + M)[0]
    return _SCENES


def small_scene_names():
    return [n for n, Y in scenes().items() if len(Y) <= 65]


def error_inputs():
    """name -> (nodes, status)."""
    Y = _curve(9, 8)
    nan = Y.copy(); nan[4, 1] = np.nan
    inf = Y.copy(); inf[8, 2] = -np.inf
    dup = Y.copy(); dup[6] = dup[2]
    zdup = Y.copy(); zdup[:, 0] = 0.0; zdup[5] = zdup[1]; zdup[5, 0] = -0.0       # equal as values, not as bits
    both = dup.copy(); both[0, 0] = np.nan                                         # the non-finite coordinate is reported first
    tiny = np.array([[0.0, 0.0, 0.0], [1e-170, 0.0, 0.0]])                          # the only distance underflows: no edge
    huge = np.array([[1e200, 0.0, 0.0], [-1e200, 0.0, 0.0], [0.0, 1e200, 0.0]])     # every distance overflows: `INFINITY > G` never holds
    big = _curve(70, 9); big[69] = big[0]                                          # the workgroup form
    return dict(nan=(nan, 1), inf=(inf, 1), dup=(dup, 2), zdup=(zdup, 2), both=(both, 1), tiny=(tiny, 3), huge=(huge, 3), big_dup=(big, 2))


_SCENES = {}
_REF = {}


def ref(name):
    """statement() of a scene, computed once per process and shared."""
    if name not in _REF:
        _REF[name] = statement(scenes()[name])
    return _REF[name]


def rope_cloud(N, seed, length=0.9):
    """A synthetic rope for the composed call: N points within 2 mm of a planar S-curve about `length` metres long, near the origin (reg starts its
    centroids on a segment of the y axis)."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 1, N)
    X = np.stack([0.15 * np.sin(2 * np.pi * s), length * (s - 0.5) * 0.8, 0.05 * np.cos(np.pi * s)], axis=1)
    return np.asfortranarray(X + 0.002 * rng.standard_normal((N, 3)))
