"""Constructed scenes for the one-launch EM loop (k_iter_fused, k_iter_fused_w0) -- test infrastructure, numpy only.

Every builder has fixed seeds and returns dict(X, Y0, sigma2_in, kw, priors, claim): the cloud, the nodes, the sigma2 handed in, the parameters (the launch
file's, synth.LAUNCH_PARAMS, unless the scene says otherwise), the correspondence priors or None, and the claim the scene is built for, in words.  Every scene is
eligible for the one-launch loop: fp32 mode, no LLE term, no visibility term.  tests/test_fused_scenes_ref.py proves the claims on the CPU (numpy and the
oracle alone); tests/test_fused_loop_edges_gpu.py runs the scenes on the three routes.

  a  dark        a run of nodes that no point's membership reaches, across the middle junction of the chain's carve
  b  coincident  two nodes in one place: an identity link, G singular
  c  priors      a prior on every junction node, two on one node, one on a dark node
  d  start       nodes 2 cm beside the rope, sigma2 from the set-up
  e  decades     the first quarter of the chain seen by a handful of points, the rest by thousands
  f  small       clouds of 1 .. 257 points
  g  lengths     every chain length of the route, and the one below it
"""
import numpy as np

from chain_numpy import carve
from trackdlo_amd import synth

CHAINS = (13, 50, 61, 64)          # the shortest chain with an unrolled trip; the headline's; the longest on k_iter_fused_w0; k_iter_fused, second sum element per thread
ITERS = tuple(range(1, 9))         # the iteration counts the GPU suite runs every scene of a .. e with
SMALL_N = (1, 7, 37, 63, 64, 65, 255, 256, 257)
SMALL_M = (8, 50)
LENGTHS = tuple(range(8, 65))
REFUSED_M = 7
WINDOW_BITS, DARK_BITS = -36.0, -60.0       # the E-step's window (a membership ratio below 2^-36 is dropped); what this file calls dark

# scene a: (points drawn, occluded arc).  13 nodes: with (0.4, 0.6) node 6 alone is dark -- the quarter of the rope around it is taken out instead.
_DARK = {13: (700, (0.25, 0.75)), 50: (700, (0.4, 0.6)), 61: (3000, (0.4, 0.6)), 64: (3000, (0.4, 0.6))}
# scene e: (points drawn, points left to the first quarter of the chain)
_DECADES = {13: (2000, 3), 50: (4000, 5), 61: (4000, 5), 64: (4000, 5)}
START_SHIFT = 0.02
LADDER_M, LADDER_MARGIN, LADDER_RUNGS = 13, 4e-5, 6


def base_kw(**over):
    P = synth.LAUNCH_PARAMS
    kw = dict(beta=P["beta"], lambda_=P["lambda_"], lle_weight=P["lle_weight"], mu=P["mu"], max_iter=30, tol=0.0, include_lle=False, alpha=0.0, k_vis=0.0,
              visibility_threshold=P["visibility_threshold"])
    kw.update(over)
    return kw


def dark_nodes(X, Y, sigma2):
    """Nodes m with -(d2(n, m) - min_m' d2(n, m')) / (2 sigma2 ln 2) < DARK_BITS for EVERY point n: each point's membership of m is below 2^-60 of its
    largest one, far outside the E-step's window of 2^-36."""
    X = np.asarray(X, dtype=np.float64); Y = np.asarray(Y, dtype=np.float64)
    d2 = ((X[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    bits = -(d2 - d2.min(axis=1, keepdims=True)) / (2.0 * sigma2 * np.log(2.0))
    return np.nonzero((bits < DARK_BITS).all(axis=0))[0]


def longest_run_through(nodes, through):
    """Length of the run of consecutive integers in `nodes` that contains `through` (0: it is not in there)."""
    s = set(int(v) for v in nodes)
    if through not in s:
        return 0
    lo = hi = through
    while lo - 1 in s:
        lo -= 1
    while hi + 1 in s:
        hi += 1
    return hi - lo + 1


def _scene(X, Y0, sigma2_in, kw, priors, claim):
    return dict(X=np.asfortranarray(X), Y0=np.asfortranarray(Y0), sigma2_in=float(sigma2_in), kw=kw, priors=priors, claim=claim)


def dark(M):
    N, occ = _DARK[M]
    X, Y0, _ = synth.scene(N, M, config=2, occlude=occ)
    return _scene(X, Y0, 1e-5, base_kw(), None,
                  f"at least three consecutive dark nodes lie across the junction j2 = {carve(M)[1]} (arc {occ} of the rope is not seen, sigma2 = 1e-5)")


def coincident(M):
    X, Y0, _ = synth.scene(700, M, config=2)
    Y0 = Y0.copy(order="F")
    Y0[M // 3 + 1] = Y0[M // 3]
    return _scene(X, Y0, 0.0, base_kw(), None, f"nodes {M // 3} and {M // 3 + 1} coincide: the link between them is the identity and G is singular")


def prior_nodes(M):
    j1, j2, j3 = carve(M)[:3]
    return dict(junctions=[0, j1, j2 - 1, j2, j3, M - 1], twice=2, dark=j2 + 1)


def priors(M):
    """On the cloud of scene a.  Rows (node, x, y, z); the two rows of node `twice` are the last two of the array's first eight, the second one wins."""
    sc = dark(M)
    Y0 = sc["Y0"]
    pn = prior_nodes(M)
    rng = np.random.default_rng(synth.BASE_SEED + 77 * M)
    rows = [[m, *(Y0[m] + rng.uniform(-0.004, 0.004, size=3))] for m in pn["junctions"]]
    rows.append([pn["twice"], *(Y0[pn["twice"]] + np.array([0.006, -0.006, 0.004]))])
    rows.append([pn["twice"], *(Y0[pn["twice"]] + np.array([-0.003, 0.005, -0.002]))])
    rows.append([pn["dark"], *(Y0[pn["dark"]] + np.array([0.0, 0.004, 0.003]))])
    return _scene(sc["X"], Y0, sc["sigma2_in"], base_kw(alpha=synth.LAUNCH_PARAMS["alpha"]), np.array(rows, dtype=np.float64),
                  f"a prior on each junction node {pn['junctions']}, two on node {pn['twice']} (the last one wins), one on the dark node {pn['dark']}")


def start(M, N=700):
    X, Y0, _ = synth.scene(N, M, config=2)
    Y0 = np.asfortranarray(Y0 + np.array([0.0, START_SHIFT, 0.0]))
    return _scene(X, Y0, 0.0, base_kw(), None, "the nodes start 2 cm beside the rope with the set-up's sigma2: large first steps, the whole chain in the window")


def decades(M):
    N, handful = _DECADES[M]
    X, Y0, _ = synth.scene(N, M, config=2)
    near = ((X[:, None, :] - Y0[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
    first = np.nonzero(near < M // 4)[0]
    keep = np.ones(len(X), dtype=bool)
    keep[first] = False
    keep[first[:: max(1, len(first) // handful)][:handful]] = True
    return _scene(X[keep], Y0, 1e-5, base_kw(), None,
                  f"nodes 0 .. {M // 4 - 1} are the nearest node of {handful} points, the others of thousands: P1 spans many decades on one chain")


def small(M, N):
    X, Y0, _ = synth.scene(N, M, config=2)
    return _scene(X, Y0, 0.0, base_kw(), None, f"a cloud of {N} point(s) on {M} nodes")


def length(M, N=700):
    X, Y0, _ = synth.scene(N, M, config=2)
    return _scene(X, Y0, 0.0, base_kw(), None, f"{M} nodes" + (": below the one-launch loop's shortest chain" if M == REFUSED_M else ""))


HARD = dict(dark=dark, coincident=coincident, priors=priors, start=start, decades=decades)


def w0_priors(Y0):
    """The three priors of tests/test_fused_w0_gpu.py."""
    M = len(Y0)
    return np.array([[1, *(Y0[1] + [0.004, -0.003, 0.002])], [M - 3, *(Y0[M - 3] + [-0.002, 0.005, 0.001])], [M // 2, *Y0[M // 2]]])


def crits(Y0, trace_Y):
    """crit_k = mean_i |Y_k[i] - Y_{k-1}[i]|, k = 1 ..: the stopping rule's quantity (trackdlo.cpp:424; conv_rule == 0 of oracle/ref_cpu.c)."""
    Ys = np.concatenate([np.asarray(Y0)[None], np.asarray(trace_Y)])
    return np.linalg.norm(np.diff(Ys, axis=0), axis=2).mean(axis=1)


def exit_ladder(crit, margin=LADDER_MARGIN):
    """[(k, tol_k)] for as many consecutive k from 1 as qualify: tol_k midway between crit_{k-1} and crit_k (crit_0: the first step doubled -- nothing
    precedes the first iteration), with crit_j >= tol_k + margin for every j < k and crit_k <= tol_k - margin.  A registration run with tol_k ends after
    exactly k iterations, and no other trajectory within `margin` of this one in the mean displacement ends elsewhere."""
    out = []
    for k in range(1, len(crit) + 1):
        prev = crit[k - 2] if k >= 2 else 2.0 * crit[0]
        tol = 0.5 * (prev + crit[k - 1])
        if not (all(c >= tol + margin for c in crit[:k - 1]) and crit[k - 1] <= tol - margin):
            break
        out.append((k, float(tol)))
    return out
