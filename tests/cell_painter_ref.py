"""The painter test over a cell of ropes, stated in numpy and Python integers from include/trackdlo_hip.h ("ropes that hide one another") -- not from the lane.
Steps 1 and 2 and the key are rig_painter_ref's (float64, ONE operation per expression); the order is a sort on (key, flat edge index); coverage is exact
integer arithmetic (rig_painter_ref.covers).  For speed the "before" filter and a pixel bounding-box reject run in numpy int64 over blocks of nodes, and
`covers` is called on the survivors alone: a covered pixel lies within w / 2 of a point of the segment, hence within w / 2 of the box of its end pixels.

A cell here is (ropes, cams, mats, w): ropes a list of (Y [M x 3], node_dist [M], threshold); cams a list of (fx, fy, cx, cy); mats None or a list with a
3 x 4 array or None per camera.
`variant` names a WRONG reading of the statement, for the tests that tell the readings apart:
  "phantom_edge"  an edge between the last node of rope f and the first node of rope f + 1
  "own_only"      only a rope's own edges hide its nodes (F single tests)
  "local_tie"     equal keys are broken by the rope-local edge index instead of the flat index
  "any_first"     first is taken over every painted edge that covers the node, not over the incident edges
  "no_order"      a covering edge hides the node wherever it stands in the order"""
import numpy as np

from rig_painter_ref import cam_node, pixel, edge_key, covers, words

BLOCK = 256


def camera_verdict(Yflat, rope_of, local, cam, T, rows, cols, w, variant=None):
    """One camera over the N flat nodes: dict with drawable / seen / hidden [N] bools, edges (flat index -> painted?), rank (painted flat edge -> place in the
    order), first [N] (a place; the number of painted edges for "after every painted edge"), px [N], survivors (pairs `covers` was asked about)."""
    N = len(Yflat)
    q = [cam_node(T, Yflat[n]) for n in range(N)]
    px = [pixel(cam, q[n], rows, cols) for n in range(N)]
    drawable = [p[0] for p in px]
    seen = [p[1] for p in px]
    is_edge = [n + 1 < N and (rope_of[n + 1] == rope_of[n] or variant == "phantom_edge") for n in range(N)]
    painted = {e: bool(drawable[e] and drawable[e + 1]) for e in range(N) if is_edge[e]}
    keys = {e: edge_key(q[e], q[e + 1]) for e in painted if painted[e]}
    ranked = sorted(keys, key=(lambda e: (float(keys[e]), local[e], rope_of[e])) if variant == "local_tie" else (lambda e: (float(keys[e]), e)))
    P = len(ranked)
    rank = {e: r for r, e in enumerate(ranked)}
    pc = np.array([p[2] for p in px], dtype=np.int64); pr = np.array([p[3] for p in px], dtype=np.int64)
    # the painted edges as arrays, in the order
    ea = np.array(ranked, dtype=np.int64)
    e_rope = np.array([rope_of[e] for e in ranked], dtype=np.int64)
    if P:
        ac, ar, bc, br = pc[ea], pr[ea], pc[ea + 1], pr[ea + 1]
        c0, c1, r0, r1 = np.minimum(ac, bc), np.maximum(ac, bc), np.minimum(ar, br), np.maximum(ar, br)
    first = []
    for n in range(N):
        inc = [rank[e] for e in (n - 1, n) if e >= 0 and painted.get(e) and (rope_of[e] == rope_of[n] or variant == "phantom_edge")]
        first.append(min(inc) if inc else P)
    hidden = [False] * N
    survivors = 0
    fa = np.array(first, dtype=np.int64)
    for b0 in range(0, N if P else 0, BLOCK):
        ns = np.array([n for n in range(b0, min(N, b0 + BLOCK)) if drawable[n]], dtype=np.int64)
        if not len(ns):
            continue
        nc, nr = pc[ns][:, None], pr[ns][:, None]
        box = (2 * (c0[None, :] - nc) <= w) & (2 * (nc - c1[None, :]) <= w) & (2 * (r0[None, :] - nr) <= w) & (2 * (nr - r1[None, :]) <= w)
        if variant in ("any_first", "no_order"):
            mask = box
        else:
            mask = box & (np.arange(P, dtype=np.int64)[None, :] < fa[ns][:, None])          # strictly before first
        if variant == "own_only":
            mask &= e_rope[None, :] == np.array([rope_of[n] for n in ns], dtype=np.int64)[:, None]
        ii, jj = np.nonzero(mask)
        survivors += len(ii)
        cover = {}
        for i, j in zip(ii.tolist(), jj.tolist()):                                          # (jj ascends within a node: the order's places)
            n, e = int(ns[i]), int(ea[j])
            if variant != "any_first" and hidden[n]:
                continue
            if covers((int(pc[n]), int(pr[n])), (int(pc[e]), int(pr[e])), (int(pc[e + 1]), int(pr[e + 1])), w):
                if variant == "any_first":
                    cover.setdefault(n, []).append(j)
                else:
                    hidden[n] = True
        for n, places in cover.items():                                                     # the wrong reading: first over the covering edges
            first[n] = min(places)
            hidden[n] = any(j < first[n] for j in places)
    return dict(drawable=drawable, seen=seen, hidden=hidden, painted=painted, keys=keys, rank=rank, first=first, px=[p[2:] for p in px], n_painted=P,
                survivors=survivors)


def flatten(ropes):
    """(Yflat [N x 3], rope_of [N], local [N], off [F + 1])."""
    Ys = [np.asarray(r[0], dtype=np.float64).reshape(-1, 3) for r in ropes]
    off = np.concatenate(([0], np.cumsum([len(Y) for Y in Ys]))).astype(int)
    rope_of = [f for f, Y in enumerate(Ys) for _ in range(len(Y))]
    local = [m for Y in Ys for m in range(len(Y))]
    return (np.concatenate(Ys) if Ys else np.zeros((0, 3))), rope_of, local, off


def cell_verdict(ropes, cams, mats, rows, cols, w, variant=None):
    """The cell's verdict: ([visible rope-local indices int32 ascending per rope], seen words [K x W], hidden words [K x W], the per-camera dicts)."""
    Yflat, rope_of, local, off = flatten(ropes)
    K = len(cams)
    per = [camera_verdict(Yflat, rope_of, local, cams[k], None if mats is None else mats[k], rows, cols, w, variant) for k in range(K)]
    vis = []
    for f, (Y, dist, thr) in enumerate(ropes):
        v = []
        for m in range(len(np.asarray(Y).reshape(-1, 3))):
            if not dist[m] <= thr:                 # (NaN fails)
                continue
            n = off[f] + m
            if any(c["seen"][n] and not c["hidden"][n] for c in per):
                v.append(m)
        vis.append(np.array(v, dtype=np.int32))
    seen = np.stack([words(c["seen"]) for c in per])
    hidden = np.stack([words(c["hidden"]) for c in per])
    return vis, seen, hidden, per
