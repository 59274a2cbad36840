"""The self-occlusion test under a rig, stated in numpy and Python integers from include/trackdlo_hip.h ("self-occlusion under a rig") -- not from the lane.
Steps 1 - 3 are float64 with ONE operation per expression, so nothing can fuse; ranks are a sort on (key, index); coverage is exact integer arithmetic.

A rig here is (cams, mats): cams a list of (fx, fy, cx, cy), mats None or a list with a 3 x 4 array or None per camera.  Y is [M x 3].
`variant` names a WRONG reading of the statement, for the tests that tell the readings apart: "no_image" (seen = drawable), "any" (hidden in ANY camera that
sees the node), "rig_keys" (keys from the rig-frame nodes), "all_edges" (ranks over all edges, painted or not), "fused" (the transform with fused multiply-adds)."""
from fractions import Fraction

import numpy as np

f64 = np.float64


def _fma(a, b, c):
    """a * b + c rounded once, exactly (finite inputs)."""
    return f64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def cam_node(T, p, fused=False):
    """Step 1: ((A0 x + A1 y) + A2 z) + b per row, every product and sum rounded on its own."""
    if T is None:
        return [f64(p[0]), f64(p[1]), f64(p[2])]
    T = np.asarray(T, dtype=f64).reshape(3, 4)
    out = []
    with np.errstate(all="ignore"):
        for r in range(3):
            if fused:
                s = f64(T[r, 0]) * f64(p[0])
                s = _fma(T[r, 1], p[1], s)
                s = _fma(T[r, 2], p[2], s)
                s = s + f64(T[r, 3])
            else:
                a = f64(T[r, 0]) * f64(p[0])
                b = f64(T[r, 1]) * f64(p[1])
                s = a + b
                c = f64(T[r, 2]) * f64(p[2])
                s = s + c
                s = s + f64(T[r, 3])
            out.append(f64(s))
    return out


def pixel(cam, q, rows, cols):
    """Step 2: (drawable, seen, c, r)."""
    fx, fy, cx, cy = (f64(v) for v in cam)
    xc, yc, zc = q
    if not zc > 0:
        return False, False, 0, 0
    with np.errstate(all="ignore"):
        a = fx * xc
        b = cx * zc
        u = a + b
        a = fy * yc
        b = cy * zc
        v = a + b
        qc = u / zc
        qr = v / zc
    if not (qc > -8193.0 and qc < 8192.0 and qr > -8193.0 and qr < 8192.0):
        return False, False, 0, 0
    c, r = int(qc), int(qr)                       # truncation toward zero, like a C cast
    return True, (0 <= c < cols and 0 <= r < rows), c, r


def edge_key(a, b, with_square=False):
    """Step 3: sqrt(mx^2 + my^2 + mz^2) of the mid-point."""
    with np.errstate(all="ignore"):
        m = []
        for k in range(3):
            s = a[k] + b[k]
            m.append(s / f64(2))
        x2 = m[0] * m[0]
        y2 = m[1] * m[1]
        s = x2 + y2
        z2 = m[2] * m[2]
        s = s + z2
        key = np.sqrt(s)
    return (key, s) if with_square else key


def covers(p, a, b, w):
    """Pixel p lies within w / 2 of the segment between pixels a and b: Python integers, no bound on anything."""
    ex, ey, fx, fy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    len2, along = ex * ex + ey * ey, fx * ex + fy * ey
    if along <= 0 or len2 == 0:
        return 4 * (fx * fx + fy * fy) <= w * w
    if along >= len2:
        gx, gy = p[0] - b[0], p[1] - b[1]
        return 4 * (gx * gx + gy * gy) <= w * w
    area = fx * ey - fy * ex
    return 4 * area * area <= w * w * len2


def camera_verdict(Y, cam, T, rows, cols, w, variant=None):
    """One camera: dict with drawable / seen / hidden [M] bools, painted [M - 1] bools, keys, rank (edge -> rank or None), first [M], pixels."""
    Y = np.asarray(Y, dtype=f64)
    M = Y.shape[0]
    q = [cam_node(T, Y[m], fused=(variant == "fused")) for m in range(M)]
    px = [pixel(cam, q[m], rows, cols) for m in range(M)]
    drawable = [p[0] for p in px]
    seen = [p[0] if variant == "no_image" else p[1] for p in px]
    painted = [drawable[i] and drawable[i + 1] for i in range(M - 1)]
    src = [[f64(v) for v in Y[m]] for m in range(M)] if variant == "rig_keys" else q
    keys = [edge_key(src[i], src[i + 1]) if painted[i] or variant == "all_edges" else None for i in range(M - 1)]
    ranked = [i for i in range(M - 1) if painted[i] or variant == "all_edges"]
    if variant == "all_edges":                    # (a key that is NaN sorts last: only the wrong reading meets one)
        ranked.sort(key=lambda i: (bool(np.isnan(keys[i])), float(np.nan_to_num(keys[i])), i))
    else:
        ranked.sort(key=lambda i: (float(keys[i]), i))
    rank = {e: r for r, e in enumerate(ranked)}
    first, hidden = [], []
    for m in range(M):
        inc = [rank[e] for e in (m - 1, m) if 0 <= e < M - 1 and e in rank]
        f = min(inc) if inc else len(ranked)
        first.append(f)
        h = False
        if drawable[m]:
            for e in ranked[:f]:                  # (only the wrong reading "all_edges" has an edge here that is not painted: its ends' pixels default to (0, 0))
                if covers(px[m][2:], px[e][2:], px[e + 1][2:], w):
                    h = True
                    break
        hidden.append(h)
    return dict(drawable=drawable, seen=seen, hidden=hidden, painted=painted, keys=keys, rank=rank, first=first, px=[p[2:] for p in px], n_painted=sum(painted))


def words(bits):
    M = len(bits)
    out = np.zeros((M + 31) // 32, dtype=np.uint32)
    for m, b in enumerate(bits):
        if b:
            out[m >> 5] |= np.uint32(1 << (m & 31))
    return out


def rig_verdict(Y, cams, mats, rows, cols, w, node_dist, thr, variant=None):
    """The rig's verdict: (visible indices int32 ascending, seen words [K x W], hidden words [K x W], the per-camera dicts)."""
    Y = np.asarray(Y, dtype=f64)
    M, K = Y.shape[0], len(cams)
    per = [camera_verdict(Y, cams[k], None if mats is None else mats[k], rows, cols, w, variant) for k in range(K)]
    vis = []
    for m in range(M):
        if not node_dist[m] <= thr:                # (NaN fails)
            continue
        votes = [c["seen"][m] and not c["hidden"][m] for c in per]
        sees = [c["seen"][m] for c in per]
        ok = (any(sees) and all(v for v, s in zip(votes, sees) if s)) if variant == "any" else any(votes)
        if ok:
            vis.append(m)
    seen = np.stack([words(c["seen"]) for c in per])
    hidden = np.stack([words(c["hidden"]) for c in per])
    return np.array(vis, dtype=np.int32), seen, hidden, per


def proj_of(cam):
    """The 3 x 4 matrix of the consequence: {fx,0,cx,0, 0,fy,cy,0, 0,0,1,0}."""
    fx, fy, cx, cy = cam
    return np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], dtype=f64)
