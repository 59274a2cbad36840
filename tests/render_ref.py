"""Numpy statement of the tracking-result image (trackdlo_node.cpp:377-452), written the reference's way: blend the whole image, then paint every
primitive in drawing order over its clipped bounding box -- a later one overwrites an earlier one.  (The kernel, csrc/tdlo_render.hip, does it the other
way round: every pixel searches the primitive table from its end for the last primitive that covers it.)

  blend   0.5 a + 0.5 (a & o), rounded half to even (cv::addWeighted on 8-bit images, cvRound)
  line    every pixel within width / 2 of the segment between the end pixels, in exact integers (the library's within_half_width)
  disc    dx^2 + dy^2 <= radius^2
Parity against OpenCV's own rasterisers is unpinned (OpenCV is not part of the build image)."""
import numpy as np

DEFAULTS = dict(line_width=5, node_radius=7, node_visible=(0, 150, 255), node_hidden=(0, 0, 255), edge_visible=(0, 255, 0), edge_hidden=(0, 0, 255))
PIXEL_LIMIT = 8192


class Guard(ValueError):
    """An input on which a last-bit difference could decide a pixel or the drawing order."""


def blend(colour, occluder=None):
    a = np.asarray(colour, dtype=np.uint8).astype(np.int64)
    o = np.full(a.shape[:2], 255, dtype=np.int64) if occluder is None else np.asarray(occluder, dtype=np.uint8).astype(np.int64)
    s = a + (a & o[..., None])
    return ((s >> 1) + ((s & 1) & ((s >> 1) & 1))).astype(np.uint8)


def node_pixels(Y, proj, guard=True):
    """(col, row) per node: fp64, the library's expression order, truncated towards zero.  Raises ValueError for a node that cannot be drawn."""
    Y = np.asarray(Y, dtype=np.float64); p = np.asarray(proj, dtype=np.float64).reshape(12)
    x, y, z = Y[:, 0], Y[:, 1], Y[:, 2]
    with np.errstate(all="ignore"):
        u = ((p[0] * x + p[1] * y) + p[2] * z) + p[3]
        v = ((p[4] * x + p[5] * y) + p[6] * z) + p[7]
        w = ((p[8] * x + p[9] * y) + p[10] * z) + p[11]
        if not np.all(w > 0):
            raise ValueError("w <= 0")
        qc, qr = u / w, v / w
    if not (np.all(np.isfinite(qc)) and np.all(np.isfinite(qr))):
        raise ValueError("non-finite pixel")
    c, r = np.trunc(qc), np.trunc(qr)
    if np.any(c < -PIXEL_LIMIT) or np.any(c > PIXEL_LIMIT - 1) or np.any(r < -PIXEL_LIMIT) or np.any(r > PIXEL_LIMIT - 1):
        raise ValueError("pixel beyond +-8192")
    if guard:
        for q in (qc, qr):
            if np.any(np.abs(q - np.rint(q)) < 1e-9):
                raise Guard("a pixel coordinate within 1e-9 of an integer")
    return c.astype(np.int64), r.astype(np.int64)


def edge_order(Y, guard=True):
    """Edge indices in drawing order: ascending by (camera distance of the mid-point, index), reversed."""
    Y = np.asarray(Y, dtype=np.float64)
    m = (Y[:-1] + Y[1:]) / 2
    key = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    order = sorted(range(len(key)), key=lambda i: (key[i], i))
    if guard:
        ks = key[order]
        if np.any(np.abs(np.diff(ks)) <= 1e-12 * np.abs(ks[1:])):
            raise Guard("two edge keys within 1e-12 relative")
    return order[::-1]


def _word(c):
    return int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)


def primitives(Y, proj, vis, params=None, guard=True):
    """[3 (M - 1) x 8] int32 {kind 0 line / 1 disc, c0, r0, c1, r1, size, b | g << 8 | r << 16, 0} in drawing order -- tdlo_render_primitives' records."""
    P = dict(DEFAULTS, **(params or {}))
    Y = np.asarray(Y, dtype=np.float64); M = len(Y)
    if not (1 <= P["line_width"] <= 255 and 1 <= P["node_radius"] <= 255):
        raise ValueError("sizes 1 .. 255")
    vis = [int(v) for v in vis]
    if any(v < 0 or v >= M for v in vis):
        raise ValueError("vis out of range")
    vs = set(vis)
    c, r = node_pixels(Y, proj, guard)
    out = []
    for i in edge_order(Y, guard):
        out.append([0, c[i], r[i], c[i + 1], r[i + 1], P["line_width"], _word(P["edge_visible"] if (i in vs or i + 1 in vs) else P["edge_hidden"]), 0])
        for k in (i, i + 1):
            out.append([1, c[k], r[k], c[k], r[k], P["node_radius"], _word(P["node_visible"] if k in vs else P["node_hidden"]), 0])
    return np.asarray(out, dtype=np.int32).reshape(-1, 8)


def covers(rec, cc, rr):
    """Boolean array: which of the pixels (cc, rr) (int64 arrays) the primitive covers."""
    kind, c0, r0, c1, r1, size = (int(v) for v in rec[:6])
    if kind == 1:
        return (cc - c0) ** 2 + (rr - r0) ** 2 <= size * size
    ex, ey = c1 - c0, r1 - r0
    fx, fy = cc - c0, rr - r0
    len2 = ex * ex + ey * ey
    along = fx * ex + fy * ey
    w2 = size * size
    cap_a = 4 * (fx * fx + fy * fy) <= w2
    gx, gy = cc - c1, rr - r1
    cap_b = 4 * (gx * gx + gy * gy) <= w2
    area = fx * ey - fy * ex
    body = 4 * area * area <= w2 * len2
    return np.where((along <= 0) | (len2 == 0), cap_a, np.where(along >= len2, cap_b, body))


def paint(img, prims):
    """Paints the records in order into img [rows x cols x 3 uint8], each over its clipped bounding box."""
    rows, cols = img.shape[:2]
    for rec in np.asarray(prims).reshape(-1, 8):
        kind, c0, r0, c1, r1, size = (int(v) for v in rec[:6])
        ext = size if kind == 1 else (size + 1) // 2
        x0, x1 = max(min(c0, c1) - ext, 0), min(max(c0, c1) + ext, cols - 1)
        y0, y1 = max(min(r0, r1) - ext, 0), min(max(r0, r1) + ext, rows - 1)
        if x0 > x1 or y0 > y1:
            continue
        rr, cc = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.int64), np.arange(x0, x1 + 1, dtype=np.int64), indexing="ij")
        hit = covers(rec, cc, rr)
        w = int(rec[6])
        img[y0:y1 + 1, x0:x1 + 1][hit] = (w & 255, (w >> 8) & 255, (w >> 16) & 255)
    return img


def corners(occluder):
    """[row, col of the first pixel in row-major order whose occluder byte is 0, row, col of the last]; -1 four times when there is none / no occluder."""
    if occluder is None:
        return [-1, -1, -1, -1]
    z = np.flatnonzero(np.asarray(occluder).reshape(-1) == 0)
    if len(z) == 0:
        return [-1, -1, -1, -1]
    cols = np.asarray(occluder).shape[1]
    return [int(z[0] // cols), int(z[0] % cols), int(z[-1] // cols), int(z[-1] % cols)]


def render(colour, occluder, Y, proj, vis, params=None, guard=True):
    """(image, corners)."""
    img = blend(colour, occluder)
    if len(Y) > 1:
        paint(img, primitives(Y, proj, vis, params, guard))
    else:
        primitives(Y, proj, vis, params, guard)          # (one node: validated, nothing drawn)
    return img, corners(occluder)


def nodes_from_pixels(px, proj_fx=100.0, z=None):
    """Nodes [M x 3] whose pixels under pinhole(proj_fx) are the integer pixels px [(col, row)]: the projection lands half a pixel beyond each coordinate,
    away from zero, so that node_pixels' guard passes and truncation towards zero gives exactly (col, row), negative ones included.
    z: per-node depth (decides the drawing order); default 1 + 0.01 m per node."""
    px = np.asarray(px, dtype=np.float64).reshape(-1, 2)
    z = 1.0 + 0.01 * np.arange(len(px)) if z is None else np.asarray(z, dtype=np.float64)
    q = px + np.where(px < 0, -0.5, 0.5)
    return np.stack([q[:, 0] * z / proj_fx, q[:, 1] * z / proj_fx, z], axis=1)


def pinhole(fx, fy=None, cx=0.0, cy=0.0):
    return np.array([fx, 0, cx, 0, 0, fx if fy is None else fy, cy, 0, 0, 0, 1, 0], dtype=np.float64)
