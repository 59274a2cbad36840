"""Depth aligned to the colour camera (include/trackdlo_hip.h: tdlo_align_depth): the numpy statement, a literal per-pixel restatement with the wrong readings a
test tells from it, and the scenes.  float64 throughout; every product, quotient and sum is one numpy operation, i.e. rounded on its own, left to right.

A scene is a dict: D (uint16 millimetres, or float32 metres), p (the params: rows_d .. max_footprint, T = None or a 3 x 4 array).  Each scene is there for one
property, which tests/test_align_ref.py asserts on the reference."""
from fractions import Fraction

import numpy as np

LIM = 2.0 ** 30


def params(rows_d, cols_d, fd, cd, rows_c, cols_c, fc, cc, T=None, max_footprint=0):
    return dict(rows_d=rows_d, cols_d=cols_d, fx_d=float(fd[0]), fy_d=float(fd[1]), cx_d=float(cd[0]), cy_d=float(cd[1]),
                rows_c=rows_c, cols_c=cols_c, fx_c=float(fc[0]), fy_c=float(fc[1]), cx_c=float(cc[0]), cy_c=float(cc[1]),
                T=None if T is None else np.ascontiguousarray(T, np.float64).reshape(3, 4), max_footprint=max_footprint)


def to_mm(D):
    """uint16 stays; float32 metres -> millimetres by the image views' rule: floor(1000 d + 1/2) where that lies in [0, 65536), else 0"""
    D = np.asarray(D)
    if D.dtype == np.uint16:
        return D
    assert D.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        x = D.astype(np.float64) * 1000.0 + 0.5
        ok = (x >= 0.0) & (x < 65536.0)
    return np.where(ok, np.floor(np.where(ok, x, 0.0)), 0.0).astype(np.uint16)


def _corners(K, p, s):
    """(X, Y, bad) of corner s of every depth pixel, vectorised; X, Y are int64 and meaningless where bad"""
    rows, cols = K.shape
    u = np.arange(cols, dtype=np.float64)[None, :] + s
    v = np.arange(rows, dtype=np.float64)[:, None] + s
    z = K.astype(np.float64) / 1000.0
    with np.errstate(all="ignore"):
        x = ((u - p["cx_d"]) / p["fx_d"]) * z
        y = ((v - p["cy_d"]) / p["fy_d"]) * z
        if p["T"] is None:
            qx, qy, qz = x, y, z
        else:
            T = p["T"]
            qx = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
            qy = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
            qz = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
        bad = ~(qz > 0.0) | ~np.isfinite(qx) | ~np.isfinite(qy) | ~np.isfinite(qz)
        px = (qx / qz) * p["fx_c"] + p["cx_c"]
        py = (qy / qz) * p["fy_c"] + p["cy_c"]
        bad |= ~(np.abs(px) < LIM) | ~(np.abs(py) < LIM)
        X = np.floor(np.where(bad, 0.0, px) + 0.5).astype(np.int64)
        Y = np.floor(np.where(bad, 0.0, py) + 0.5).astype(np.int64)
    return X, Y, bad, px, py


def verdicts(D, p):
    """per depth pixel: 0 no return, 1 used, 2 dropped, 3 wide -- and the footprints (x0, y0, x1, y1)"""
    K = to_mm(D)
    mf = p["max_footprint"] or 16
    x0, y0, b0, _, _ = _corners(K, p, -0.5)
    x1, y1, b1, _, _ = _corners(K, p, 0.5)
    dropped = b0 | b1 | (x0 < 0) | (y0 < 0) | (x1 >= p["cols_c"]) | (y1 >= p["rows_c"]) | (x1 < x0) | (y1 < y0)
    wide = ~dropped & (((x1 - x0 + 1) > mf) | ((y1 - y0 + 1) > mf))
    ver = np.where(K == 0, 0, np.where(dropped, 2, np.where(wide, 3, 1)))
    return ver, (x0, y0, x1, y1)


def counts_of(ver):
    return [int((ver != 0).sum()), int((ver == 1).sum()), int((ver == 2).sum()), int((ver == 3).sum())]


def align(D, p):
    """THE STATEMENT.  Returns (A uint16 [rows_c, cols_c], counts [4])"""
    K = to_mm(D)
    ver, (x0, y0, x1, y1) = verdicts(D, p)
    mf = p["max_footprint"] or 16
    plane = np.full(p["rows_c"] * p["cols_c"], 0xFFFFFFFF, np.uint32)
    used = ver == 1
    k = K[used].astype(np.uint32)
    ax0, ay0, ax1, ay1 = x0[used], y0[used], x1[used], y1[used]
    for dy in range(mf):
        my = ay0 + dy <= ay1
        if not my.any():
            break
        for dx in range(mf):
            m = my & (ax0 + dx <= ax1)
            if not m.any():
                break
            np.minimum.at(plane, (ay0[m] + dy) * p["cols_c"] + ax0[m] + dx, k[m])
    A = np.where(plane == 0xFFFFFFFF, 0, plane).astype(np.uint16).reshape(p["rows_c"], p["cols_c"])
    return A, counts_of(ver)


def fma(a, b, c):
    """round(a b + c), one rounding: exact rational arithmetic (float(Fraction) rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def align_literal(D, p, rounding="floor", dtype=np.float64, reduce="min", footprint=True, clip=False, wide_first=False, fused=False):
    """The statement pixel by pixel in plain Python (small images), with the wrong readings as switches:
    rounding="trunc" the SDK's (int)(p + 0.5); dtype=np.float32 the arithmetic in single precision; reduce="last" / "max" for the minimum; footprint=False the
    centre pixel only; clip=True footprints clipped to the image instead of dropped; wide_first=True the wide test in front of the border test;
    fused=True the transform's multiply-adds fused (one rounding each)."""
    K = to_mm(D)
    f = dtype
    mf = p["max_footprint"] or 16
    rows_c, cols_c = p["rows_c"], p["cols_c"]
    A = np.zeros((rows_c, cols_c), np.int64)
    have = np.zeros((rows_c, cols_c), bool)
    n = [0, 0, 0, 0]
    g = {k: f(p[k]) for k in ("fx_d", "fy_d", "cx_d", "cy_d", "fx_c", "fy_c", "cx_c", "cy_c")}
    T = None if p["T"] is None else p["T"].astype(f)

    def corner(u, v, s, z):
        with np.errstate(all="ignore"):
            x = ((f(u + s) - g["cx_d"]) / g["fx_d"]) * z
            y = ((f(v + s) - g["cy_d"]) / g["fy_d"]) * z
            if T is None:
                q = (x, y, z)
            elif fused:
                q = tuple(f(fma(float(T[i, 2]), float(z), fma(float(T[i, 1]), float(y), float(T[i, 0] * x)))) + T[i, 3] for i in range(3))
            else:
                q = tuple(((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3))
            if not (q[2] > 0) or not all(np.isfinite(c) for c in q):
                return None
            px = (q[0] / q[2]) * g["fx_c"] + g["cx_c"]
            py = (q[1] / q[2]) * g["fy_c"] + g["cy_c"]
            if not (abs(px) < LIM) or not (abs(py) < LIM):
                return None
            if rounding == "trunc":
                return int(px + f(0.5)), int(py + f(0.5))
            return int(np.floor(px + f(0.5))), int(np.floor(py + f(0.5)))

    for v in range(K.shape[0]):
        for u in range(K.shape[1]):
            k = int(K[v, u])
            if k == 0:
                continue
            n[0] += 1
            z = f(k) / f(1000.0)
            if footprint:
                c0, c1 = corner(u, v, -0.5, z), corner(u, v, 0.5, z)
            else:
                c0 = c1 = corner(u, v, 0.0, z)
            if c0 is None or c1 is None:
                n[2] += 1
                continue
            (x0, y0), (x1, y1) = c0, c1
            is_wide = x1 - x0 + 1 > mf or y1 - y0 + 1 > mf
            if wide_first and is_wide:
                n[3] += 1
                continue
            if clip:
                if x1 < x0 or y1 < y0 or x1 < 0 or y1 < 0 or x0 >= cols_c or y0 >= rows_c:
                    n[2] += 1
                    continue
                x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, cols_c - 1), min(y1, rows_c - 1)
            elif x0 < 0 or y0 < 0 or x1 >= cols_c or y1 >= rows_c or x1 < x0 or y1 < y0:
                n[2] += 1
                continue
            if is_wide:
                n[3] += 1
                continue
            n[1] += 1
            for yy in range(y0, y1 + 1):
                for xx in range(x0, x1 + 1):
                    if not have[yy, xx] or reduce == "last" or (reduce == "min" and k < A[yy, xx]) or (reduce == "max" and k > A[yy, xx]):
                        A[yy, xx] = k
                        have[yy, xx] = True
    return A.astype(np.uint16), n


# ---- the scenes -------------------------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def transform(R=np.eye(3), t=(0.0, 0.0, 0.0)):
    return np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])


def depth_image(rows, cols, seed, lo=400, hi=3000, holes=0.1):
    rng = np.random.default_rng(seed)
    D = rng.integers(lo, hi, (rows, cols)).astype(np.uint16)
    D[rng.random((rows, cols)) < holes] = 0
    return D


def camera(rows, cols, f):
    """intrinsics of a rows x cols camera of focal length f pixels, the principal point a little off the centre (and no integer)"""
    return (f, f * 1.01), (cols / 2.0 - 0.37, rows / 2.0 + 0.21)


def same_camera(rows, cols, seed, T=None, **kw):
    f, c = camera(rows, cols, 0.9 * cols)
    return dict(D=depth_image(rows, cols, seed, **kw), p=params(rows, cols, f, c, rows, cols, f, c, T))


def scene_upscale(max_footprint=0):
    fd, cd = camera(48, 64, 60.0)
    fc, cc = camera(72, 96, 90.0)
    T = transform(rot("y", 1.5) @ rot("x", -1.0), (0.015, 0.001, -0.002))
    return dict(D=depth_image(48, 64, 11), p=params(48, 64, fd, cd, 72, 96, fc, cc, T, max_footprint))


def scene_downscale():
    fd, cd = camera(96, 128, 120.0)
    fc, cc = camera(48, 64, 60.0)
    rng = np.random.default_rng(12)
    D = rng.integers(900, 1100, (96, 128)).astype(np.uint16)                       # no holes: every output pixel is under at least four footprints
    return dict(D=D, p=params(96, 128, fd, cd, 48, 64, fc, cc, transform(np.eye(3), (0.002, 0.0, 0.0))))


def scene_one_pixel():
    fd, cd = camera(24, 32, 30.0)
    return dict(D=depth_image(24, 32, 13), p=params(24, 32, fd, cd, 9, 11, (1e-3, 1e-3), (5.0, 4.0)))


def scene_border():
    s = same_camera(40, 56, 14, transform(np.eye(3), (0.05, -0.04, 0.0)), lo=600, hi=1500, holes=0.05)
    fc = (s["p"]["fx_c"] * 1.3, s["p"]["fy_c"] * 1.3)
    s["p"] = dict(s["p"], fx_c=fc[0], fy_c=fc[1])
    return s


def scene_rot180():
    return same_camera(20, 28, 15, transform(rot("z", 180.0)))


def scene_looking_away():
    return same_camera(20, 28, 16, transform(rot("y", 180.0)))


def scene_rot80():
    s = same_camera(32, 48, 17, transform(rot("y", 80.0), (0.0, 0.0, 0.25)), lo=500, hi=900, holes=0.05)
    s["p"] = dict(s["p"], fx_d=20.0, fy_d=20.0, fx_c=10.0, fy_c=10.0)
    return s


def scene_ratio20(max_footprint=0):
    fd, cd = camera(12, 16, 15.0)
    fc, cc = camera(300, 400, 300.0)
    return dict(D=depth_image(12, 16, 18), p=params(12, 16, fd, cd, 300, 400, fc, cc, None, max_footprint))


def scene_ratio20_border():
    """the focal ratio of 20 with the colour camera turned aside: footprints that are wide AND reach over a border, which the statement counts as dropped"""
    s = scene_ratio20()
    s["p"] = dict(s["p"], cx_c=s["p"]["cx_c"] + 170.0, cy_c=s["p"]["cy_c"] - 120.0)
    return s


def scene_f32():
    s = same_camera(16, 24, 19)
    rng = np.random.default_rng(19)
    D = rng.uniform(0.4, 3.0, (16, 24)).astype(np.float32)
    flat = D.reshape(-1)
    flat[:14] = [np.nan, np.inf, -np.inf, -1.0, -0.0004, 65.5355, 65.5354, 70.0, 0.0004, 0.0005, 0.0015, 1.0005, 1.00049, 2.4995]
    flat[14:40] = (rng.integers(400, 3000, 26) + 0.5) / 1000.0                        # at the .5 mm borders, as float32 holds them
    s["D"] = D
    return s


def scene_rope(rows_d=480, cols_d=640, rows_c=720, cols_c=1280):
    """the full-size case: a rope-like depth band with 30 % holes over an empty image"""
    fd, cd = camera(rows_d, cols_d, 0.6 * cols_d)
    fc, cc = camera(rows_c, cols_c, 0.72 * cols_c)
    rng = np.random.default_rng(21)
    u = np.arange(cols_d)
    mid = rows_d / 2 + 0.2 * rows_d * np.sin(u / cols_d * 2 * np.pi)
    v = np.arange(rows_d)[:, None]
    band = np.abs(v - mid[None, :]) < 0.03 * rows_d
    D = np.where(band, 800 + (60 * np.sin(u / 37.0)).astype(np.int64)[None, :] + rng.integers(0, 5, (rows_d, cols_d)), 0).astype(np.uint16)
    D[rng.random((rows_d, cols_d)) < 0.3] = 0
    T = transform(rot("y", 0.8) @ rot("z", 0.3), (0.015, 0.0005, 0.001))
    return dict(D=D, p=params(rows_d, cols_d, fd, cd, rows_c, cols_c, fc, cc, T))


def scene_fused():
    """A scene that tells the fused transform from the statement: a generic T moves no corner across a pixel border (a fused and a separately rounded sum differ
    in the last bit, a border is hit by chance once in 2^40), so the border is put there -- corners are searched whose q_x differs between the two readings,
    and cx_c is chosen so that the separately rounded px + 0.5 is the integer n exactly or just below it while the fused one lies on the other side."""
    rng = np.random.default_rng(23)
    fd, cd = camera(6, 8, 9.0)
    T = transform(rot("y", 2.0) @ rot("x", 1.0), (0.0123, -0.0045, 0.0031))
    D = rng.integers(700, 1500, (6, 8)).astype(np.uint16)
    base = params(6, 8, fd, cd, 12, 16, (11.0, 11.0), (0.0, 6.3), T)
    for v in range(6):
        for u in range(8):
            z = float(D[v, u]) / 1000.0
            for s in (-0.5, 0.5):
                x = ((u + s - base["cx_d"]) / base["fx_d"]) * z
                y = ((v + s - base["cy_d"]) / base["fy_d"]) * z
                q = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
                qf = [fma(T[i, 2], z, fma(T[i, 1], y, T[i, 0] * x)) + T[i, 3] for i in range(3)]
                if not (q[2] > 0 and qf[2] > 0):
                    continue
                a, af = (q[0] / q[2]) * base["fx_c"], (qf[0] / qf[2]) * base["fx_c"]
                if a == af:
                    continue
                n = 7.0 if s < 0 else 9.0                                           # where the corner is to land: inside the image, the footprint 2 - 3 wide
                cx = (n - 0.5) - max(a, af)                                          # the larger reading's px + 0.5 is n up to rounding, the smaller one's lies below
                for _ in range(64):
                    lo, hi = min(a, af) + cx + 0.5, max(a, af) + cx + 0.5
                    if lo < n <= hi:
                        p = dict(base, cx_c=float(cx))
                        A, _ = align_literal(D, p)
                        F, _ = align_literal(D, p, fused=True)
                        if not np.array_equal(A, F):
                            return dict(D=D, p=p)
                        break
                    cx = np.nextafter(cx, np.inf if hi < n else -np.inf)
    raise AssertionError("no corner separates the fused transform from the statement")


def shapes():
    """depth sizes at the wave and block borders of k_align_splat (64 lanes a wave, 256 a workgroup): the same camera with a small T, the colour image two
    pixels larger on every side so that the border footprints are used too"""
    T = transform(rot("z", 0.7), (0.004, -0.003, 0.001))
    out = {}
    for r, c in ((1, 1), (1, 63), (1, 64), (1, 65), (3, 257), (5, 7)):
        f, cc = camera(r, c, 0.9 * max(c, 8))
        out[f"{r}x{c}"] = dict(D=depth_image(r, c, 100 + r + c, holes=0.15 if r * c > 1 else 0.0), p=params(r, c, f, cc, r + 4, c + 4, f, (cc[0] + 2.0, cc[1] + 2.0), T))
    return out


def all_scenes():
    sc = dict(shapes())
    sc.update(upscale=scene_upscale(), upscale_mf1=scene_upscale(1), downscale=scene_downscale(), one_pixel=scene_one_pixel(),
              identical_null=same_camera(24, 32, 20), identical_eye=same_camera(24, 32, 20, transform()), border=scene_border(), rot180=scene_rot180(),
              looking_away=scene_looking_away(), rot80=scene_rot80(), ratio20=scene_ratio20(), ratio20_mf64=scene_ratio20(64), ratio20_border=scene_ratio20_border(), f32=scene_f32(),
              all_zero=dict(same_camera(9, 13, 22), D=np.zeros((9, 13), np.uint16)), fused=scene_fused())
    return sc


def as_view_array(D, kind):
    """(buffer, data offset in bytes, row stride in bytes) of D laid out as `kind`: "packed", "pitched" (rows 3 elements apart from one another) or "bottom_up" """
    rows, cols = D.shape
    if kind == "packed":
        return np.ascontiguousarray(D), 0, cols * D.itemsize
    buf = np.full((rows, cols + 3), 7, D.dtype)                                      # (the padding holds a depth that would show if it were read)
    if kind == "pitched":
        buf[:, :cols] = D
        return buf, 0, (cols + 3) * D.itemsize
    buf[::-1, :cols] = D
    return buf, (rows - 1) * (cols + 3) * D.itemsize, -(cols + 3) * D.itemsize
