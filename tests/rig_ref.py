"""The numpy statement of a rig (include/trackdlo_hip.h: tdlo_rig_to_cloud): the point list R of K cameras and the cloud V(R, leaf) -- written from the
contract, not from the kernels.  A camera's kept pixels in row-major order, camera after camera; the camera-frame point in float64 by the arithmetic of
trackdlo_node.cpp:219-224; with a transform [A | b] component r is (float32)(((A[r][0] xd + A[r][1] yd) + A[r][2] zd) + b[r]) -- numpy's element-wise
float64 products and sums are rounded one by one, which is the contract's "no fused multiply-add"; a point with a float that is not finite is dropped."""
from fractions import Fraction

import numpy as np

import colour_ref
import voxel_ref

F = np.float32


class Cam:
    """One camera of a rig: depth [rows x cols] uint16; mask [rows x cols] uint8, or colour [rows x cols x 3] uint8 with ranges = (lower, upper, rgb_order)
    and an optional occluder; cam = (fx, fy, cx, cy); T None or [3 x 4] float64."""

    def __init__(self, depth, mask=None, colour=None, ranges=None, occluder=None, cam=(1.0, 1.0, 0.0, 0.0), T=None):
        self.depth = np.ascontiguousarray(depth, dtype=np.uint16)
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self.colour = None if colour is None else np.ascontiguousarray(colour, dtype=np.uint8)
        self.ranges, self.occluder = ranges, (None if occluder is None else np.ascontiguousarray(occluder, dtype=np.uint8))
        self.cam = tuple(float(v) for v in cam)
        self.T = None if T is None else np.ascontiguousarray(T, dtype=np.float64).reshape(3, 4)

    def kept(self):
        """The camera's segmentation: its mask, or (no mask) the colour segmentation under its ranges with its occluder."""
        if self.mask is not None:
            return self.mask != 0
        lower, upper, rgb = self.ranges
        return colour_ref.colour_mask(self.colour, lower, upper, rgb, self.occluder) != 0

    def replaced(self, **kw):
        d = dict(depth=self.depth, mask=self.mask, colour=self.colour, ranges=self.ranges, occluder=self.occluder, cam=self.cam, T=self.T)
        d.update(kw)
        return Cam(**d)


def camera_frame(c):
    """(xd, yd, zd) float64 of the camera's kept pixels, row-major."""
    fx, fy, cx, cy = c.cam
    i, j = np.nonzero(c.kept())                                       # row-major
    zd = c.depth[i, j].astype(np.float64) / 1000.0
    xd = (j.astype(np.float64) - cx) * zd / fx
    yd = (i.astype(np.float64) - cy) * zd / fy
    return xd, yd, zd


def transformed(T, xd, yd, zd):
    """float64 [n x 3]: ((A[r][0] xd + A[r][1] yd) + A[r][2] zd) + b[r], every product and sum on its own."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((T[r, 0] * xd + T[r, 1] * yd) + T[r, 2] * zd) + T[r, 3] for r in range(3)], axis=1)


def camera_points(c):
    """The camera's share of R: float32 [n x 3], non-finite points dropped."""
    xd, yd, zd = camera_frame(c)
    P = np.stack([xd, yd, zd], axis=1) if c.T is None else transformed(c.T, xd, yd, zd)
    with np.errstate(over="ignore", invalid="ignore"):
        P32 = P.astype(F)
    return P32[np.isfinite(P32).all(axis=1)].reshape(-1, 3)


def points(cams):
    """R: float32 [n_raw x 3]."""
    return np.concatenate([camera_points(c) for c in cams], axis=0) if len(cams) else np.zeros((0, 3), dtype=F)


def rig_ref(cams, leaf):
    """(X [n x 3] float64, n_raw): V(R, leaf)."""
    return voxel_ref.voxel_ref(points(cams), None, leaf)


# ---- WRONG readings of the statement (tests/test_rig_ref.py tells each from it) ---------------------------------------------------------------------
def points_reversed(cams):
    return points(list(cams)[::-1])


def points_rounded_first(cams):
    """The camera-frame point rounded to float32 BEFORE the transform (what feeding K single back-projections to a float transform would do)."""
    out = []
    for c in cams:
        xd, yd, zd = camera_frame(c)
        if c.T is not None:
            xd, yd, zd = (v.astype(F).astype(np.float64) for v in (xd, yd, zd))
        P = np.stack([xd, yd, zd], axis=1) if c.T is None else transformed(c.T, xd, yd, zd)
        P32 = P.astype(F)
        out.append(P32[np.isfinite(P32).all(axis=1)].reshape(-1, 3))
    return np.concatenate(out, axis=0)


def points_float_transform(cams):
    """The transform evaluated in float32: matrix and point rounded, float32 products and sums."""
    out = []
    for c in cams:
        xd, yd, zd = camera_frame(c)
        if c.T is None:
            P32 = np.stack([xd, yd, zd], axis=1).astype(F)
        else:
            T, x, y, z = c.T.astype(F), xd.astype(F), yd.astype(F), zd.astype(F)
            P32 = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1).astype(F)
        out.append(P32[np.isfinite(P32).all(axis=1)].reshape(-1, 3))
    return np.concatenate(out, axis=0)


def _fma(a, b, c):
    """a b + c with ONE rounding (exact rational arithmetic; float() of a Fraction is correctly rounded)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def points_fused(cams, form=0):
    """The transform with fused multiply-adds, which the contract rules out.  form 0: fma(A2, zd, fma(A0, xd, A1 yd)) + b -- what a contracting compiler
    made of the three products and two sums; form 1: fma(A2, zd, fma(A1, yd, A0 xd)) + b, the source order fused.  In double nearly every component
    differs from the statement by an ulp now and then; after the rounding to float only where the sum lies at a float rounding boundary
    (rig_scenes.fused_boundary is built so that it does)."""
    out = []
    for c in cams:
        xd, yd, zd = camera_frame(c)
        if c.T is None:
            P = np.stack([xd, yd, zd], axis=1)
        else:
            P = np.empty((len(xd), 3))
            for r in range(3):
                a0, a1, a2, b = (float(v) for v in c.T[r])
                for k in range(len(xd)):
                    x, y, z = float(xd[k]), float(yd[k]), float(zd[k])
                    inner = _fma(a0, x, a1 * y) if form == 0 else _fma(a1, y, a0 * x)
                    P[k, r] = _fma(a2, z, inner) + b
        P32 = P.astype(F)
        out.append(P32[np.isfinite(P32).all(axis=1)].reshape(-1, 3))
    return np.concatenate(out, axis=0)


def points_fused_source_order(cams):
    return points_fused(cams, 1)
