"""Numpy statement of the colour segmentation in front of the depth -> cloud step (trackdlo_node.cpp:84-119, :158-180): 8-bit BGR -> HSV by
OpenCV's published integer routine (hsv_shift = 12, hue range 180: two tables of rounded fixed-point quotients, NOT the rounded float formula),
cv::inRange over up to four ranges, the AND with an occluder image.  Restated from the algorithm; parity against OpenCV itself is unpinned (OpenCV is
not part of the build image).  The device code (csrc/tdlo_cloud.hip, colour_hsv) is held to this file bit for bit over the whole colour cube."""
import numpy as np

HSV_SHIFT = 12

# the launch file's single range and color_thresholding's four (trackdlo_node.cpp:88-99: blue, red above 130, red below 10, yellow), H S V
LAUNCH_RANGE = ([[90, 90, 30]], [[130, 255, 255]])
MULTI_RANGES = ([[90, 90, 60], [130, 60, 50], [0, 60, 50], [15, 100, 80]], [[130, 255, 255], [255, 255, 255], [10, 255, 255], [40, 255, 255]])


def tables():
    """sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)) in fp64, ties to even; entry 0 is 0."""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv = np.zeros(256, dtype=np.int32); hdiv = np.zeros(256, dtype=np.int32)
    sdiv[1:] = np.rint((255 << HSV_SHIFT) / (1.0 * i)).astype(np.int32)
    hdiv[1:] = np.rint((180 << HSV_SHIFT) / (6.0 * i)).astype(np.int32)
    return sdiv, hdiv


_SDIV, _HDIV = tables()


def bgr_to_hsv(img, rgb_order=0):
    """img: [..., 3] uint8 (B, G, R; rgb_order = 1: R, G, B).  Returns [..., 3] uint8 (H 0..179, S, V)."""
    img = np.asarray(img, dtype=np.uint8)
    b = img[..., 2 if rgb_order else 0].astype(np.int32); g = img[..., 1].astype(np.int32); r = img[..., 0 if rgb_order else 2].astype(np.int32)
    v = np.maximum(np.maximum(b, g), r); vmin = np.minimum(np.minimum(b, g), r)
    d = v - vmin
    s = (d * _SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * _HDIV[d] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT            # (numpy's >> on signed integers is the arithmetic shift)
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def in_ranges(hsv, lower, upper):
    """255 where any of the ranges passes (lo <= hsv <= hi on all three channels, bounds clamped to 0..255), else 0."""
    lo = np.clip(np.asarray(lower, dtype=np.int64).reshape(-1, 3), 0, 255); hi = np.clip(np.asarray(upper, dtype=np.int64).reshape(-1, 3), 0, 255)
    assert 1 <= len(lo) <= 4 and len(lo) == len(hi)
    x = hsv.astype(np.int64)
    ok = np.zeros(hsv.shape[:-1], dtype=bool)
    for l, u in zip(lo, hi):
        ok |= np.all((x >= l) & (x <= u), axis=-1)
    return ok.astype(np.uint8) * 255


def colour_mask(img, lower, upper, rgb_order=0, occluder=None):
    """The frame's segmentation mask (trackdlo_node.cpp:159-180): inRange of the HSV image, 0 where the occluder image is 0."""
    m = in_ranges(bgr_to_hsv(img, rgb_order), lower, upper)
    if occluder is not None:
        m = np.where(np.asarray(occluder) != 0, m, 0).astype(np.uint8)
    return m


def cube():
    """Every 8-bit colour once: [4096, 4096, 3] uint8, pixel index = b | g << 8 | r << 16."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def textbook(img):
    """The textbook float formula without rounding, in fp64: H in degrees (60 (g - b) / d, 120 + 60 (b - r) / d, 240 + 60 (r - g) / d, + 360 when
    negative) halved, S = 255 d / v.  Returns (H [0, 180), S) as float64."""
    b = img[..., 0].astype(np.float64); g = img[..., 1].astype(np.float64); r = img[..., 2].astype(np.float64)
    v = np.maximum(np.maximum(b, g), r); d = v - np.minimum(np.minimum(b, g), r)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, 255.0 * d / v, 0.0)
        h = np.where(v == r, 60.0 * (g - b) / d, np.where(v == g, 120.0 + 60.0 * (b - r) / d, 240.0 + 60.0 * (r - g) / d))
    h = np.where(d > 0, h, 0.0)
    h = np.where(h < 0, h + 360.0, h)
    return h / 2.0, s
