"""The numpy statement of image views (tdlo_image_view, include/trackdlo_hip.h): the canonical image a view stands for, the 32FC1 -> millimetre rule,
and the bytes a view addresses.  Everything that takes a view -- the host pack (csrc/tdlo_image_host.cpp) and k_image_import (csrc/tdlo_image.hip) -- is
held to canonical() byte for byte.  A view is stated on a flat uint8 buffer: `byte_offset` is where v->data points into it."""
import numpy as np

U8C1, U8C3, U8C4, U16C1, F32C1 = 0, 1, 2, 3, 4
DEPTH, COLOUR, OCCLUDER, MASK = 0, 1, 2, 3
BPP = {U8C1: 1, U8C3: 3, U8C4: 4, U16C1: 2, F32C1: 4}            # bytes per pixel
ELEM = {U8C1: 1, U8C3: 1, U8C4: 1, U16C1: 2, F32C1: 4}           # bytes per element
ROLE_FORMATS = {DEPTH: (U16C1, F32C1), COLOUR: (U8C3, U8C4), OCCLUDER: (U8C1,), MASK: (U8C1,)}
MAX_PIXELS = 1 << 26


def f32_to_mm(d):
    """mm = floor(1000 d + 1/2) where 0 <= 1000 d + 1/2 < 65536, else 0 (NaN, +-inf, negatives, d >= 65.5355).  Evaluated in float64, where the product
    and the sum are exact wherever the result can depend on them (1000 d >= 0.125; below that the sum is under 1)."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = d.astype(np.float64) * 1000.0 + 0.5
        ok = (x >= 0.0) & (x < 65536.0)
        return np.where(ok, np.floor(np.where(ok, x, 0.0)), 0.0).astype(np.uint16)


def f32_to_mm_exact(d):
    """The same rule in exact rational arithmetic, one value at a time (the check of the float64 evaluation above)."""
    from fractions import Fraction
    import math
    d = float(np.float32(d))
    if math.isnan(d) or math.isinf(d):
        return 0
    x = Fraction(d) * 1000 + Fraction(1, 2)
    return math.floor(x) if 0 <= x < 65536 else 0


def extent(format, row_stride, rows, cols):
    """[lo, hi) in bytes relative to data: [min over rows of the row's start, max over rows of the row's start + cols x bytes per pixel)."""
    starts = [0, (rows - 1) * row_stride]
    return min(starts), max(starts) + cols * BPP[format]


def check(data_address, format, location, row_stride, rows, cols, role):
    """True when (view, rows, cols, role) describes an image (the list of tdlo_image_view_check)."""
    if data_address == 0 or role not in ROLE_FORMATS or format not in BPP or location not in (0, 1, 2):
        return False
    if format not in ROLE_FORMATS[role] or rows <= 0 or cols <= 0 or rows * cols > MAX_PIXELS:
        return False
    if data_address % ELEM[format] or row_stride % ELEM[format]:
        return False
    if rows > 1 and abs(row_stride) < cols * BPP[format]:
        return False
    lo, hi = extent(format, row_stride, rows, cols)
    return -(1 << 62) < lo and hi < (1 << 62)


def canonical(buffer, byte_offset, format, row_stride, rows, cols):
    """The packed canonical image of the view: uint16 [rows x cols] depth (U16C1 as it is, F32C1 by f32_to_mm), uint8 [rows x cols x 3] colour (the first
    three bytes of every pixel), uint8 [rows x cols] occluder / mask."""
    buf = np.frombuffer(buffer, dtype=np.uint8) if not isinstance(buffer, np.ndarray) else buffer.view(np.uint8).reshape(-1)
    bpp = BPP[format]
    idx = byte_offset + np.arange(rows, dtype=np.int64)[:, None, None] * row_stride + np.arange(cols, dtype=np.int64)[None, :, None] * bpp + np.arange(bpp, dtype=np.int64)
    assert idx.min() >= 0 and idx.max() < buf.size
    px = np.ascontiguousarray(buf[idx])                           # rows x cols x bpp bytes
    if format == U8C1:
        return px[:, :, 0].copy()
    if format in (U8C3, U8C4):
        return np.ascontiguousarray(px[:, :, :3])
    if format == U16C1:
        return px.view(np.uint16)[:, :, 0].copy()
    return f32_to_mm(px.view(np.float32)[:, :, 0])


def form(data_address, row_stride, cols, format):
    """The import kernel's load form: 0 element by element; with cols % 4 == 0 and data, pitch multiples of 4: 1 dword loads; multiples of 8 (U16C1) / 16
    (U8C4, F32C1) as well: 2, one wide load.  A vector load must be naturally aligned and lie inside one row."""
    if cols % 4 or data_address % 4 or row_stride % 4:
        return 0
    wide = {U16C1: 8, U8C4: 16, F32C1: 16}.get(format, 0)
    return 2 if wide and data_address % wide == 0 and row_stride % wide == 0 else 1


def layouts(rows, cols, format, rng, poison=None):
    """The layouts both suites use: (name, buffer, byte_offset, row_stride).  data byte offset in {0, 1, 2, 4, 8} kept to the element's alignment;
    pitch = row bytes + {0, one element, 4, 12, 16}; a negative stride.  Every byte of the buffer outside the view's rows holds a poison that changes the
    canonical image if it is used: 0xA5 bytes (a nonzero mask, a colour, 42405 mm) or, for F32C1, floats that convert to other millimetres (1.2345 m)."""
    bpp, es = BPP[format], ELEM[format]
    row_bytes = cols * bpp
    out = []

    def lay(name, off, stride):
        lo, hi = extent(format, stride, rows, cols)
        base = off - lo                                            # data's place in the buffer: `off` poisoned bytes in front of the extent
        size = base + hi
        if format == F32C1:
            buf = np.full((size + 3) // 4 + 1, 1.2345, dtype=np.float32).view(np.uint8)[off % 4:][:size].copy()
        else:
            buf = np.full(size, 0xA5, dtype=np.uint8)
        for r in range(rows):
            s = base + r * stride
            if format == F32C1:
                mm = rng.integers(0, 65536, cols)
                mm[rng.random(cols) < 0.2] = 0
                buf[s:s + row_bytes] = (mm / 1000.0).astype(np.float32).view(np.uint8)
            else:
                buf[s:s + row_bytes] = rng.integers(0, 256, row_bytes, dtype=np.uint8)
            if format == U8C4 and poison is not False:
                buf[s + 3:s + row_bytes:4] = rng.integers(1, 256, cols, dtype=np.uint8)      # alpha: never 0, never used
        out.append((name, buf, base, stride))

    for off in (0, 1, 2, 4, 8):
        if off % es == 0:
            lay(f"off{off}", off, row_bytes)
    for extra in (es, 4, 12, 16):
        if extra % es == 0:
            lay(f"pitch+{extra}", 0, row_bytes + extra)
    lay("bottom-up", 0, -row_bytes)
    lay("bottom-up-pitch+16", 0, -(row_bytes + 16))
    if es < 4:
        lay("off-and-pitch", es, row_bytes + es)
    return out
