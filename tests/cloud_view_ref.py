"""The numpy statement of a cloud view (include/trackdlo_hip.h, tdlo_cloud_view): component c of point n is element
n * stride_point + c * stride_comp of the view, counted from `data`; the library's import is held to widen() bit for bit and its extent to extent()."""
import numpy as np
from numpy.lib.stride_tricks import as_strided


def widen(buffer, dtype, offset_elems, stride_point, stride_comp, N):
    """The N x 3 cloud the view addresses, as Fortran-ordered float64: what tdlo_set_cloud would be handed.  buffer: any array (or bytes-like) that
    holds the elements; `data` is element offset_elems of it, viewed as dtype."""
    flat = np.frombuffer(buffer, dtype=dtype) if not isinstance(buffer, np.ndarray) else buffer.reshape(-1).view(dtype)
    es = flat.itemsize
    lo, hi = extent(dtype, stride_point, stride_comp, N)
    assert 0 <= offset_elems * es + lo and offset_elems * es + hi <= flat.size * es, "the view leaves its buffer"
    v = as_strided(flat[offset_elems:offset_elems + 1], shape=(N, 3), strides=(stride_point * es, stride_comp * es))
    return np.asfortranarray(v.astype(np.float64))


def extent(dtype, stride_point, stride_comp, N):
    """[lo, hi) in bytes relative to `data`: first byte of the lowest element addressed to one past the last byte of the highest (Python integers)."""
    es = np.dtype(dtype).itemsize
    a, b = (N - 1) * int(stride_point), 2 * int(stride_comp)
    return (min(a, 0) + min(b, 0)) * es, (max(a, 0) + max(b, 0) + 1) * es
