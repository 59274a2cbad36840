"""The numpy statement of V(view, N, select, leaf): pcl::VoxelGrid (PCL 1.10 applyFilter, downsample_all_data, min_points_per_voxel = 0, no filter
field) on the points of a cloud view, as include/trackdlo_hip.h states it for tdlo_cloud_view_voxel_grid -- written from that contract, not from the
kernels.  All point arithmetic is np.float32; a cell's points are summed SEQUENTIALLY in input order (np.add.at adds in index order; np.sum and
reduceat add pairwise and do not give PCL's bits)."""
import numpy as np

F = np.float32
I32_MAX = 2 ** 31 - 1


class TooFar(ValueError):
    """Step 8: no pass-through and a floor(mn * inv) or floor(mx * inv) outside int32 -- TDLO_E_INVALID."""


class BadGrid(ValueError):
    """A leaf that is no positive finite float, or a box with mn > mx / a component that is not finite -- TDLO_E_INVALID."""


def backproject(depth, mask, fx, fy, cx, cy):
    """The float32 points of the masked pixels in row-major order, by the arithmetic of trackdlo_node.cpp:219-224 (double arithmetic, float storage)."""
    depth = np.asarray(depth, dtype=np.uint16)
    i, j = np.nonzero(np.asarray(mask) != 0)                      # row-major
    z = depth[i, j].astype(np.float64) / 1000.0
    x = (j.astype(np.float64) - cx) * z / fx
    y = (i.astype(np.float64) - cy) * z / fy
    return np.stack([x.astype(F), y.astype(F), z.astype(F)], axis=1)


def to_float(P):
    """Step 1: float32 passes through; float64 is rounded to nearest-even, beyond float range to +-inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(P)[:, :3].astype(F)


def kept(P32, select=None):
    """Step 2: all three floats finite and, with a selection, its byte != 0."""
    k = np.isfinite(P32).all(axis=1)
    if select is not None:
        k &= np.asarray(select).reshape(-1) != 0
    return k


def grid(mn, mx, leaf_size):
    """Steps 5, 6, 8 on a float box: (min_b [3] int64, div_b [3] int64, nodown).  Pass-through: min_b = 0, div_b = 1."""
    leaf = F(leaf_size)
    mn = np.asarray(mn, dtype=F); mx = np.asarray(mx, dtype=F)
    if not (leaf > 0 and np.isfinite(leaf)):
        raise BadGrid("leaf")
    if not (np.isfinite(mn).all() and np.isfinite(mx).all() and (mn <= mx).all()):
        raise BadGrid("box")
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv = F(1.0) / leaf
        ext = (mx - mn) * inv                                     # float32
        prod, nodown = 1, False                                   # python integers: exact
        for d in range(3):
            if not (np.isfinite(ext[d]) and ext[d] < F(2.0 ** 31)):
                nodown = True
                break
            prod *= int(ext[d]) + 1                               # (long long) truncates
            if prod > I32_MAX:
                nodown = True
                break
        if nodown:
            return np.zeros(3, dtype=np.int64), np.ones(3, dtype=np.int64), True
        lo = np.floor(mn * inv); hi = np.floor(mx * inv)          # float32
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise TooFar()
    lo_i = np.array([int(v) for v in lo], dtype=object); hi_i = np.array([int(v) for v in hi], dtype=object)
    if any(v < -2 ** 31 or v > I32_MAX for v in list(lo_i) + list(hi_i)) or any(int(h) - int(l) + 1 > I32_MAX for l, h in zip(lo_i, hi_i)):
        raise TooFar()
    return lo_i.astype(np.int64), (hi_i - lo_i + 1).astype(np.int64), False


class TooManyCells(ValueError):
    """Step 9: div_b0 div_b1 div_b2 >= 0xffffffff -- TDLO_E_INVALID."""


def bits_for(values):
    """Bits that hold 0 .. values - 1 (at least one)."""
    return 1 if values <= 2 else (int(values) - 1).bit_length()


def group(Q, leaf_size):
    """Steps 5 .. 10 on the kept points Q [n_raw x 3] float32, n_raw > 0: (min_b, div_b, nodown, key, order, cell).  key [n_raw] int64 is every point's cell
    index, order the stable ascending sort of key, cell [n_raw] the output index of every SORTED point.  With nodown the last three are None."""
    min_b, div_b, nodown = grid(Q.min(axis=0), Q.max(axis=0), leaf_size)
    if nodown:
        return min_b, div_b, True, None, None, None
    if int(div_b[0]) * int(div_b[1]) * int(div_b[2]) >= 0xffffffff:
        raise TooManyCells()
    inv = F(1.0) / F(leaf_size)
    ijk = (np.floor(Q * inv) - min_b.astype(F)[None, :]).astype(np.int64)      # float32 floor and subtraction, then (int)
    key = ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(len(ks), dtype=bool); head[1:] = ks[1:] != ks[:-1]
    return min_b, div_b, False, key, order, np.cumsum(head) - 1


def centroids(Qs, cell):
    """Step 10: Qs [n_raw x 3] float32 in sorted order, cell [n_raw] their output index.  Sequential float32 sums from 0 in the given order,
    float32 division, widened."""
    n = int(cell.max()) + 1
    sums = np.zeros((n, 3), dtype=F)
    np.add.at(sums, cell, Qs)                                     # sequential float32 sums in input order
    cnt = np.bincount(cell, minlength=n).astype(F)
    return (sums / cnt[:, None]).astype(np.float64)               # float32 division, correctly rounded; widened


def structure(P, select, leaf_size):
    """What the reference's own arithmetic makes of a point set: a dict of n_raw, nodown, min_b, div_b, cells (div_b0 div_b1 div_b2), rb = bits_for(n_raw),
    kb = bits_for(cells), runs (the occupied cells' point counts in ascending key order; with nodown every point is its own run) and n = len(runs)."""
    P32 = to_float(P)
    Q = P32[kept(P32, select)]
    n_raw = Q.shape[0]
    if n_raw == 0:
        return dict(n_raw=0, nodown=False, min_b=None, div_b=None, cells=0, rb=1, kb=1, runs=np.zeros(0, dtype=np.int64), n=0)
    min_b, div_b, nodown, _, _, cell = group(Q, leaf_size)
    runs = np.ones(n_raw, dtype=np.int64) if nodown else np.bincount(cell).astype(np.int64)
    cells = int(div_b[0]) * int(div_b[1]) * int(div_b[2])
    return dict(n_raw=n_raw, nodown=nodown, min_b=min_b, div_b=div_b, cells=cells, rb=bits_for(n_raw), kb=bits_for(cells), runs=runs, n=len(runs))


def voxel_ref(P, select, leaf_size):
    """V: returns (X [n x 3] float64, n_raw).  P: [N x >= 3] float32 or float64."""
    P32 = to_float(P)
    Q = P32[kept(P32, select)]                                    # kept points, input order
    n_raw = Q.shape[0]
    if n_raw == 0:
        return np.zeros((0, 3)), 0
    _, _, nodown, _, order, cell = group(Q, leaf_size)
    if nodown:
        return Q.astype(np.float64), n_raw                        # step 7: the kept points, input order
    return centroids(Q[order], cell), n_raw
