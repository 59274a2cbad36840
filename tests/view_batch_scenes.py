"""Scenes of the view-batch tests (tests/test_view_batch_cpu.py, tests/test_view_batch_gpu.py): point sets with optional selection bytes, built once and never
written again, and the rule -- from the reference's own arithmetic alone (tests/voxel_ref.py, tests/cloud_scenes.route_rule) -- that says what
tdlo_cloud_view_voxel_grid_batch does with each: "served" by the batch launch, "passed" on to the single call."""
import functools

import numpy as np

import cloud_scenes
import voxel_ref

LEAF = 0.008
TILE = 4096                        # elements per tile of the one-launch kernels
MAX_N = 1 << 20                    # elements of a frame the batch launch takes
NMAX = 32704                       # kept points the in-LDS sort takes
F32 = np.float32


def _ro(a):
    a.setflags(write=False)
    return a


def route(P, select, N=None, leaf=LEAF, fused=True):
    """What the call does with the frame (P [N x 3], select): 'served' or 'passed' -- from the reference structure alone."""
    N = len(P) if N is None else N
    if not fused or N > MAX_N:
        return "passed"
    try:
        st = voxel_ref.structure(P, select, leaf)
    except (voxel_ref.TooFar, voxel_ref.TooManyCells):
        return "passed"                                           # (cases 8 / 9: the single call refuses them)
    T = (N + TILE - 1) // TILE
    return "served" if cloud_scenes.route_rule(st, T) == "taken" else "passed"


def counts(frames, leaf=LEAF, fused=True):
    """[served, passed] over frames of (P, select)."""
    r = [route(P, s, leaf=leaf, fused=fused) for P, s in frames]
    return [r.count("served"), r.count("passed")]


@functools.lru_cache(maxsize=None)
def rope(N, seed, spread=0.004):
    """N float32 points scattered about a curved rope of 0.6 m: a compact cloud, a few points per 8 mm cell."""
    rng = np.random.default_rng(seed)
    s = rng.random(N)
    c = np.stack([0.6 * s - 0.3 + 0.01 * seed, 0.08 * np.sin(5.0 * s + seed), 0.55 + 0.05 * np.cos(3.0 * s)], axis=1)
    return _ro((c + spread * rng.standard_normal((N, 3))).astype(F32))


SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8193)       # the last word of a view, the tile border, frames of one and three tiles side by side


@functools.lru_cache(maxsize=None)
def box_cloud(N, seed, side=0.3):
    """N float32 points uniform in a cube: many occupied cells (32 704 points at 0.3 m: 16 cell bits + 15 rank bits)."""
    rng = np.random.default_rng(seed)
    return _ro((side * rng.random((N, 3)) + np.array([0.0, 0.0, 0.5])).astype(F32))


@functools.lru_cache(maxsize=None)
def wide_cloud(cells, n=5, seed=3):
    """n points whose box spans `cells` = (cx, cy, cz) leaf cells: the cell-index bits are set by the box, the rank bits by n."""
    rng = np.random.default_rng(seed)
    ext = np.array(cells, dtype=np.float64) * LEAF
    P = rng.random((n, 3)) * ext * 0.9
    P[0] = 0.0
    P[1] = ext - LEAF / 2
    return _ro(P.astype(F32))


@functools.lru_cache(maxsize=None)
def far_cloud():
    """Case 8 of the header: no pass-through, floor(mn / leaf) beyond int32 -- the frame fails on its own with TDLO_E_INVALID."""
    return _ro(np.array([[2.0e7, 0.0, 0.5], [2.0e7 + 2.0, 0.01, 0.5], [2.0e7, 0.02, 0.51]], dtype=F32))


@functools.lru_cache(maxsize=None)
def special_cloud():
    """Non-finite points among finite ones, and a cell of -0.0f only."""
    P = np.array(rope(600, 11))
    P[5] = [np.nan, 0.0, 0.5]; P[17] = [0.1, np.inf, 0.5]; P[99] = [0.1, 0.0, -np.inf]; P[300, 2] = np.nan
    P[400] = [-0.0, -0.0, 0.55]; P[401] = [-0.0, -0.0, 0.55]
    return _ro(P)


@functools.lru_cache(maxsize=None)
def organized(rows=96, cols=128, ropes=3, seed=5):
    """One organized cloud (rows x cols points, NaN where the sensor saw nothing) and `ropes` disjoint selections of a rope's worth each."""
    rng = np.random.default_rng(seed)
    j, i = np.meshgrid(np.arange(cols), np.arange(rows))
    z = 0.6 + 0.02 * rng.standard_normal((rows, cols))
    P = np.stack([(j - cols / 2) * z / 150.0, (i - rows / 2) * z / 150.0, z], axis=2).reshape(-1, 3).astype(F32)
    P[rng.random(rows * cols) < 0.05] = np.nan
    sels = []
    for r in range(ropes):
        m = np.zeros((rows, cols), dtype=np.uint8)
        r0 = 10 + 25 * r
        for c in range(cols):
            rr = r0 + int(6 * np.sin(c / 20.0 + r))
            m[rr:rr + 4, c] = 255 if r != 1 else 1                 # (any non-zero byte selects)
        sels.append(_ro(m.reshape(-1)))
    return _ro(P), sels


@functools.lru_cache(maxsize=None)
def big_view():
    """A view of MAX_N + 1 elements with a rope's worth selected: more than the batch launch takes."""
    N = MAX_N + 1
    P = np.array(box_cloud(N, 21, side=0.5))
    sel = np.zeros(N, dtype=np.uint8)
    sel[::353] = 7
    return _ro(P), _ro(sel)


def borders():
    """(name, P, select) of the frames at the borders of the in-LDS sort, in call order, each between served rope frames."""
    return [("rope-a", rope(700, 31), None),
            ("32704 kept", box_cloud(NMAX, 7), None),
            ("32705 kept", box_cloud(NMAX + 1, 8), None),
            ("rope-b", rope(4097, 32), None),
            ("rb + kb = 33", wide_cloud((1001, 1001, 701)), None),
            ("pass-through", wide_cloud((2001, 2001, 2001)), None),
            ("keeps nothing", rope(300, 33), _ro(np.zeros(300, dtype=np.uint8))),
            ("non-finite, -0.0f", special_cloud(), None),
            ("rope-c", rope(5, 34), None)]
