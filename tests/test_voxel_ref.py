"""CPU suite for the voxel grid on cloud views: tests/voxel_ref.py (the numpy statement of V, include/trackdlo_hip.h) is held to the C oracle of the depth
path bit for bit, and tdlo_voxel_grid_dims -- the one host statement of the grid rule that the depth path and the view path share -- to voxel_ref's
grid.  No GPU."""
import numpy as np
import pytest

import voxel_ref as R

LEAVES = [0.008, 0.02, 0.05, 1e-6]          # the last is PCL's pass-through ("leaf size too small")
CAM = (606.0, 605.5, 63.5, 47.5)            # fx, fy, cx, cy of a 96 x 128 frame

TDLO_E_INVALID = -2


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    binding.load_library()
    return binding


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def random_frame(rng, rows=96, cols=128):
    depth = rng.integers(300, 1500, size=(rows, cols)).astype(np.uint16)
    mask = (rng.random((rows, cols)) < 0.3).astype(np.uint8) * 255
    return depth, mask


def smooth_frame(rng, rows=96, cols=128):
    """A slanted, gently curved surface close to the camera: neighbouring pixels share cells (several points per cell)."""
    i, j = np.mgrid[0:rows, 0:cols]
    z = 400.0 + 0.8 * j + 0.5 * i + 15.0 * np.sin(i / 9.0 + rng.random()) + rng.random((rows, cols))
    mask = ((i // 7 + j // 5) % 3 != 0).astype(np.uint8)
    return z.astype(np.uint16), mask


@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_voxel_ref_on_backprojected_points_is_the_depth_oracle_bit_for_bit(oracle, kind):
    fx, fy, cx, cy = CAM
    for seed in range(5):
        rng = np.random.default_rng(seed)
        depth, mask = random_frame(rng) if kind == "random" else smooth_frame(rng)
        P = R.backproject(depth, mask, fx, fy, cx, cy)
        assert P.dtype == np.float32 and P.shape == (np.count_nonzero(mask), 3)
        for leaf in LEAVES:
            want, want_raw = oracle.depth_to_cloud(depth, mask, fx, fy, cx, cy, leaf)
            got, got_raw = R.voxel_ref(P, None, leaf)
            assert got_raw == want_raw and got.shape == want.shape, (seed, leaf, got.shape, want.shape)
            np.testing.assert_array_equal(_bits(got), _bits(want))
            if leaf == 1e-6:
                assert got.shape[0] == want_raw                   # pass-through
            elif kind == "smooth" and leaf >= 0.02:
                assert got.shape[0] * 3 < want_raw                # several points per cell


def test_voxel_ref_selection_and_non_finite_points():
    rng = np.random.default_rng(3)
    P = rng.standard_normal((500, 3)).astype(np.float32)
    sel = (rng.random(500) < 0.5).astype(np.uint8)
    bad = P.copy()
    bad[::7, 1] = np.nan; bad[3::11, 0] = np.inf; bad[5::13, 2] = -np.inf
    fine = np.isfinite(bad).all(axis=1)
    a, na = R.voxel_ref(bad, sel, 0.2)
    b, nb = R.voxel_ref(P[fine & (sel != 0)], None, 0.2)
    assert na == nb == int((fine & (sel != 0)).sum())
    np.testing.assert_array_equal(_bits(a), _bits(b))
    big = P.astype(np.float64); big[10, 0] = 1e300; big[11, 2] = -1e39
    assert R.voxel_ref(big, None, 0.2)[1] == 498                  # beyond float range: +-inf, not kept
    assert R.voxel_ref(P, np.zeros(500, np.uint8), 0.2)[1] == 0


def _dims_cases():
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(200):                                           # random boxes, negative coordinates among them
        a = rng.uniform(-3, 3, 3); b = a + rng.uniform(0, 2, 3) * rng.integers(0, 2, 3)
        cases.append((a, b, float(rng.choice([0.008, 0.02, 0.05, 0.1, 1e-3]))))
    cases.append(([-2.5, -1.25, -0.75], [-2.0, -1.0, -0.5], 0.008))
    cases.append(([0.5, -0.25, 1.0], [0.5, -0.25, 1.0], 0.008))    # mn == mx
    cases.append(([0.008, 0.016, -0.008], [0.008, 0.016, -0.008], 0.008))
    # the stepwise product across 2^31 - 1 from both sides: dd = (1290, 1290, 1290) -> 2 146 689 000 (below), (1291, 1290, 1290) -> 2 148 353 100 (above)
    for n0 in (1288, 1289, 1290, 1291, 1292):
        cases.append(([0.0, 0.0, 0.0], [n0 - 0.5, 1289.5, 1289.5], 1.0))
    cases.append(([0.0, 0.0, 0.0], [46340.5, 46339.5, 0.0], 1.0))  # 46341 * 46340 = 2 147 441 940 (below)
    cases.append(([0.0, 0.0, 0.0], [46340.5, 46340.5, 0.0], 1.0))  # 46341^2 = 2 147 488 281 (above)
    cases.append(([0.0, 0.0, 0.0], [2147483000.0, 0.0, 0.0], 1.0)) # one factor alone just below 2^31
    cases.append(([0.0, 0.0, 0.0], [2147483000.0, 1.5, 0.0], 1.0))
    # an extent of >= 2^31 cells on one axis: pass-through outright (the product would overflow 64 bits with three such)
    cases.append(([0.0, 0.0, 0.0], [3.0e9, 1.0, 1.0], 1.0))
    cases.append(([-1e5, -1e5, -1e5], [1e5, 1e5, 1e5], 1e-6))
    cases.append(([-3e38, 0.0, 0.0], [3e38, 1.0, 1.0], 0.008))     # mx - mn overflows float
    cases.append(([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 1e-42))        # 1 / leaf = inf
    # a small cloud at x ~ 1e9 with leaf 0.008: no pass-through, floor(x / leaf) beyond int32
    cases.append(([1.0e9, 0.0, 0.0], [1.0e9 + 64.0, 0.1, 0.1], 0.008))
    cases.append(([-1.0e9, 0.0, 0.0], [-1.0e9, 0.1, 0.1], 0.008))
    cases.append(([1.0e7, 0.0, 0.0], [1.0e7 + 1.0, 0.1, 0.1], 0.008))      # far, but inside int32
    for leaf in (0.0, -0.008, float("nan"), float("inf"), 1e-60):
        cases.append(([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], leaf))
    cases.append(([1.0, 0.0, 0.0], [0.0, 1.0, 1.0], 0.008))        # mn > mx
    cases.append(([0.0, float("nan"), 0.0], [1.0, 1.0, 1.0], 0.008))
    return cases


def test_voxel_grid_dims_is_voxel_refs_grid(B):
    seen = {"grid": 0, "nodown": 0, "far": 0, "bad": 0}
    for mn, mx, leaf in _dims_cases():
        mn32 = np.asarray(mn, dtype=np.float32); mx32 = np.asarray(mx, dtype=np.float32)
        try:
            want = R.grid(mn32, mx32, leaf)
        except (R.TooFar, R.BadGrid) as e:
            with pytest.raises(B.TdloError) as ei:
                B.voxel_grid_dims(mn32, mx32, leaf)
            assert ei.value.code == TDLO_E_INVALID, (mn, mx, leaf)
            seen["far" if isinstance(e, R.TooFar) else "bad"] += 1
            continue
        min_b, div_b, nodown = B.voxel_grid_dims(mn32, mx32, leaf)
        assert nodown == want[2], (mn, mx, leaf)
        np.testing.assert_array_equal(min_b.astype(np.int64), want[0], err_msg=str((mn, mx, leaf)))
        np.testing.assert_array_equal(div_b.astype(np.int64), want[1], err_msg=str((mn, mx, leaf)))
        seen["nodown" if nodown else "grid"] += 1
    assert seen["grid"] >= 200 and seen["nodown"] >= 8 and seen["far"] == 2 and seen["bad"] == 7, seen


def test_voxel_grid_dims_the_named_cases(B):
    """The cases of the contract by their outcome, without the reference in between."""
    assert B.voxel_grid_dims([0, 0, 0], [1289.5, 1289.5, 1289.5], 1.0)[2] is False
    assert B.voxel_grid_dims([0, 0, 0], [1290.5, 1289.5, 1289.5], 1.0)[2] is True
    assert B.voxel_grid_dims([0, 0, 0], [3.0e9, 1.0, 1.0], 1.0)[2] is True
    min_b, div_b, nodown = B.voxel_grid_dims([-0.02, 0.008, 0.0], [0.02, 0.008, 0.0], 0.008)
    assert not nodown and list(min_b) == [-3, 1, 0] and list(div_b) == [6, 1, 1]
    for bad in (([1.0e9, 0, 0], [1.0e9, 0.1, 0.1], 0.008), ([0, 0, 0], [1, 1, 1], 0.0), ([0, 0, 0], [1, 1, 1], -1.0), ([0, 0, 0], [1, 1, 1], float("nan"))):
        with pytest.raises(B.TdloError):
            B.voxel_grid_dims(*bad)
    assert B.load_library().tdlo_voxel_grid_dims(None, None, 0.008, None, None, None) == TDLO_E_INVALID


def test_the_binding_declares_the_view_calls(B):
    lib = B.load_library()
    for name in ("tdlo_voxel_grid_dims", "tdlo_cloud_view_voxel_grid", "tdlo_tracker_frame_from_cloud_view"):
        assert name in B.SYMBOLS and hasattr(lib, name)
    assert hasattr(B.Context, "voxel_grid_view") and hasattr(B.trackdlo, "frame_from_cloud_view")
