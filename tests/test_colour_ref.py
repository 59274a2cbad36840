"""CPU suite for the colour segmentation (tdlo_colour_*): the numpy statement tests/colour_ref.py against itself -- spot values, the textbook formula to
within one unit over all 2^24 colours, and the two difference counts that fingerprint the table arithmetic (a rounded float implementation has neither)
-- and the built library: every new symbol exported, a bad range count refused."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as R


@pytest.fixture(scope="module")
def cube_hsv():
    c = R.cube()
    return c, R.bgr_to_hsv(c)


def test_spot_values():
    for bgr, hsv in (((255, 0, 0), (120, 255, 255)), ((0, 255, 255), (30, 255, 255)), ((7, 7, 7), (0, 0, 7)), ((12, 200, 77), (50, 240, 200))):
        assert tuple(int(x) for x in R.bgr_to_hsv(np.array(bgr, dtype=np.uint8))) == hsv
        assert tuple(int(x) for x in R.bgr_to_hsv(np.array(bgr[::-1], dtype=np.uint8), rgb_order=1)) == hsv
    sdiv, hdiv = R.tables()
    assert sdiv[0] == hdiv[0] == 0 and sdiv[1] == 255 << 12 and hdiv[1] == 30 << 12 and sdiv[255] == 4096 and hdiv[255] == 482


def test_whole_cube_against_the_textbook_formula(cube_hsv):
    c, hsv = cube_hsv
    h = hsv[..., 0].astype(np.float64); s = hsv[..., 1].astype(np.float64)
    assert hsv[..., 0].max() == 179
    assert np.array_equal(hsv[..., 2], c.max(axis=-1))
    H, S = R.textbook(c)
    assert np.abs(s - S).max() < 1.0
    dh = np.abs(h - H); dh = np.minimum(dh, 180.0 - dh)
    assert dh.max() < 1.0
    # the fingerprint of the table arithmetic: where it differs from the rounded textbook value
    hr = np.rint(H); hr = np.where(hr >= 180.0, hr - 180.0, hr)
    assert int(np.count_nonzero(s != np.rint(S))) == 199146
    assert int(np.count_nonzero(h != hr)) == 368109


def test_launch_range_share_of_the_cube(cube_hsv):
    _, hsv = cube_hsv
    m = R.in_ranges(hsv, *R.LAUNCH_RANGE)
    assert set(np.unique(m)) == {0, 255}
    assert abs(100.0 * np.count_nonzero(m) / m.size - 19.956) < 5e-4
    # a range with lower == upper passes exactly the colours with that HSV value; a range with lower > upper passes nothing
    one = R.in_ranges(hsv, [[50, 240, 200]], [[50, 240, 200]])
    assert one.reshape(-1)[12 | 200 << 8 | 77 << 16] == 255 and np.array_equal(one != 0, np.all(hsv == np.array([50, 240, 200], dtype=np.uint8), axis=-1))
    assert not R.in_ranges(hsv[:64], [[100, 0, 0]], [[90, 255, 255]]).any()


def test_colour_scene_is_what_it_says():
    from trackdlo_amd import synth
    for ranges, occ, order in ((R.LAUNCH_RANGE, None, 0), (R.MULTI_RANGES, (200, 260, 300, 340), 0), (R.LAUNCH_RANGE, (0, 50, 0, 20), 1)):
        depth, colour, occl, mask, cam, _ = synth.colour_scene(30, *ranges, config=9, frame=2, occluder=occ, rgb_order=order, razor=0.25)
        d0, rope, _, _ = synth.depth_scene(30, config=9, frame=2)
        assert np.array_equal(depth, d0) and colour.shape == rope.shape + (3,) and colour.dtype == np.uint8
        assert np.array_equal(R.colour_mask(colour, *ranges, rgb_order=order), rope)          # rope pixels pass, every other pixel fails
        assert np.array_equal(R.colour_mask(colour, *ranges, rgb_order=order, occluder=occl), mask)
        assert (occl is None) == (occ is None) and (occ is None or np.count_nonzero(mask) < np.count_nonzero(rope) or not rope[occ[0]:occ[1], occ[2]:occ[3]].any())
        # the stated share of razor colours, on both sides
        hsv = R.bgr_to_hsv(colour, order).astype(np.int64)
        b = np.concatenate([np.asarray(ranges[0]), np.asarray(ranges[1])]).reshape(-1, 3)
        edge = np.any(np.abs(hsv[:, :, None, :] - b[None, None, :, :]) <= 1, axis=(2, 3))
        assert abs(edge[rope != 0].mean() - 0.25) < 0.03 and abs(edge[rope == 0].mean() - 0.25) < 0.01


def test_library_exports_the_colour_calls_and_refuses_a_bad_range_count():
    from trackdlo_amd import binding as B
    lib = B.load_library()
    for name in ("tdlo_colour_mask", "tdlo_colour_buffers", "tdlo_colour_depth_to_cloud", "tdlo_colour_depth_to_cloud_visibility", "tdlo_tracker_frame_from_colour"):
        assert hasattr(lib, name) and name in B.SYMBOLS
    img = np.zeros((2, 4, 3), dtype=np.uint8); out = np.zeros((2, 4), dtype=np.uint8)
    for n in (0, 5):
        p = B.make_colour_params()
        p.n_ranges = n
        assert lib.tdlo_colour_mask(None, img.ctypes.data_as(C.c_void_p), 2, 4, C.byref(p), None, out.ctypes.data_as(C.c_void_p), None) == B.TDLO_E_INVALID
    with pytest.raises(ValueError):
        B.make_colour_params([[0, 0, 0]] * 5, [[1, 1, 1]] * 5)
    p = B.make_colour_params(*B.COLOUR_MULTI, rgb_order=1)
    assert p.n_ranges == 4 and p.rgb_order == 1 and list(p.lower[1]) == [130, 60, 50] and list(p.upper[3]) == [40, 255, 255]
    assert (B.COLOUR_LAUNCH, B.COLOUR_MULTI) == (R.LAUNCH_RANGE, R.MULTI_RANGES)
