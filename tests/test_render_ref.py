"""The numpy statement of the tracking-result image (tests/render_ref.py) against facts checked by hand, and the library's host half
(tdlo_render_primitives, no GPU) against it, record for record.  Also confirms that the inputs of tests/test_render_gpu.py pass the reference's guards."""
import numpy as np
import pytest

import render_cases as K
import render_ref as R
from trackdlo_amd import binding as B

BLACK = np.zeros((40, 40, 3), dtype=np.uint8)


def _count(rec, rows=40, cols=40):
    img = R.paint(np.zeros((rows, cols, 3), dtype=np.uint8), np.asarray([rec], dtype=np.int32))
    return int(np.count_nonzero(img.any(axis=2)))


def test_a_radius_7_disc_holds_149_pixels():
    assert _count([1, 20, 20, 20, 20, 7, 0xffffff, 0]) == 149


def test_a_width_5_line_of_ten_pixels_holds_71():
    assert _count([0, 10, 10, 20, 10, 5, 0xffffff, 0]) == 71


def test_a_zero_length_width_5_line_holds_21():
    assert _count([0, 15, 15, 15, 15, 5, 0xffffff, 0]) == 21


def test_primitives_are_clipped_to_the_image():
    assert _count([1, 0, 0, 0, 0, 7, 0xffffff, 0]) == sum(1 for x in range(8) for y in range(8) if x * x + y * y <= 49)
    assert _count([1, -100, -100, -100, -100, 7, 0xffffff, 0]) == 0


def test_the_blend_is_addweighted_for_all_byte_pairs():
    c = K.all_byte_pairs()
    a = c["colour"].astype(np.float64); o = c["occluder"].astype(np.int64)
    want = np.rint((a + (c["colour"].astype(np.int64) & o[..., None])) / 2).astype(np.uint8)       # np.rint: ties to even
    assert np.array_equal(R.blend(c["colour"], c["occluder"]), want)
    s = np.arange(511)
    assert np.array_equal((s >> 1) + ((s & 1) & ((s >> 1) & 1)), np.rint(s / 2).astype(np.int64))
    assert np.array_equal(R.blend(c["colour"], None), c["colour"])


def test_the_last_covering_primitive_per_pixel_equals_the_painters_order():
    c = K.crossing()["mixed"]
    c = dict(c, colour=c["colour"][:40, :40], occluder=c["occluder"][:40, :40])
    prims = R.primitives(c["Y"], c["proj"], c["vis"])
    want, _ = R.render(c["colour"], c["occluder"], c["Y"], c["proj"], c["vis"])
    got = R.blend(c["colour"], c["occluder"])
    covered = 0
    for r in range(40):
        for col in range(40):
            for rec in prims[::-1]:
                if R.covers(rec, np.int64(col), np.int64(r)):
                    w = int(rec[6]); got[r, col] = (w & 255, (w >> 8) & 255, (w >> 16) & 255); covered += 1
                    break
    assert covered > 200 and np.array_equal(got, want)


@pytest.mark.parametrize("vis, line, first, second", [([], "edge_hidden", "node_hidden", "node_hidden"), ([0], "edge_visible", "node_visible", "node_hidden"),
                                                      ([1], "edge_visible", "node_hidden", "node_visible"), ([0, 1], "edge_visible", "node_visible", "node_visible")])
def test_the_colour_table(vis, line, first, second):
    """trackdlo_node.cpp:409-440: the line is red only when neither end node is in vis."""
    params = dict(node_visible=(1, 2, 3), node_hidden=(4, 5, 6), edge_visible=(7, 8, 9), edge_hidden=(10, 11, 12))
    Y = R.nodes_from_pixels([(5, 5), (30, 20)], K.FX)
    p = R.primitives(Y, K.PROJ, vis, params)
    assert [int(w) for w in p[:, 6]] == [R._word(params[k]) for k in (line, first, second)] and list(p[:, 0]) == [0, 1, 1]
    if vis == []:
        d = R.primitives(Y, K.PROJ, vis)
        assert [int(w) for w in d[:, 6]] == [0xff0000, 0xff0000, 0xff0000] and list(d[:, 5]) == [5, 7, 7]      # the reference's red, in bgr8 order
        assert R._word(R.DEFAULTS["node_visible"]) == (0 | 150 << 8 | 255 << 16) and R._word(R.DEFAULTS["edge_visible"]) == 255 << 8


# ---- the host half against the reference ---------------------------------------------------------------------------------------------------------------
def _random_rope(rng, M):
    """A rope of M nodes about a metre from a 640 x 480 camera, wandering enough to cross itself; returns (Y, proj)."""
    step = rng.normal(0.0, 0.03, size=(M, 3))
    Y = np.cumsum(step, axis=0) + np.array([0.0, 0.0, 0.9 + 0.4 * rng.random()])
    return np.asfortranarray(Y), R.pinhole(615.0, 615.0, 320.0, 240.0)


def test_render_primitives_on_200_random_ropes():
    rng = np.random.default_rng(7001)
    total = 0
    for _ in range(200):
        M = int(rng.integers(2, 65))
        Y, proj = _random_rope(rng, M)
        vis = np.flatnonzero(rng.random(M) < 0.6).astype(np.int32)
        params = None
        if rng.random() < 0.5:
            params = dict(line_width=int(rng.integers(1, 12)), node_radius=int(rng.integers(1, 12)), node_visible=tuple(int(v) for v in rng.integers(0, 256, 3)),
                          edge_hidden=tuple(int(v) for v in rng.integers(0, 256, 3)))
        want = R.primitives(Y, proj, vis, params)                 # (raises if a guard is violated: the seed is chosen so that none is)
        got = B.render_primitives(Y, proj, vis, B.make_render_params(**params) if params else None)
        assert got.shape == (3 * (M - 1), 8) and np.array_equal(got, want)
        total += len(got)
    assert total > 10000


def test_render_primitives_on_the_gpu_tests_inputs():
    """Every input of tests/test_render_gpu.py that can be formed without a GPU passes the guards, and the host half gives the reference's records."""
    for name, c in K.cpu_checkable().items():
        want = R.primitives(c["Y"], c["proj"], c["vis"], c["params"])
        got = B.render_primitives(c["Y"], c["proj"], c["vis"], B.make_render_params(**c["params"]) if c["params"] else None)
        assert np.array_equal(got, want), name


def test_default_params_are_the_references():
    p = B.make_render_params()
    assert (p.line_width, p.node_radius) == (5, 7)
    assert [tuple(getattr(p, k)) for k in ("node_visible", "node_hidden", "edge_visible", "edge_hidden")] == [(0, 150, 255), (0, 0, 255), (0, 255, 0), (0, 0, 255)]


@pytest.mark.parametrize("what", ["w<=0", "w<0", "nan", "inf", "col>8191", "row<-8192", "vis>=M", "vis<0", "line_width=0", "node_radius=256"])
def test_nodes_that_cannot_be_drawn(what):
    Y = R.nodes_from_pixels([(5, 5), (30, 20), (40, 40)], K.FX)
    vis, params = [0], {}
    if what == "w<=0":
        Y[1, 2] = 0.0
    elif what == "w<0":
        Y[1, 2] = -1.0
    elif what == "nan":
        Y[2, 0] = np.nan
    elif what == "inf":
        Y[0, 1] = np.inf
    elif what == "col>8191":
        Y[1] = R.nodes_from_pixels([(8192, 5)], K.FX)[0]
    elif what == "row<-8192":
        Y[1] = R.nodes_from_pixels([(5, -8193)], K.FX)[0]
    elif what == "vis>=M":
        vis = [0, 3]
    elif what == "vis<0":
        vis = [-1]
    elif what == "line_width=0":
        params = dict(line_width=0)
    else:
        params = dict(node_radius=256)
    with pytest.raises(ValueError):
        R.primitives(Y, K.PROJ, vis, params, guard=False)
    with pytest.raises(B.TdloError) as e:
        B.render_primitives(Y, K.PROJ, vis, B.make_render_params(**params))
    assert e.value.code == B.TDLO_E_INVALID


def test_the_pixel_range_is_inclusive():
    Y = R.nodes_from_pixels([(8191, -8192), (-8192, 8191)], K.FX)
    assert np.array_equal(B.render_primitives(Y, K.PROJ, [0]), R.primitives(Y, K.PROJ, [0]))
