"""CPU suite for the constructed scenes of the one-launch depth -> cloud kernels (tests/cloud_scenes.py): every scene has the property it was built for,
asserted on the reference's structure alone (voxel_ref.structure); voxel_ref equals the C oracle bit for bit on every scene; and every scene
DISCRIMINATES -- deliberately wrong numpy variants of the reference, each modelling one way the kernels can fail, differ in bits from the reference on the
scene built for that failure.  No GPU, and nothing of the library is called."""
import os
import re

import numpy as np
import pytest

import cloud_scenes as S
import colour_ref
import voxel_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _heads(st):
    return S.heads_of(st["runs"])


def _run_at(st, p):
    """[start, end) of the run that holds sorted position p."""
    h = _heads(st)
    i = int(np.searchsorted(h, p, side="right")) - 1
    return int(h[i]), int(h[i] + st["runs"][i])


# ---- the constants and rules the scenes are built on are the kernels' ---------------------------------------------------------------------------
def test_the_scene_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "trackdlo_amd", "csrc", "tdlo_cloud.hip")).read()
    seen = {}
    for name, expr in re.findall(r"constexpr int (k\w+) = ([0-9A-Za-z_ *+/()-]+);", text):
        try:
            seen[name] = int(eval(expr, {"__builtins__": {}}, dict(seen)))
        except Exception:
            pass
    for name, value in S.CONSTANTS.items():
        assert seen.get(name) == value, (name, seen.get(name), value)
    # the slice rule of the team, the thread rule and the staging switch of the single workgroup, the tile limit of both
    for rule in ("const int K = a.T < kTK ? a.T : kTK;", "const int per = ((n + K - 1) / K + 63) & ~63;", "const int R = (n + kFT - 1) / kFT;",
                 "if (3 * n <= kFNmax) {", "e_k < s0 + kTVcap ? e_k : s0 + kTVcap", "<= (size_t)kFTmax; }"):
        assert rule in text, rule
    assert 3 * 10901 <= S.kFNmax < 3 * 10902 and S.fused_R(31744) == 31 and S.fused_R(31745) == 32 and S.fused_R(1024) == 1 and S.fused_R(1025) == 2
    assert S.team_slices(S.N_FULL, 12) == (8, 4096, [0, 4096, 8192, 12288, 16384, 20480, 24576, 28672, 32704])
    assert S.team_slices(65, 12)[2] == [0, 64, 65, 65, 65, 65, 65, 65, 65] and S.team_slices(3000, 7)[:2] == (7, 448)
    assert [V.bits_for(v) for v in (1, 2, 3, 4, 5, 256, 257, 32704, 32768, 32769)] == [1, 1, 2, 2, 3, 8, 9, 15, 15, 16]


# ---- every scene has its property ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_scene_structure_and_route(name):
    s = S.get(name)
    st = s.structure
    assert s.route == S.route_rule(st, s.T), (name, s.route, st["rb"], st["kb"], st["nodown"], st["n_raw"], s.T)
    assert st["n_raw"] == np.count_nonzero(s.mask) and st["n"] == s.ref[0].shape[0] and s.ref[1] == st["n_raw"]
    if s.runs is not None:                                         # what the builder was asked for is what the reference sees
        assert np.array_equal(st["runs"], s.runs)
    assert s.mask[s.mask != 0].min() >= 1 and (S.family(name) == "G" or len(np.unique(s.mask)) > 200 or st["n_raw"] < 2000)      # mask bytes 1 .. 255


def test_A_slice_borders():
    st = S.get("A").structure
    K, per, s = S.team_slices(st["n_raw"], S.get("A").T)
    assert (st["n_raw"], K, per) == (S.N_FULL, 8, 4096)
    heads = set(_heads(st).tolist())
    assert {s[1], s[2], s[3]} <= heads                                                       # heads exactly at s1, s2, s3
    assert _run_at(st, s[2]) == (s[2], s[2] + 1)                                             # (one of them a run of one point)
    for k in (4, 5):
        assert _run_at(st, s[k]) == (s[k] - 1, s[k] + 1)                                     # crosses the slice end by a single point
    assert _run_at(st, s[6] - 1) == (s[6] - 1, s[6]) and s[6] in heads                       # a run of one point at s6 - 1, a head at s6
    a, e = _run_at(st, s[7])
    assert a == s[7] - 40 and e > s[7] + 1                                                   # slice 7 starts inside a run
    assert len(heads) > 1500 and st["runs"].max() <= 65


def test_B_long_runs():
    _, per, s = S.team_slices(S.N_FULL, 12)
    assert np.array_equal(S.get("B_i").structure["runs"], [S.N_FULL])
    st = S.get("B_ii").structure
    assert _run_at(st, 4000) == (4000, 11000) and 4000 < s[1] < 11000 and 11000 > s[0] + S.kTVcap
    st = S.get("B_iii").structure
    a, e = _run_at(st, 8186)
    assert (a, e) == (8186, 14386) and a == s[2] - 6 and a < s[2] and s[3] < e and e > s[1] + S.kTVcap       # slice 2 wholly inside, tail beyond slice 1's window
    assert _run_at(S.get("B_iv_at").structure, 4000) == (4000, s[0] + S.kTVcap)
    assert _run_at(S.get("B_iv_past").structure, 4000) == (4000, s[0] + S.kTVcap + 1)
    st = S.get("B_v").structure
    assert st["runs"].tolist() == [100, 9000, 23604]
    inside = [k for k in range(8) if _run_at(st, s[k])[0] < s[k] and _run_at(st, s[k])[1] >= s[k + 1]]
    assert inside == [1, 3, 4, 5, 6, 7]                                                      # slices without a head of their own


def test_C_sizes():
    assert S.C_SIZES == [1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 10901, 10902, 16384, 16385, 31744, 31745, 32703, 32704]
    for n in S.C_SIZES + [S.kFNmax + 1]:
        s = S.get("C_%d" % n)
        st = s.structure
        assert st["n_raw"] == n and s.T == 12 and 1 <= st["runs"].min() and st["runs"].max() <= 40
        assert n < 63 or len(np.unique(st["runs"])) >= (10 if n >= 511 else 2)               # mixed
        assert s.route == ("taken" if n <= S.kFNmax else "passed")
    st = S.get("C_distinct").structure
    assert st["n"] == st["n_raw"] == S.N_FULL
    empty = [n for n in S.C_SIZES if S.team_slices(n, 12)[2][1] == n and n > 1]              # member slices that are empty apart from n = 1
    assert empty == [2, 63, 64]


def test_D_team_sizes_and_tiles():
    rem = set()
    for T, (rows, cols) in S.D_IMAGES.items():
        for place in S.D_PLACES:
            s = S.get("D_%d_%s" % (T, place))
            assert s.T == T and s.depth.shape == (rows, cols) and S.team_slices(s.structure["n_raw"], T)[0] == min(8, T)
            per_tile = np.bincount(np.nonzero(s.mask.reshape(-1))[0] // S.kFPix, minlength=T)
            if place == "first":
                assert per_tile[0] == s.structure["n_raw"]
            elif place == "last":
                assert per_tile[T - 1] == s.structure["n_raw"] and s.mask[-1, -1] != 0
            else:
                assert (per_tile[0::2][: (T - 1) // 2 + 1] > 0).all() and per_tile[1::2][: (T - 1) // 2].sum() == 0 and s.mask[-1, -1] != 0
                if T >= 7:
                    toff = np.concatenate([[0], np.cumsum(per_tile)])
                    assert (np.diff(toff) == 0).sum() >= 2                                  # empty tiles: equal offsets in the search
            if place != "first":
                rem.add(s.P % 4)
    assert sorted(S.D_IMAGES) == [1, 2, 7, 8, 9] and {1, 2, 3} <= rem


def test_E_many_tiles():
    s = S.get("E_1026")
    assert s.depth.shape == (2048, 2051) and s.T == 1026 and s.T > S.kFT
    assert sorted(set((np.nonzero(s.mask.reshape(-1))[0] // S.kFPix).tolist())) == [0, 1023, 1024, 1025]
    s = S.get("E_max")
    assert s.P == S.kFTmax * S.kFPix and s.T == S.kFTmax and s.route == "taken"
    s = S.get("E_over")
    assert s.P == S.kFTmax * S.kFPix + 1 and s.T == S.kFTmax + 1 and s.route == "untouched" and s.mask.reshape(-1)[-1] != 0


def test_F_word_layout():
    for kb in (1, 4, 5, 8, 9, 16, 17):
        st = S.get("F_kb%d" % kb).structure
        assert st["kb"] == kb and st["rb"] + kb <= 32 and st["cells"] > 1
    a, b = S.get("F_rbkb32"), S.get("F_rbkb33")
    assert a.structure["rb"] + a.structure["kb"] == 32 and a.route == "taken"
    assert b.structure["rb"] + b.structure["kb"] == 33 and b.route == "passed" and not b.structure["nodown"]


def test_G_values():
    st = S.get("G_wall").structure
    assert st["min_b"][0] < 0 and st["min_b"][1] < 0 and (st["div_b"] > 10).all() and st["runs"].max() > 8
    s = S.get("G_far")
    assert s.depth[s.mask != 0].max() == 65535 and s.structure["n"] > 1000
    for name in ("G_zero", "G_zero_pass"):
        s = S.get(name)
        zero = s.note["zero"]
        i, j = np.nonzero(zero)
        assert j.max() < s.cam[2] and i.max() < s.cam[3] and (s.mask[zero] != 0).all() and (s.depth[zero] == 0).all() and (s.depth[(s.mask != 0) & ~zero] > 0).all()
        Q = s.points()
        zq = Q[zero[s.mask != 0]]
        assert np.array_equal(zq.view(np.uint32), np.tile(np.array([0x80000000, 0x80000000, 0], dtype=np.uint32), (len(zq), 1)))      # -0.0f, -0.0f, +0.0f
        X = s.ref[0]
        if name == "G_zero":
            allzero = np.nonzero((_bits(X) == 0).all(axis=1))[0]
            assert len(allzero) == 1 and not (X[np.arange(len(X)) != allzero[0]] == 0).all(axis=1).any()      # the cell of the zero pixels: +0.0, +0.0, 0.0, and nothing else in it
            assert s.structure["runs"].max() == zero.sum()
        else:
            assert s.structure["nodown"] and X.shape[0] == s.structure["n_raw"]
            rows = X[zero[s.mask != 0]]
            assert np.array_equal(_bits(rows), np.tile(np.array([1 << 63, 1 << 63, 0], dtype=np.uint64), (len(rows), 1)))          # the points come back with their sign bits


# ---- the reference is the oracle on every scene -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", "ABCDEFG")
def test_voxel_ref_is_the_oracle_on_every_scene(oracle, fam):
    for name in S.NAMES:
        if S.family(name) != fam:
            continue
        s = S.get(name)
        Xo, nraw_o = oracle.depth_to_cloud(np.asarray(s.depth), np.asarray(s.mask), *s.cam, s.leaf)
        assert nraw_o == s.ref[1] and _same(np.ascontiguousarray(Xo), s.ref[0]), name


# ---- wrong variants of the reference: each one way the kernels can fail -------------------------------------------------------------------------
def _parts(s):
    Q = s.points()
    _, _, nodown, key, order, cell = V.group(Q, s.leaf)
    assert not nodown
    return Q, key, order, cell


def _cells_from_heads(head):
    return np.cumsum(head) - 1


def _slice_of(p, s):
    _, per, _ = S.team_slices(s.structure["n_raw"], s.T)
    return p // per


def v_reverse(s):
    """A run summed in reverse order."""
    Q, key, order, cell = _parts(s)
    return V.centroids(Q[order][::-1], cell[::-1])


def v_from_first(s):
    """A run's sums started from its first element instead of from zero."""
    Q, key, order, cell = _parts(s)
    Qs = Q[order]
    head = np.ones(len(cell), dtype=bool); head[1:] = cell[1:] != cell[:-1]
    sums = Qs[head].copy()
    np.add.at(sums, cell[~head], Qs[~head])
    cnt = np.bincount(cell).astype(F)
    return (sums / cnt[:, None]).astype(np.float64)


def v_truncated(s):
    """A run whose head lies in slice k summed only up to s_k + kTVcap (the points beyond the staging window lost; the count kept)."""
    Q, key, order, cell = _parts(s)
    Qs = Q[order].copy()
    _, per, sl = S.team_slices(len(Qs), s.T)
    h = _heads(s.structure)
    limit = (h // per) * per + S.kTVcap                              # per run
    pos = np.arange(len(Qs))
    Qs[pos >= limit[cell]] = 0.0                                     # (+0.0 added to a positive sum leaves it as it is)
    return V.centroids(Qs, cell)


def _crossing(s):
    """Per run: does it cross a slice end (start < s_k < end)?"""
    st = s.structure
    _, per, sl = S.team_slices(st["n_raw"], s.T)
    h = _heads(st); e = h + st["runs"]
    return (h // per) != ((e - 1) // per)


def v_crossing_dropped(s):
    return s.ref[0][~_crossing(s)]


def v_split(s):
    """A head forced at every slice's first position: the run that crosses a slice end split at the border."""
    Q, key, order, cell = _parts(s)
    _, per, sl = S.team_slices(len(cell), s.T)
    head = np.ones(len(cell), dtype=bool); head[1:] = cell[1:] != cell[:-1]
    head[[p for p in sl[1:-1] if p < len(cell)]] = True
    return V.centroids(Q[order], _cells_from_heads(head))


def v_suppressed(s):
    """A head at a slice's first position suppressed: the run joins the one in front."""
    Q, key, order, cell = _parts(s)
    _, per, sl = S.team_slices(len(cell), s.T)
    head = np.ones(len(cell), dtype=bool); head[1:] = cell[1:] != cell[:-1]
    head[[p for p in sl[1:-1] if p < len(cell)]] = False
    return V.centroids(Q[order], _cells_from_heads(head))


def v_carry_dropped(s):
    """The tile offsets' carry dropped after 1024 tiles: the offsets of the tiles 1024 .. start from 0 again; every rank's point is looked up by the
    kernels' binary search over those offsets (a rank that lands outside its tile's points reads zeros)."""
    m = np.asarray(s.mask).reshape(-1) != 0
    T = s.T
    tcnt = np.bincount(np.nonzero(m)[0] // S.kFPix, minlength=T)
    toff = np.zeros(T + 1, dtype=np.int64)
    for b0 in range(0, T, S.kFT):
        c = tcnt[b0:b0 + S.kFT]
        toff[b0:b0 + len(c)] = np.cumsum(c) - c
    n = int(tcnt.sum())
    toff[T] = n
    true_off = np.concatenate([[0], np.cumsum(tcnt)])
    Q = s.points()
    g = np.arange(n)
    lo = np.zeros(n, dtype=np.int64); hi = np.full(n, T, dtype=np.int64)
    while (hi - lo > 1).any():
        mid = (lo + hi) >> 1
        go = (toff[mid] <= g) & (hi - lo > 1)
        stay = ~go & (hi - lo > 1)
        lo = np.where(go, mid, lo); hi = np.where(stay, mid, hi)
    idx = g - toff[lo]
    ok = (idx >= 0) & (idx < tcnt[lo])
    Qw = np.zeros_like(Q)
    Qw[ok] = Q[true_off[lo[ok]] + idx[ok]]
    return V.voxel_ref(Qw, None, s.leaf)[0]


def v_full_last_digit(s):
    """A sort word that carries the rank ABOVE the cell index (rank << kb | key), sorted by 8-bit digits with the last digit taken with a full mask: with kb
    no multiple of 8 the last digit holds rank bits, and the points are ordered by them."""
    Q, key, order, cell = _parts(s)
    kb = s.structure["kb"]
    word = (np.arange(len(key), dtype=np.int64) << kb) | key
    o = np.argsort(word & ((1 << (8 * ((kb + 7) // 8))) - 1), kind="stable")
    ks = key[o]
    head = np.ones(len(ks), dtype=bool); head[1:] = ks[1:] != ks[:-1]
    return V.centroids(Q[o], _cells_from_heads(head))


def v_unstable(s):
    """An unstable sort: equal keys in descending input order."""
    Q, key, order, cell = _parts(s)
    o = np.lexsort((-np.arange(len(key)), key))
    return V.centroids(Q[o], cell)


CAUGHT = [
    (v_reverse, ["B_i", "B_ii", "B_iii", "B_v", "C_32704", "A"]),
    (v_from_first, ["G_zero"]),
    (v_truncated, ["B_i", "B_ii", "B_iii", "B_iv_past", "B_v"]),
    (v_crossing_dropped, ["A", "B_ii", "B_iii", "B_iv_at", "B_v"]),
    (v_split, ["A", "B_ii", "B_iii", "B_iv_at", "B_v", "B_i"]),
    (v_suppressed, ["A"]),
    (v_carry_dropped, ["E_1026"]),
    (v_full_last_digit, ["F_kb1", "F_kb4", "F_kb5", "F_kb9", "F_kb17"]),
    (v_unstable, ["B_i", "B_v", "A", "C_32704"]),
]
NOT_CAUGHT = [
    (v_truncated, ["B_iv_at", "A"]),                 # a run that ends exactly at the window's end loses nothing: the border is sharp
    (v_full_last_digit, ["F_kb8", "F_kb16"]),        # whole digits: a full mask is the right one
    (v_from_first, ["A", "B_i"]),                    # without a -0.0 the first element and 0 + the first element are the same float
    (v_carry_dropped, ["D_9_alternate"]),            # up to 1024 tiles there is no carry
    (v_suppressed, ["B_i"]),                         # no head at any slice's first position to suppress
]


@pytest.mark.parametrize("variant,names", CAUGHT, ids=[v.__name__ for v, _ in CAUGHT])
def test_every_wrong_variant_is_caught_by_its_scene(variant, names):
    for name in names:
        s = S.get(name)
        assert not _same(variant(s), s.ref[0]), (variant.__name__, name)


@pytest.mark.parametrize("variant,names", NOT_CAUGHT, ids=[v.__name__ for v, _ in NOT_CAUGHT])
def test_the_variants_are_wrong_only_where_they_model_a_fault(variant, names):
    for name in names:
        s = S.get(name)
        assert _same(variant(s), s.ref[0]), (variant.__name__, name)


def test_every_taken_scene_of_A_B_is_caught_by_some_variant():
    """No scene of the border families is one the listed faults pass through unseen."""
    for name in ("A", "B_i", "B_ii", "B_iii", "B_iv_at", "B_iv_past", "B_v"):
        s = S.get(name)
        assert any(not _same(v(s), s.ref[0]) for v in (v_reverse, v_truncated, v_split, v_unstable)), name


# ---- the colour scenes' painting reproduces the wanted mask -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "D_7_last"])
def test_the_painted_colour_image_gives_the_wanted_mask(name):
    s = S.get(name)
    colour, occ, lower, upper = S.paint(s, seed=900)
    want = (np.asarray(s.mask) != 0)
    got = colour_ref.colour_mask(colour, lower, upper, 0, occ)
    assert np.array_equal(got != 0, want) and set(np.unique(got)) <= {0, 255}
    hsv = colour_ref.bgr_to_hsv(colour)
    inr = colour_ref.in_ranges(hsv, lower, upper) != 0
    assert (inr & ~want).sum() > 20 and ((occ == 0) & inr).sum() == (inr & ~want).sum()      # in-range pixels behind an occluder byte of 0
    out = ~inr
    lo, hi = np.asarray(lower[0]), np.asarray(upper[0])
    d = np.maximum(lo - hsv[out].astype(int), hsv[out].astype(int) - hi).max(axis=1)
    assert (d == 1).all()                                                                    # every other pixel one unit outside, in H, S or V
    assert all(((hsv[out][:, c].astype(int) < lo[c]) | (hsv[out][:, c].astype(int) > hi[c])).any() for c in range(3))
