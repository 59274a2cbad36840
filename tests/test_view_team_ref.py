"""CPU suite for the one-launch voxel grid on cloud views (k_cloud_team's view instantiations, trackdlo_amd/csrc/tdlo_cloud.hip).

1. The scene catalogue of tests/cloud_scenes.py read as ORGANIZED CLOUDS + SELECTION: every pixel back-projected, the mask as the selection bytes.  The
   numpy statement V (tests/voxel_ref.py) of that view is the scene's reference bit for bit, and the header's route rule on its structure is the scene's
   route -- so tests/test_view_team_gpu.py may hold the view route to the catalogue.
2. The lane of phase A over a view (csrc/tdlo_view_lane.h, the very code the GPU runs) compiled for the host into tests/cpp/view_lane_host_test.cpp with
   -fsanitize=address,undefined and run as a child process (nothing is loaded into python): every lane of every tile, on views and selection buffers
   allocated at exactly their extents, against the element-by-element statement below."""
import os
import subprocess

import numpy as np
import pytest

import cloud_scenes as S
import voxel_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC, XYZ12, COLS2 = 0, 1, 2                                     # ImportForm (csrc/tdlo_view_load.h)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def organized(s):
    """The scene as an organized float32 cloud [P x 3] (every pixel back-projected, row-major) and its selection bytes [P]."""
    return V.backproject(s.depth, np.ones_like(s.mask), *s.cam), np.asarray(s.mask).reshape(-1)


@pytest.mark.parametrize("name", [n for n in S.NAMES if n not in S.LARGE])
def test_the_scene_as_an_organized_cloud_is_the_scene(name):
    s = S.get(name)
    org, sel = organized(s)
    assert org.shape == (s.P, 3) and np.isfinite(org).all()
    X, n_raw = V.voxel_ref(org, sel, s.leaf)
    assert n_raw == s.ref[1] and X.shape == s.ref[0].shape and np.array_equal(_bits(X), _bits(s.ref[0]))
    assert S.route_rule(V.structure(org, sel, s.leaf), s.T) == s.route
    # compacted (the masked points, no selection) it is the scene's own reference; fewer tiles, the same rule
    assert S.route_rule(s.structure, S.tiles(max(s.ref[1], 1))) == s.route


def test_the_header_lists_the_view_route_and_its_counters():
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    assert "int tdlo_cloud_view_voxel_grid_visibility(tdlo_ctx *ctx, int slot, const tdlo_cloud_view *v, int N, const unsigned char *select, double leaf_size," in text
    assert " * 27 / 28: tdlo_cloud_view_voxel_grid calls" in text and "29: view frames whose visibility pre-pass rode" in text
    from trackdlo_amd import binding as B
    lib = B.load_library()
    assert hasattr(lib, "tdlo_cloud_view_voxel_grid_visibility") and "tdlo_cloud_view_voxel_grid_visibility" in B.SYMBOLS
    assert hasattr(B.Context, "voxel_grid_view_visibility") and hasattr(B.Context, "view_route_counts")


# ---- the lane ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 4095, 4096, 4097)


def _values(N, dtype, rng):
    """N points: a tenth with a NaN or an infinity in one component; float64: another tenth beyond float range (+-1e300, and the first double that rounds
    to +inf) -- whether selected or not is the selection's draw."""
    P = rng.standard_normal((N, 3)).astype(dtype)
    bad = rng.random(N) < 0.1
    P[bad, rng.integers(0, 3, N)[bad]] = rng.choice(np.array([np.nan, np.inf, -np.inf]), N)[bad].astype(dtype)
    if dtype == np.float64:
        big = rng.random(N) < 0.1
        P[big, rng.integers(0, 3, N)[big]] = rng.choice(np.array([1e300, -1e300, 3.4028235677973366e38, -3.5e38]), N)[big]
        ok = rng.random(N) < 0.05
        P[ok, 0] = 3.4028234e38                                   # (below FLT_MAX: stays finite)
    return P


def _layouts(N):
    """(dtype, stride_point, stride_comp, lead bytes in front of the extent, form): strides 3 / 4 / 8, column-major with even and odd leading dimension,
    views whose data is not 8-byte aligned, reversed and odd strides, float64."""
    ld = N + 5
    ev, od = ld + ld % 2, ld + 1 - ld % 2
    f, d = np.float32, np.float64
    return [(f, 3, 1, 0, XYZ12), (f, 4, 1, 0, XYZ12), (f, 8, 1, 0, XYZ12), (f, 3, 1, 4, XYZ12), (f, 4, 1, 4, XYZ12),
            (f, 1, ev, 0, COLS2), (f, 1, N + N % 2, 0, COLS2), (f, 1, ev, 8, COLS2), (f, 1, od, 0, GENERIC), (f, 1, ev, 4, GENERIC),
            (f, -3, 1, 0, GENERIC), (f, 1, -ld, 0, GENERIC), (f, 5, 2, 0, GENERIC),
            (d, 3, 1, 0, GENERIC), (d, 1, N, 0, GENERIC), (d, -4, 1, 8, GENERIC), (d, 8, 1, 0, GENERIC)]


def _cases():
    rng = np.random.default_rng(2718)
    out = []
    for N in SIZES:
        for dtype, sp, sc, lead, form in _layouts(N):
            idx = np.arange(N)[:, None] * sp + np.arange(3)[None, :] * sc
            lo, hi = int(idx.min()), int(idx.max()) + 1
            if sp == 1 and abs(sc) < N:
                continue                                            # (columns would overlap)
            for sel_off in (-1, 0, 1, 2, 3):
                P = _values(N, dtype, rng)
                flat = np.full(hi - lo, np.nan, dtype=dtype)
                flat[idx - lo] = P
                sel = None if sel_off < 0 else ((rng.random(N) < 0.7) * rng.integers(1, 256, N)).astype(np.uint8)
                out.append(dict(N=N, dtype=dtype, sp=sp, sc=sc, lead=lead, form=form, data_off=-lo, flat=flat, sel_off=sel_off, sel=sel, P=P))
    return out


def _statement(case):
    """Element by element: kept iff selected (no selection: every element) and three finite floats after the conversion; the floats of the kept, 0 elsewhere."""
    P32 = V.to_float(case["P"])
    kept = V.kept(P32, case["sel"])
    return kept.astype(np.uint8), np.where(kept[:, None], P32, np.float32(0.0)).astype(np.float32)


def test_the_lane_compiled_for_the_host(tmp_path):
    exe = str(tmp_path / "view_lane_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", "view_lane_host_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = _cases()
    blob = [np.array([len(cases)], dtype=np.int64).tobytes()]
    for c in cases:
        blob.append(np.array([c["dtype"] == np.float64, c["form"], c["N"], c["sp"], c["sc"], c["data_off"], c["flat"].size, c["lead"], c["sel_off"]], dtype=np.int64).tobytes())
        blob.append(c["flat"].tobytes())
        if c["sel"] is not None:
            blob.append(c["sel"].tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases run" in r.stdout, r.stdout
    counts = [int(x) for x in r.stdout.split(":")[-1].split()]
    assert len(counts) == 4 and min(counts) >= 100, r.stdout        # all four forms
    got = (tmp_path / "out.bin").read_bytes()
    at, dropped_selected, dropped_range = 0, 0, 0
    for c in cases:
        N = c["N"]
        kept, xyz = _statement(c)
        what = (N, c["dtype"].__name__, c["sp"], c["sc"], c["lead"], c["form"], c["sel_off"])
        assert got[at:at + N] == kept.tobytes(), what
        assert got[at + N:at + 13 * N] == xyz.tobytes(), what
        at += 13 * N
        chosen = np.ones(N, bool) if c["sel"] is None else c["sel"] != 0
        dropped_selected += int((chosen & ~kept.astype(bool)).sum())
        if c["dtype"] == np.float64:
            dropped_range += int((chosen & np.isfinite(c["P"]).all(axis=1) & ~kept.astype(bool)).sum())
    assert at == len(got)
    assert dropped_selected > 1000 and dropped_range > 300          # non-finite points among the selected, doubles beyond float range among them
