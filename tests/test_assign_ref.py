"""One cloud dealt out among F ropes without a GPU: the host call tdlo_cloud_assign_host equals the statement (tests/assign_ref.py) in owner, d2 bits and counts
on every scene; four wrong readings of the statement are each told from it on a scene built for that, the distinguishing property asserted on the reference;
the reference's fused multiply-add is held to the Fraction form; the lane runs over a whole (block, tile) grid in a sanitized stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from trackdlo_amd import binding as B
import assign_ref as AR
import prepass_ref as PR

NEW = ["tdlo_cloud_assign", "tdlo_cloud_assign_visibility", "tdlo_cloud_assign_host", "tdlo_tracker_frames_from_shared_cloud_batch"]


def host_equals_statement(X, ropes, d_max):
    own, d2, n_each, un = B.cloud_assign_host(X, ropes, d_max)
    ro, rg, rn, ru = AR.assign(X, ropes, d_max)
    assert np.array_equal(own, ro) and np.array_equal(AR.bits(d2), AR.bits(rg)) and n_each == rn and un == ru
    return ro, rg


def test_the_new_names_are_declared_required_and_exported():
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert "tdlo_assign_rope;" in hdr and lib.tdlo_abi_version() == 3
    f = B.AssignRopeC
    assert B.C.sizeof(f) == 24 and (f.slot.offset, f.Y.offset, f.M.offset) == (0, 8, 16)
    assert lib.tdlo_debug_route_count(None, 53) == -1 and lib.tdlo_debug_route_count(None, 54) == -1
    assert re.search(r"\* 53 / 54: calls of tdlo_cloud_assign", text)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "tdlo_cloud_assign" in open(os.path.join(ROOT, doc)).read(), doc


def test_the_reference_fma_is_the_fraction_form():
    rng = np.random.default_rng(8)
    for _ in range(2000):
        a, b, c = (float(v) for v in rng.normal(0, 1, 3) * 10.0 ** rng.integers(-8, 3, 3))
        assert AR.fma(a, b, c) == PR.fma(a, b, c)
    X, ropes, _ = AR.cloud_scene(65, (2, 45), seed=2)
    for x in X[:20]:
        for y in ropes[1][:10]:
            assert AR.d2_fused(y, x) == PR.d2_fused(y, x)


@pytest.mark.parametrize("n,Ms", [(1, (1,)), (64, (2, 45)), (257, (1, 2, 45, 300)), (1025, (45, 45, 45)), (300, (300, 300, 45))])
def test_host_call_equals_the_statement(n, Ms):
    X, ropes, _ = AR.cloud_scene(n, Ms, seed=1)
    for d_max in (0.008, np.inf):
        owner, _ = host_equals_statement(X, ropes, d_max)
    assert sum(Ms) <= AR.TILE or len(Ms) == 3      # (the last case crosses the kernel's node tile)
    if n >= 64:
        assert len(set(owner.tolist()) - {-1}) == len(Ms)
    Xs, bad = AR.with_specials(X)
    owner, g = host_equals_statement(Xs, ropes, 0.008)
    assert (owner[bad] == -1).all() and np.isinf(g[bad]).all()


def test_refusals_of_the_host_call():
    X, ropes, _ = AR.cloud_scene(10, (2, 3))
    nan_rope = np.array(ropes[1]); nan_rope[1, 2] = np.nan
    for bad in (dict(d_max=0.0), dict(d_max=-1.0), dict(d_max=np.nan), dict(ropes=[ropes[0], nan_rope]), dict(ropes=[ropes[0], np.zeros((0, 3))])):
        with pytest.raises(B.TdloError):
            B.cloud_assign_host(X, bad.get("ropes", ropes), bad.get("d_max", 0.01))
    assert B.cloud_assign_host(np.zeros((0, 3)), ropes, 0.01)[2:] == ([0, 0], 0)      # a cloud of 0 points: every count 0


def test_ties_go_to_the_lowest_rope():
    X, ropes, d_max, i = AR.tie_scene()
    D = [AR.rope_min(X[i:i + 1], Y)[0] for Y in ropes]
    assert D[0] == D[2] < D[1] and D[0] == PR.d2_fused(ropes[0][7], X[i]) == PR.d2_fused(ropes[2][40], X[i])       # exactly tied, in different node tiles
    assert 7 < AR.TILE <= len(ropes[0]) + len(ropes[1]) + 40
    owner, _ = host_equals_statement(X, ropes, d_max)
    wrong = AR.assign(X, ropes, d_max, tie="highest")[0]
    assert owner[i] == 0 and wrong[i] == 2
    assert B.cloud_assign_host(X, ropes, d_max)[0][i] == 0


def test_the_gate_is_less_or_equal():
    X, ropes, d_max = AR.gate_scene()
    g = [min(PR.d2_fused(Y[0], x) for Y in ropes) for x in X]
    dmax2 = d_max * d_max
    assert g[0] == dmax2 and g[1] == np.nextafter(dmax2, np.inf) and g[2] < dmax2 < g[3]
    owner, rg = host_equals_statement(X, ropes, d_max)
    assert owner.tolist() == [0, -1, 1, -1] and rg.tolist() == g
    assert AR.assign(X, ropes, d_max, gate="<")[0].tolist() == [-1, -1, 1, -1]


def test_the_distance_is_the_fused_form():
    X, ropes = AR.fused_flip_scene()
    fused = [PR.d2_fused(Y[0], X[0]) for Y in ropes]
    plain = [AR.d2_plain(Y[0], X[0]) for Y in ropes]
    assert (fused[0] < fused[1]) != (plain[0] < plain[1]) and fused[0] != fused[1] and plain[0] != plain[1]
    owner, _ = host_equals_statement(X, ropes, np.inf)
    assert owner[0] == int(np.argmin(fused)) != AR.assign(X, ropes, np.inf, d2=AR.d2_plain)[0][0]


def test_the_destinations_keep_source_order():
    X, ropes, _ = AR.cloud_scene(257, (45, 45), seed=4)
    owner, g = host_equals_statement(X, ropes, 0.008)
    parts = AR.split(X, owner, 2)
    for f in range(2):
        idx = np.nonzero(owner == f)[0]
        assert np.array_equal(AR.bits(parts[f]), AR.bits(X[idx])) and (np.diff(idx) > 0).all()
        by_distance = X[idx[np.argsort(g[idx], kind="stable")]]
        assert not np.array_equal(by_distance, parts[f])               # sorting by distance gives another cloud
    Z, zr = AR.zero_scene()
    zo, _ = host_equals_statement(Z, zr, 0.05)
    assert zo.tolist() == [0, 0, 0, 0] and np.signbit(AR.split(Z, zo, 2)[0]).sum() == np.signbit(Z).sum() == 8


def test_lane_over_a_block_and_tile_grid_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/assign_lane_host_test.cpp with csrc/tdlo_assign_host.cpp: no HIP, built with -fsanitize=address,undefined (the runtime linked into the program)
    and run as a child process of its own.  Nothing sanitized is loaded into python."""
    exe = str(tmp_path / "assign_lane_host_test")
    csrc = os.path.join(ROOT, "trackdlo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "assign_lane_host_test.cpp"), os.path.join(csrc, "tdlo_assign_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"(\d+) points, 0 differing, (\d+) ties to the lower rope, (\d+) unowned\n", r.stdout)
    assert m and int(m.group(1)) == 23832 and int(m.group(2)) > 100 and int(m.group(3)) > 100, r.stdout
