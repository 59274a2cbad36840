"""One cloud clustered into F ropes without a GPU: the host call tdlo_cloud_cluster_host equals the statement (tests/cluster_ref.py) in owners and counts on
every scene; six wrong readings of the statement are each told from it on a scene built for that; the lane runs over a whole (workgroup, tile) grid in several
visiting orders in a sanitized stand-alone program.  Everything is exact: integers equal, clouds equal as bit patterns."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from trackdlo_amd import binding as B
import assign_ref as AR
import cluster_ref as CR

NEW = ["tdlo_cloud_cluster", "tdlo_cloud_cluster_host", "tdlo_tracker_initialize_from_shared_cloud_batch"]


def test_the_new_names_are_declared_required_and_exported():
    text = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tdlo_[a-z0-9_]+)\s*\(", hdr))
    lib = B.load_library()
    for name in NEW:
        assert name in declared and name in B.SYMBOLS and hasattr(lib, name), name
    assert lib.tdlo_abi_version() == 3
    assert lib.tdlo_debug_route_count(None, 55) == -1 and lib.tdlo_debug_route_count(None, 56) == -1
    assert re.search(r"\* 55 / 56: calls of tdlo_cloud_cluster", text)
    assert "starting F same-coloured ropes from one cloud (reg + sort_pts" not in text      # no longer out of scope
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "tdlo_tracker_initialize_from_shared_cloud_batch" in open(os.path.join(ROOT, doc)).read(), doc


@pytest.mark.parametrize("name", list(CR.SCENES))
def test_host_call_equals_the_statement(name):
    s, (owner, C, n_each, un, _) = CR.scene(name)
    own, hc, hn, hu = B.cloud_cluster_host(s["X"], s["F"], s["tol"], s["min_size"])
    assert np.array_equal(own, owner) and (hc, hn, hu) == (C, n_each, un), name
    assert sum(n_each) + un == len(s["X"])


def test_refusals_of_the_host_call():
    X = CR.ropes(10, 2)
    for bad in (dict(tol=0.0), dict(tol=-1.0), dict(tol=np.nan), dict(tol=np.inf), dict(min_size=0), dict(min_size=-3), dict(F=0)):
        with pytest.raises(B.TdloError):
            B.cloud_cluster_host(X, bad.get("F", 2), bad.get("tol", CR.TOL), bad.get("min_size", 1))
    assert B.cloud_cluster_host(np.zeros((0, 3)), 2, CR.TOL, 1)[1:] == (0, [0, 0], 0)      # a cloud of 0 points: every count 0
    lib = B.load_library()
    big = np.zeros(3)
    assert lib.tdlo_cloud_cluster_host(B._ptr(big), 262145, 1, 0.01, 1, None, None, None, None) == B.TDLO_E_INVALID      # refused before X is read


def differs(name, **reading):
    s, ref = CR.scene(name)
    wrong = CR.cluster(**s, **reading)
    return not (np.array_equal(wrong[0], ref[0]) and wrong[1:4] == ref[1:4])


def test_each_wrong_reading_is_told_from_the_statement():
    assert differs("gate", gate="<")
    assert differs("fused", d2=AR.d2_plain)
    assert differs("numbering", numbering="size") and differs("noise", numbering="size")
    assert differs("numbering", numbering="largest")
    assert differs("noise", keep=">")
    assert differs("chain_identity", linkage="first") and differs("chain_stride", linkage="first")
    for name in ("gate", "fused", "numbering", "noise", "chain_identity", "chain_stride"):      # ... and the host call sides with the statement on each
        s, (owner, C, n_each, un, _) = CR.scene(name)
        own, hc, hn, hu = B.cloud_cluster_host(s["X"], s["F"], s["tol"], s["min_size"])
        assert np.array_equal(own, owner) and (hc, hn, hu) == (C, n_each, un)


def test_the_link_is_symmetric_and_the_reference_decides_near_the_gate_in_the_fused_form():
    s, _ = CR.scene("gate")
    X, tol = s["X"], s["tol"]
    for i in range(3):
        for j in range(3):
            assert AR.d2_fused(X[i], X[j]) == AR.d2_fused(X[j], X[i])
    A = CR.links(X, tol)
    assert A[0, 1] and A[1, 0] and not A[1, 2] and not A[2, 1] and not A[0, 2]
    s, _ = CR.scene("fused")
    assert CR.links(s["X"], s["tol"])[0, 1] == (AR.d2_fused(s["X"][1], s["X"][0]) <= s["tol"] * s["tol"])


def test_the_destinations_keep_source_order_and_bits():
    s, (owner, C, n_each, un, _) = CR.scene("zeros")
    parts = CR.split(s["X"], owner, s["F"])
    assert np.array_equal(CR.bits(parts[0]), CR.bits(s["X"][:3])) and np.signbit(parts[0]).sum() == 5
    s, (owner, *_rest) = CR.scene("ropes3_n257")
    for f, part in enumerate(CR.split(s["X"], owner, 3)):
        idx = np.nonzero(owner == f)[0]
        assert (np.diff(idx) > 0).all() and np.array_equal(CR.bits(part), CR.bits(s["X"][idx]))


def test_lane_over_a_workgroup_and_tile_grid_in_a_sanitized_stand_alone_program(tmp_path):
    """tests/cpp/cluster_lane_host_test.cpp with csrc/tdlo_cluster_host.cpp: no HIP, built with -fsanitize=address,undefined (the runtime linked into the
    program) and run as a child process of its own.  Nothing sanitized is loaded into python."""
    exe = str(tmp_path / "cluster_lane_host_test")
    csrc = os.path.join(ROOT, "trackdlo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "cluster_lane_host_test.cpp"), os.path.join(csrc, "tdlo_cluster_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"(\d+) runs, 0 differing, (\d+) clusters, (\d+) lanes skipped\n", r.stdout)
    assert m and int(m.group(1)) == 180 and int(m.group(2)) >= 18 and int(m.group(3)) > 100, r.stdout
