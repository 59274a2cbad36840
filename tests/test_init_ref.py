"""CPU suite of the chain order (`sort_pts`, utils.cpp:95-170): the numpy statement (tests/init_ref.py) against what the reference's prototype
returned (tests/golden/proto_sort_pts.npz), the scenes' stated properties on the statement's trace, the host twin (tdlo_sort_pts_host) against the
statement on every scene -- permutation, nodes and coordinate bits, and the verdicts on what it refuses --, three wrong variants of the rule that the
scenes must tell from it, and the twin in a stand-alone program under -fsanitize=address,undefined.  No GPU, and no sanitizer on code loaded into
python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import init_ref as R


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    binding.load_library()
    return binding


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_statement_equals_the_prototype_row_for_row():
    z = np.load(os.path.join(GOLDEN, "proto_sort_pts.npz"))
    names = [str(n) for n in z["names"]]
    sizes = [len(z[f"in_{n}"]) for n in names]
    assert len(names) >= 35 and min(sizes) == 2 and max(sizes) == 64
    for n in names:
        Y = z[f"in_{n}"]
        r = R.statement(Y)
        assert r["status"] == 0, n
        assert np.array_equal(_bits(r["Y"]), _bits(z[f"out_{n}"])), n
        assert np.array_equal(_bits(r["coord"]), _bits(z[f"coord_{n}"])), n
        lit = R.statement_literal(Y)
        assert np.array_equal(lit["perm"], r["perm"]) and lit["rounds"] == r["rounds"] and lit["reverse"] == r["reverse"], n


def test_the_two_forms_of_the_statement_agree():
    for n in R.small_scene_names():
        Y = R.scenes()[n]
        for variant in (None, "largest_parent", "counter_off", "zero_edge"):
            a = R.statement_literal(Y, variant); b = R.statement(Y, variant) if variant else R.ref(n)
            assert a["status"] == b["status"] and a["rounds"] == b["rounds"] and a["reverse"] == b["reverse"], (n, variant)
            assert a["status"] or np.array_equal(a["perm"], b["perm"]), (n, variant)
    for n, (Y, st) in R.error_inputs().items():
        assert R.statement(Y)["status"] == st and R.statement_literal(Y)["status"] == st, n


def test_every_scene_has_its_property():
    sc = R.scenes()
    assert sorted(len(sc[f"rope{M}"]) for M in R.SIZES) == R.SIZES
    for n in sc:
        r = R.ref(n)
        assert r["status"] == 0 and sorted(r["perm"].tolist()) == list(range(len(sc[n]))), n
        assert r["rounds"][0][0] == 0 and r["perm"].tolist().index(0) >= 0
        c = r["coord"]
        assert c[0] == 0.0 and (np.diff(c) > 0).all(), n
    assert set(R.ref("end_first")["reverse"]) == {0}                                 # node 0 at an end: the list is only appended to
    rv = R.ref("middle_first")["reverse"]
    assert 1 in rv and 2 in rv and rv.index(1) < rv.index(2)                         # node 0 in the middle: one turn, then back
    assert max(R.ref("u_shape")["reverse"]) >= 3
    t = R.ref("lattice")["ties"]
    assert len(sc["lattice"]) == 64 and sum(1 for x in t if x > 1) > len(t) // 2     # equal distances in most rounds: the tie rule decides
    Y = sc["one_ulp"]
    d = np.abs(Y[:, None, :] - Y[None, :, :]).sum(axis=2) + np.eye(len(Y))
    i, j = np.unravel_index(np.argmin(d), d.shape)
    assert np.array_equal(Y[i, 1:], Y[j, 1:]) and abs(int(_bits(Y[i, :1])[0]) - int(_bits(Y[j, :1])[0])) == 1
    p = R.ref("one_ulp")["perm"].tolist()
    assert abs(p.index(i) - p.index(j)) == 1                                         # (the two are neighbours in the chain)
    Y = sc["signed_zero"]
    assert (Y[:, 0] == 0.0).all() and 0 < np.signbit(Y[:, 0]).sum() < len(Y) and R.precheck(Y) == 0
    G = R.dist2_matrix(sc["underflow"])
    assert G[0, 1] == 0.0 and (0, 1) not in R.ref("underflow")["rounds"] and not np.array_equal(sc["underflow"][0], sc["underflow"][1])
    # a shuffled rope comes back in the rope's own order, or its reverse
    for fn in (R.rope_end_first, R.rope_middle_first):
        Y, order = fn()
        d = np.diff(order[R.statement(Y)["perm"]])
        assert (d == 1).all() or (d == -1).all()


def test_host_twin_equals_the_statement(B):
    for n, Y in R.scenes().items():
        r = R.ref(n)
        Ys, perm, coord = B.sort_pts_host(Y)
        assert np.array_equal(perm, r["perm"]), n
        assert np.array_equal(_bits(Ys), _bits(r["Y"])) and np.array_equal(_bits(coord), _bits(r["coord"])), n
    lib = B.load_library()
    for n, (Y, st) in R.error_inputs().items():
        Yf = np.asfortranarray(Y)
        Ys = np.full(Yf.shape, 7.0, order="F"); perm = np.full(len(Y), -7, dtype=np.int32); coord = np.full(len(Y), 7.0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.tdlo_sort_pts_host(p(Yf), len(Y), p(Ys), p(perm), p(coord)) == B.TDLO_E_NUMERIC, n
        assert (Ys == 7.0).all() and (perm == -7).all() and (coord == 7.0).all(), n
    one = np.zeros((1, 3), order="F")
    for M in (1, 0, -3, 1025):
        assert lib.tdlo_sort_pts_host(one.ctypes.data_as(C.c_void_p), M, None, None, None) == B.TDLO_E_INVALID
    assert lib.tdlo_sort_pts_host(None, 5, None, None, None) == B.TDLO_E_INVALID
    Y = np.asfortranarray(R.scenes()["end_first"])
    assert lib.tdlo_sort_pts_host(Y.ctypes.data_as(C.c_void_p), len(Y), None, None, None) == 0      # every output is optional


@pytest.mark.parametrize("variant", ["largest_parent", "counter_off", "zero_edge"])
def test_a_wrong_rule_is_told_from_the_statement(variant):
    differs = []
    for n in R.small_scene_names():
        q = R.statement(R.scenes()[n], variant); r = R.ref(n)
        if q["status"] != r["status"] or not np.array_equal(q["perm"], r["perm"]):
            differs.append(n)
    assert differs, variant


def test_host_twin_in_a_sanitized_stand_alone_program(tmp_path):
    """csrc/tdlo_host.cpp built into tests/cpp/sort_pts_host_test.cpp with -fsanitize=address,undefined and run as a child process of its own (nothing
    preloaded) on every scene and every refused input: inputs and outputs are heap blocks of exactly their sizes."""
    exe = str(tmp_path / "sort_pts_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "trackdlo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sort_pts_host_test.cpp"),
                        os.path.join(ROOT, "trackdlo_amd", "csrc", "tdlo_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [(n, Y, 0) for n, Y in R.scenes().items()] + [(n, Y, st) for n, (Y, st) in R.error_inputs().items()]
    blob = [np.array([len(cases)], dtype=np.int64).tobytes()]
    for _, Y, _ in cases:
        blob.append(np.array([len(Y)], dtype=np.int64).tobytes()); blob.append(np.asfortranarray(Y).tobytes(order="F"))
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases sorted" in r.stdout, r.stdout
    got = (tmp_path / "out.bin").read_bytes()
    at = 0
    for n, Y, st in cases:
        M = len(Y)
        assert int(np.frombuffer(got, dtype=np.int64, count=1, offset=at)[0]) == st, n
        at += 8
        if st == 0:
            ref = R.ref(n)
            Ys = np.frombuffer(got, dtype=np.float64, count=3 * M, offset=at).reshape(3, M).T; at += 24 * M
            perm = np.frombuffer(got, dtype=np.int32, count=M, offset=at); at += 4 * M
            coord = np.frombuffer(got, dtype=np.float64, count=M, offset=at); at += 8 * M
            assert np.array_equal(perm, ref["perm"]) and np.array_equal(_bits(Ys), _bits(ref["Y"])) and np.array_equal(_bits(coord), _bits(ref["coord"])), n
    assert at == len(got)
