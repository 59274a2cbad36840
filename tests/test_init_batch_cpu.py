"""What a batched start (tdlo_reg_batch, tdlo_sort_pts_batch, tdlo_tracker_initialize_from_cloud_batch) can be held to without a GPU: the new names in
the header, the library and the binding; a null context; the per-frame plan of the workspace (csrc/tdlo_reg_plan.h through tdlo_debug_reg_batch_plan,
and in a stand-alone program under -fsanitize=address,undefined -- nothing sanitized is loaded into python); the binding's marshalling against a
stand-in library, as tests/test_tracker_batch_cpu.py does it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from trackdlo_amd import binding as B
from test_tracker_batch_cpu import addr, arr, stub_context, stub_tracker, patched_handles

NEW = ["tdlo_reg_batch", "tdlo_sort_pts_batch", "tdlo_tracker_initialize_from_cloud_batch", "tdlo_debug_reg_batch_plan"]
CLOUD_SIZES = [255, 256, 257, 1, 3000, 70001]          # the border sizes of tests/test_init_batch_gpu.py, case 1
NODE_COUNTS = [4, 5, 64, 65, 356, 890]                 # ... and the node counts of its case 2


@pytest.fixture(scope="module")
def lib():
    return B.load_library()


def test_the_new_names_are_declared_exported_and_required(lib):
    hdr = open(os.path.join(ROOT, "include", "trackdlo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in B.SYMBOLS and hasattr(lib, name), name
    assert lib.tdlo_abi_version() == 3


def test_a_null_context_is_refused(lib):
    one = np.zeros(12); sl = np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tdlo_reg_batch(None, p(sl), 1, p(one), p(one), 4, 0.05, 1) == B.TDLO_E_INVALID
    assert lib.tdlo_sort_pts_batch(None, p(one), 1, 4, None, None, None, None) == B.TDLO_E_INVALID
    assert lib.tdlo_tracker_initialize_from_cloud_batch(None, 1, 0.05, 1, None, None) == B.TDLO_E_INVALID
    null_tab = (C.c_void_p * 1)(None)
    assert lib.tdlo_tracker_initialize_from_cloud_batch(C.cast(null_tab, C.c_void_p), 1, 0.05, 1, None, None) == B.TDLO_E_INVALID
    assert lib.tdlo_debug_route_count(None, 36) == -1 and lib.tdlo_debug_route_count(None, 37) == -1


def _plan(lib, N, M):
    F = len(N)
    Na = np.array(N, dtype=np.int32); nblk = np.zeros(F, dtype=np.int32)
    so = np.zeros(F, dtype=np.int64); po = np.zeros(F, dtype=np.int64); oo = np.zeros(F, dtype=np.int64); total = C.c_longlong(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tdlo_debug_reg_batch_plan(p(Na), F, M, p(nblk), p(so), p(po), p(oo), C.byref(total)) == 0
    return nblk.tolist(), so.tolist(), po.tolist(), oo.tolist(), total.value


def _single_nblk(N):
    return max(1, min(-(-N // 256), 256))              # reg_enqueue's rule (tests/reg_ref.py: geometry)


def _reg_ws_doubles(M, nblk):
    return 8 + 3 * M + nblk * (5 * M + 1) + 8          # csrc/tdlo_reg.hip


def _sort_pts_out_doubles(M):
    return 2 + 4 * M + (M + 1) // 2                    # csrc/tdlo_init.hip


def _check_plan(N, M, nblk, so, po, oo, total):
    assert nblk == [_single_nblk(n) for n in N]
    blocks = []
    for f in range(len(N)):
        blocks += [(so[f], 8 + 3 * M), (po[f], nblk[f] * (5 * M + 1)), (oo[f], _sort_pts_out_doubles(M))]
        assert oo[f] % 2 == 0 and so[f] % 2 == 0, (f, oo[f], so[f])          # 16 bytes
    blocks.sort()
    assert blocks[0][0] >= 0 and blocks[-1][0] + blocks[-1][1] <= total
    for (a, n), (b, _) in zip(blocks, blocks[1:]):
        assert a + n <= b, (a, n, b)


@pytest.mark.parametrize("M", NODE_COUNTS + [8])
def test_plan_blocks_are_disjoint_aligned_and_inside_the_total(lib, M):
    for N in (CLOUD_SIZES, CLOUD_SIZES[::-1], [300, 301, 302], [1], [70001] * 32):
        _check_plan(N, M, *_plan(lib, N, M))


@pytest.mark.parametrize("M", NODE_COUNTS + [8])
def test_plan_of_one_frame_is_the_single_calls(lib, M):
    for N in CLOUD_SIZES:
        nblk, so, po, oo, total = _plan(lib, [N], M)
        assert total == _reg_ws_doubles(M, nblk[0]) + _sort_pts_out_doubles(M)
        assert so == [0] and po == [8 + 3 * M + ((3 * M) & 1)]               # state and partials where launch_reg has them


def test_plan_refusals_and_optional_outputs(lib):
    Na = np.array([5, 6], dtype=np.int32); total = C.c_longlong(-1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tdlo_debug_reg_batch_plan(p(Na), 2, 8, None, None, None, None, C.byref(total)) == 0 and total.value == _plan(lib, [5, 6], 8)[4]
    assert lib.tdlo_debug_reg_batch_plan(p(Na), 2, 8, None, None, None, None, None) == 0
    for args in ((None, 2, 8), (p(Na), 0, 8), (p(Na), -1, 8), (p(Na), 2, 0)):
        assert lib.tdlo_debug_reg_batch_plan(*args, None, None, None, None, C.byref(total)) == B.TDLO_E_INVALID
    assert lib.tdlo_debug_reg_batch_plan(p(np.array([5, 0], dtype=np.int32)), 2, 8, None, None, None, None, C.byref(total)) == B.TDLO_E_INVALID


def test_plan_in_a_sanitized_stand_alone_program(lib, tmp_path):
    """tests/cpp/reg_plan_host_test.cpp: the plan header alone (no HIP), built with -fsanitize=address,undefined, run as a child process of its own
    (nothing preloaded): it fills every block of every frame in a heap workspace of exactly `total` doubles."""
    exe = str(tmp_path / "reg_plan_host_test")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "trackdlo_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "reg_plan_host_test.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    for M in NODE_COUNTS:
        for N in (CLOUD_SIZES, [1], [300, 301, 302]):
            r = subprocess.run([exe, str(M)] + [str(n) for n in N], capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0, (M, N, r.stdout + r.stderr)
            lines = r.stdout.split("\n")
            nblk, so, po, oo, total = _plan(lib, N, M)
            assert lines[0] == f"F={len(N)} M={M} total={total}"
            assert [[int(x) for x in ln.split()] for ln in lines[1:1 + len(N)]] == [list(t) for t in zip(nblk, so, po, oo)]
    r = subprocess.run([exe, "8", "5", "0"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 3 and "refused" in r.stdout


# ---- the binding's marshalling ---------------------------------------------------------------------------------------------------------------
class StubLib:
    """Records what the binding hands to the three entry points and fills the outputs like the library would."""
    def __init__(self):
        self.calls = []
        self.rc = 0

    def tdlo_last_error(self, h):
        return b"stub"

    def tdlo_debug_route_count(self, h, which):
        return 100 + which

    def tdlo_reg_batch(self, h, slots, F, Y, sigma2, M, mu, max_iter):
        self.calls.append(dict(h=h, F=F, slots=arr(slots, F, C.c_int), M=M, mu=mu, max_iter=max_iter))
        out = (C.c_double * (3 * M * F)).from_address(addr(Y))
        for i in range(3 * M * F):
            out[i] = float(i)
        for f in range(F):
            (C.c_double * F).from_address(addr(sigma2))[f] = 0.5 + f
        return self.rc

    def tdlo_sort_pts_batch(self, h, Y, F, M, Ys, perm, coord, rcs):
        self.calls.append(dict(h=h, F=F, M=M, Y=arr(Y, 3 * M * F, C.c_double)))
        o = (C.c_double * (3 * M * F)).from_address(addr(Ys))
        for i in range(3 * M * F):
            o[i] = 1000.0 + i
        (C.c_int * (M * F)).from_address(addr(perm))[M] = 7
        (C.c_double * (M * F)).from_address(addr(coord))[M + 1] = 0.25
        (C.c_int * F).from_address(addr(rcs))[F - 1] = self.rc
        return self.rc

    def tdlo_tracker_initialize_from_cloud_batch(self, tab, F, mu, max_iter, s2, rcs):
        self.calls.append(dict(trackers=arr(tab, F, C.c_void_p), F=F, mu=mu, max_iter=max_iter))
        for f in range(F - 1):
            (C.c_double * F).from_address(addr(s2))[f] = 2.0 + f
        (C.c_int * F).from_address(addr(rcs))[F - 1] = self.rc
        return self.rc


def test_reg_batch_marshalling():
    lib = StubLib(); ctx = stub_context(lib)
    Y, s2 = ctx.reg_batch([5, 0, 3], 4, 0.1, 7)
    c = lib.calls[0]
    assert (c["h"], c["F"], c["slots"], c["M"], c["mu"], c["max_iter"]) == (0x1234, 3, [5, 0, 3], 4, 0.1, 7)
    assert Y.shape == (3, 4, 3) and s2.tolist() == [0.5, 1.5, 2.5]
    for f in range(3):                   # F consecutive column-major M x 3 blocks
        assert Y[f].T.reshape(-1).tolist() == [float(12 * f + i) for i in range(12)]
    assert ctx.init_batch_route_counts() == [136, 137]
    lib.rc = B.TDLO_E_INVALID
    with pytest.raises(B.TdloError):
        ctx.reg_batch([0, 0], 4)


def test_sort_pts_batch_marshalling():
    lib = StubLib(); ctx = stub_context(lib)
    F, M = 3, 5
    Ys = np.arange(F * M * 3, dtype=np.float64).reshape(F, M, 3)
    Yo, perm, coord, codes = ctx.sort_pts_batch(Ys)
    c = lib.calls[0]
    assert (c["h"], c["F"], c["M"]) == (0x1234, 3, 5)
    for f in range(F):
        assert c["Y"][15 * f: 15 * (f + 1)] == Ys[f].T.reshape(-1).tolist()
        assert Yo[f].T.reshape(-1).tolist() == [1000.0 + 15 * f + i for i in range(15)]
    assert perm.shape == (F, M) and perm[1, 0] == 7 and coord[1, 1] == 0.25 and codes == [0, 0, 0]
    lib.rc = B.TDLO_E_NUMERIC
    assert ctx.sort_pts_batch(Ys, check=False)[3] == [0, 0, B.TDLO_E_NUMERIC]
    with pytest.raises(B.TdloError):
        ctx.sort_pts_batch(Ys)


def test_initialize_from_cloud_batch_marshalling():
    lib = StubLib(); ctx = stub_context(lib)
    trk = [stub_tracker(ctx, 0x3000 + i) for i in range(3)]
    patched_handles(trk)
    codes, s2 = B.initialize_from_cloud_batch(trk, 0.07, 11)
    c = lib.calls[-1]
    assert c["trackers"] == [0x3000, 0x3001, 0x3002] and (c["F"], c["mu"], c["max_iter"]) == (3, 0.07, 11)
    assert codes == [0, 0, 0] and s2[:2].tolist() == [2.0, 3.0] and np.isnan(s2[2])      # (a frame the library does not write stays NaN)
    lib.rc = B.TDLO_E_NUMERIC
    assert B.initialize_from_cloud_batch(trk, check=False)[0] == [0, 0, B.TDLO_E_NUMERIC]
    assert (lib.calls[-1]["mu"], lib.calls[-1]["max_iter"]) == (0.05, 100)
    with pytest.raises(B.TdloError):
        B.initialize_from_cloud_batch(trk)
    for t in trk:
        t.h = None           # (nothing for __del__ to destroy)
