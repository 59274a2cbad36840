"""CPU suite for image views (tdlo_image_view; csrc/tdlo_image_host.cpp): check and extent against the numpy statement (tests/image_view_ref.py), the
import kernel's form chooser over a grid of alignments, pitches and widths, the 32FC1 -> millimetre rule against exact integer arithmetic, the ctypes
layout against the header as a C++ compiler lays it out, and the host pack-and-convert through a stand-alone program built with
-fsanitize=address,undefined whose source buffers are allocated at exactly their extents.  No GPU, and no sanitizer on code loaded into python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import image_view_ref as R

SHAPES = [(1, 1), (1, 3), (3, 5), (2, 7), (5, 8), (4, 12), (33, 68)]
FORMAT_ROLE = [(R.U8C1, R.MASK), (R.U8C1, R.OCCLUDER), (R.U8C3, R.COLOUR), (R.U8C4, R.COLOUR), (R.U16C1, R.DEPTH), (R.F32C1, R.DEPTH)]


@pytest.fixture(scope="module")
def B():
    from trackdlo_amd import binding
    binding.load_library()
    return binding


def _view(B, addr, fmt, stride, loc=1):
    return B.ImageView(addr, fmt, loc, stride, None)


def test_check_and_extent_against_the_statement(B):
    A = 1 << 20                                                    # an address that is never dereferenced: check and extent are arithmetic
    cases = []
    for fmt, role in FORMAT_ROLE:
        bpp, es = R.BPP[fmt], R.ELEM[fmt]
        for rows, cols in SHAPES + [(480, 640)]:
            rb = cols * bpp
            for stride in (rb, rb + es, rb + 16, -rb, -(rb + 16), rb - es, -(rb - es), 0, 3, 1 << 40, -(1 << 40), (1 << 62) // max(rows - 1, 1) + 4096):
                cases.append((A, fmt, 1, stride, rows, cols, role))
        cases += [(A + 1, fmt, 1, 64 * bpp, 4, 8, role), (A + 2, fmt, 0, 64 * bpp, 4, 8, role), (A, fmt, 2, 64 * bpp + 2, 4, 8, role),
                  (A, fmt, 3, 64 * bpp, 4, 8, role), (A, fmt, -1, 64 * bpp, 4, 8, role), (A, fmt, 1, 64 * bpp, 4, 8, 4), (A, fmt, 1, 64 * bpp, 4, 8, -1),
                  (A, fmt, 1, 64 * bpp, 0, 8, role), (A, fmt, 1, 64 * bpp, 4, 0, role), (A, fmt, 1, 64 * bpp, -4, 8, role),
                  (A, fmt, 1, 8192 * bpp, 8192, 8192, role), (A, fmt, 1, 8193 * bpp, 8192, 8193, role), (A, fmt, 1, (1 << 26) * bpp, 1, 1 << 26, role),
                  (A, fmt, 1, 4, 1, (1 << 26) + 1, role), (0, fmt, 1, 64 * bpp, 4, 8, role)]
        for other in range(4):                                     # a format the role does not take
            cases.append((A, fmt, 1, 64 * bpp, 4, 8, other))
    cases += [(A, f, 1, 64, 2, 8, R.DEPTH) for f in (-1, 5, 99)]
    n_ok = n_bad = 0
    for addr, fmt, loc, stride, rows, cols, role in cases:
        want = R.check(addr, fmt, loc, stride, rows, cols, role)
        v = _view(B, addr, fmt, stride, loc)
        got = B.image_view_check(v, role, rows, cols)
        assert got == (0 if want else B.TDLO_E_INVALID), (addr, fmt, loc, stride, rows, cols, role)
        n_ok += want; n_bad += not want
        if want:
            assert B.image_view_extent(v, rows, cols) == R.extent(fmt, stride, rows, cols)
    assert n_ok > 200 and n_bad > 200
    # the legal odd cases, by name: one row with any stride (0, smaller than the row, negative), a negative stride, a pitch larger than the row
    for stride in (0, 1, -1, 5, -4096):
        assert B.image_view_check(_view(B, A, R.U8C3, stride), R.COLOUR, 1, 100) == 0
        assert B.image_view_extent(_view(B, A, R.U8C3, stride), 1, 100) == (0, 300)
    assert B.image_view_check(_view(B, A, R.U16C1, -200), R.DEPTH, 10, 100) == 0 and B.image_view_extent(_view(B, A, R.U16C1, -200), 10, 100) == (-1800, 200)
    assert B.image_view_check(_view(B, A, R.F32C1, 512), R.DEPTH, 10, 100) == 0 and B.image_view_extent(_view(B, A, R.F32C1, 512), 10, 100) == (0, 9 * 512 + 400)
    assert B.image_view_check(_view(B, A, R.U16C1, 198), R.DEPTH, 10, 100) == B.TDLO_E_INVALID          # rows overlap
    assert B.image_view_check(_view(B, A, R.U16C1, 201), R.DEPTH, 10, 100) == B.TDLO_E_INVALID          # pitch no multiple of the element
    with pytest.raises(B.TdloError):
        B.image_view_extent(_view(B, A, R.U16C1, 198), 10, 100)


def test_form_chooser_over_the_grid(B):
    """The chooser against the statement for alignment 0 .. 15, pitch offset 0 .. 16, cols 1 .. 9 (and 12, 16), both pitch signs; and the property the
    statement stands for: whenever a vector form is chosen, every load of it is naturally aligned and lies wholly inside one row of the view."""
    base = 1 << 20
    load_bytes = {(R.U8C1, 1): 4, (R.U8C3, 1): 4, (R.U8C4, 1): 4, (R.U16C1, 1): 4, (R.F32C1, 1): 4, (R.U8C4, 2): 16, (R.U16C1, 2): 8, (R.F32C1, 2): 16}
    seen = set()
    for fmt in (R.U8C1, R.U8C3, R.U8C4, R.U16C1, R.F32C1):
        bpp = R.BPP[fmt]
        for align in range(16):
            for extra in range(17):
                for cols in list(range(1, 10)) + [12, 16]:
                    for sign in (1, -1):
                        stride = sign * (cols * bpp + extra)
                        got = B.image_view_form(_view(B, base + align, fmt, stride), cols)
                        assert got == R.form(base + align, stride, cols, fmt), (fmt, align, extra, cols, sign)
                        seen.add((fmt, got))
                        if got:
                            assert cols % 4 == 0
                            w = load_bytes[(fmt, got)]
                            for row in range(3):
                                start = base + align + row * stride
                                for group in range(cols // 4):
                                    for a in range(start + 4 * group * bpp, start + 4 * (group + 1) * bpp, w):
                                        assert a % w == 0 and start <= a and a + w <= start + cols * bpp
    assert seen == {(R.U8C1, 0), (R.U8C1, 1), (R.U8C3, 0), (R.U8C3, 1), (R.U8C4, 0), (R.U8C4, 1), (R.U8C4, 2), (R.U16C1, 0), (R.U16C1, 1), (R.U16C1, 2),
                    (R.F32C1, 0), (R.F32C1, 1), (R.F32C1, 2)}


def _mm_exact(d):
    """floor(1000 d + 1/2) on [0, 65536), else 0, in exact integer arithmetic on the float's own bits: d = m 2^-s, so floor((2000 m + 2^s) / 2^(s + 1))."""
    bits = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign, ex, man = bits >> 31, (bits >> 23) & 0xff, bits & 0x7fffff
    m = np.where(ex > 0, man | (1 << 23), man)
    s = 150 - np.maximum(ex, 1)                                    # d = m 2^-s; s <= 0: d >= 2^23, too large; s > 40: 2000 m < 2^35 <= 2^(s - 6), so 0
    small = (s >= 1) & (s <= 40)
    sc = np.where(small, s, 1)
    q = np.where(small, (2000 * m + (np.int64(1) << sc)) >> (sc + 1), 0)
    q = np.where((q < 65536) & (sign == 0) & (ex != 0xff), q, 0)    # (a negative d gives 1000 d + 1/2 < 1/2: floor 0 or out of range, 0 either way)
    return q.astype(np.uint16)


def _mm_library(B, d):
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1)
    out = np.zeros(d.size, dtype=np.uint16)
    for a in range(0, d.size, 1 << 26):
        part = d[a:a + (1 << 26)]
        v = B.image_view(part.reshape(1, -1))
        assert B.load_library().tdlo_image_view_pack(C.byref(v), 1, part.size, R.DEPTH, out[a:].ctypes.data_as(C.c_void_p)) == 0
    return out


def test_float_rule(B):
    set_a = (np.arange(1 << 20, dtype=np.uint32) << 12).view(np.float32)                 # every float32 whose low 12 mantissa bits are zero
    centre = ((np.arange(65537) + 0.5) / 1000.0).astype(np.float32).view(np.uint32).astype(np.int64)
    set_b = (centre[:, None] + np.arange(-4, 5)[None, :]).reshape(-1).astype(np.uint32).view(np.float32)      # +-4 ulps around every (k + 0.5) / 1000
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 65.535, 65.5354, 65.5355, 65.536, 1e-45, -1e-45, 0.0005, 0.00049999, -0.0004, -1.0, 1e30],
                       dtype=np.float32)
    for name, d in (("A", set_a), ("B", set_b), ("special", special)):
        want = _mm_exact(d)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(R.f32_to_mm(d), want, err_msg=name)             # the statement's float64 evaluation is the exact rule
        np.testing.assert_array_equal(_mm_library(B, d), want, err_msg=name)              # and so is the library's
    assert [int(x) for x in R.f32_to_mm(special[:7])] == [0, 0, 0, 0, 0, 65535, 65535] and int(R.f32_to_mm(np.float32(65.536))) == 0
    assert [R.f32_to_mm_exact(x) for x in special] == [int(x) for x in R.f32_to_mm(special)]
    rng = np.random.default_rng(3)
    for x in set_b[rng.integers(0, set_b.size, 3000)]:                                    # exact rationals agree with the integer form
        assert R.f32_to_mm_exact(x) == int(_mm_exact(np.array([x]))[0])
    # properties: the maximum is 65535, and k / 1000 as float32 comes back as k
    assert int(R.f32_to_mm(set_b).max()) == 65535 and int(_mm_library(B, set_b).max()) == 65535
    with np.errstate(invalid="ignore"):
        assert not R.f32_to_mm(set_a[~(set_a.astype(np.float64) < 65.5355)]).any() and not R.f32_to_mm(set_b[~(set_b.astype(np.float64) < 65.5355)]).any()      # (beyond the range, NaN included: 0)
    k = np.arange(65536)
    np.testing.assert_array_equal(R.f32_to_mm((k / 1000.0).astype(np.float32)), k.astype(np.uint16))
    np.testing.assert_array_equal(_mm_library(B, (k / 1000.0).astype(np.float32)), k.astype(np.uint16))


def test_ctypes_layout_matches_the_header(B, tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "trackdlo_hip.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(tdlo_image_view), offsetof(tdlo_image_view, data), '
                   'offsetof(tdlo_image_view, format), offsetof(tdlo_image_view, location), offsetof(tdlo_image_view, row_stride), '
                   'offsetof(tdlo_image_view, ready_stream), sizeof(tdlo_frame_view), offsetof(tdlo_frame_view, depth), offsetof(tdlo_frame_view, colour), '
                   'offsetof(tdlo_frame_view, occluder), offsetof(tdlo_frame_view, mask)); return 0; }\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    V, F = B.ImageView, B.FrameView
    assert got == [C.sizeof(V), V.data.offset, V.format.offset, V.location.offset, V.row_stride.offset, V.ready_stream.offset,
                   C.sizeof(F), F.depth.offset, F.colour.offset, F.occluder.offset, F.mask.offset]
    assert (B.IMG_U8C1, B.IMG_U8C3, B.IMG_U8C4, B.IMG_U16C1, B.IMG_F32C1) == (R.U8C1, R.U8C3, R.U8C4, R.U16C1, R.F32C1)


def test_image_view_of_numpy_arrays(B):
    a = np.zeros((6, 8, 4), dtype=np.uint8)
    v = B.image_view(a[::-1, :6])
    assert (v.format, v.location, v.row_stride, v.rows, v.cols, v.data) == (R.U8C4, B.MEM_HOST, -32, 6, 6, a.ctypes.data + 5 * 32)
    d = np.zeros((6, 10), dtype=np.int16)
    v = B.image_view(d[:, 1:9], format=B.IMG_U16C1)
    assert (v.format, v.row_stride, v.cols, v.data) == (R.U16C1, 20, 8, d.ctypes.data + 2)
    assert B.image_view(np.zeros((4, 4), dtype=np.float32)).format == R.F32C1 and B.image_view(np.zeros((4, 4, 3), dtype=np.uint8)).format == R.U8C3
    for bad in (np.zeros((4, 4), dtype=np.int16), np.zeros((4, 4, 2), dtype=np.uint8), np.zeros(4, dtype=np.uint8), np.zeros((4, 8), dtype=np.uint8)[:, ::2]):
        with pytest.raises(TypeError):
            B.image_view(bad)
    with pytest.raises(ValueError):
        B.frame_view(np.zeros((4, 4), dtype=np.uint16), mask=np.zeros((4, 5), dtype=np.uint8))


def _cases(rng):
    out = []
    for fmt, role in FORMAT_ROLE:
        if role == R.OCCLUDER:
            continue
        for rows, cols in SHAPES:
            for name, buf, off, stride in R.layouts(rows, cols, fmt, rng):
                out.append((f"{fmt}-{rows}x{cols}-{name}", fmt, role, rows, cols, buf, off, stride))
    return out


def _run_cases(tmp_path, program, sources, said):
    """Builds tests/cpp/<program>.cpp with the sanitizers, runs it on the layouts of both suites as a child process with nothing preloaded, and compares
    the canonical bytes it writes with the statement's."""
    exe = str(tmp_path / program)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "cpp", program + ".cpp")] + [os.path.join(ROOT, "trackdlo_amd", "csrc", f) for f in sources] + ["-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = _cases(np.random.default_rng(11))
    blob = [np.array([len(cases)], dtype=np.int64).tobytes()]
    want = []
    for name, fmt, role, rows, cols, buf, off, stride in cases:
        lo, hi = R.extent(fmt, stride, rows, cols)
        lead = off + lo                                             # the poisoned bytes in front of the extent
        assert lead in (0, 1, 2, 4, 8) and buf.size == off + hi
        blob.append(np.array([fmt, role, rows, cols, stride, lead, lo, hi], dtype=np.int64).tobytes())
        blob.append(buf[lead:].tobytes())
        want.append(R.canonical(buf, off, fmt, stride, rows, cols).tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases {said}" in r.stdout, r.stdout
    got = (tmp_path / "out.bin").read_bytes()
    assert len(got) == sum(len(w) for w in want)
    at = 0
    for (name, *_), w in zip(cases, want):
        assert got[at:at + len(w)] == w, name
        at += len(w)
    return r.stdout


def test_host_pack_in_a_sanitized_stand_alone_program(tmp_path):
    """csrc/tdlo_image_host.cpp built into tests/cpp/image_pack_test.cpp with -fsanitize=address,undefined and run as a child process of its own (nothing
    preloaded): every source buffer is a heap block that ends -- and, where the sanitizer's 8-byte granule allows, starts -- at the view's extent, so a
    host access outside the extent is a report; the canonical bytes it writes are the statement's."""
    _run_cases(tmp_path, "image_pack_test", ["tdlo_image_host.cpp"], "packed")


def test_the_kernels_lane_compiled_for_the_host(tmp_path):
    """csrc/tdlo_image_lane.h -- the code a lane of k_image_import runs -- compiled for the host (tests/cpp/image_lane_host_test.cpp) and run lane by lane
    under the same sanitizers on the same layouts: a load outside a view's extent, a misaligned vector load or a store outside the canonical image is a
    report, and the bytes are the statement's, in all three load forms.  The CPU-side check of the kernel's logic; the GPU build is checked by
    tests/test_image_view_gpu.py."""
    said = _run_cases(tmp_path, "image_lane_host_test", ["tdlo_image_host.cpp"], "imported")
    counts = [int(x) for x in said.split(":")[-1].split()]
    assert len(counts) == 3 and min(counts) > 20, said
