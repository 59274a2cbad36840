"""The prologue of k_iter_fused's M-step half is ONE memory round trip -- checked on the compiler's output, on the CPU.

tdlo_iter_fused.hip is compiled device-only to gfx950 assembly with the Makefile's flags.  The M-step half (tdlo_mstep_chain_body.h, FUSE == 1) emits the
comment line TDLO_FUSED_PROLOGUE_REQUESTED through inline asm behind its last request; on the path of chains of up to 63 nodes (nS <= 256):

  * no `s_waitcnt vmcnt(..)` stands between the kernel's first vector load and that line (before: three -- the state copy's, the one in front of
    acc_shift()'s v_readfirstlane, the one in front of the slot's requests);
  * at most one `s_waitcnt lgkmcnt(0)` that waits for kernel-argument loads stands in front of it (before: six batches);
  * no vector load follows it in front of the first s_barrier;
  * the kernel uses no scratch memory.

The text between the kernel's entry and the marker is straight-line but for forward branches over blocks that lie inside it (the points' `n < N0`, the
second element of a chain of 64 nodes, the priors): the test checks that every branch target lies inside, so that reading the text line by line covers
every path.  Without the marker (the kernel before this prologue) the region ends at the last vector load in front of the first s_barrier, and the same
counts are taken there.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trackdlo_amd", "csrc")
MARKER = "TDLO_FUSED_PROLOGUE_REQUESTED"
VLOAD = re.compile(r"^(global_load|flat_load|buffer_load|scratch_load)")


def _hipcc():
    for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if p and os.path.exists(p):
            return p
    return None


def _makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^GPU_ARCH\s*:=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(EXTRA)", "").split()
    rule = re.search(r"^build/tdlo_iter_fused\.o:.*\n\t.*\n\t(.*)$", mk, re.M).group(1)      # the object's own recipe: no further flags today
    assert "$(FLAGS)" in rule and "-mllvm" not in rule, rule
    return ["--offload-arch=" + arch] + flags


@pytest.fixture(scope="module")
def kernel_text(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "tdlo_iter_fused.s")
    subprocess.check_call([hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", "tdlo_iter_fused.hip", "-o", out], cwd=CSRC,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel(text):
    m = re.search(r"^(_ZN4tdlo12k_iter_fusedIfEE\w+):", text, re.M)
    assert m, "k_iter_fused<float> not in the assembly"
    end = text.index(".Lfunc_end", m.end())
    body = [l.strip() for l in text[m.end():end].splitlines()]
    meta = text[end:]
    return [l for l in body if l and (not l.startswith(";") or MARKER in l)], meta


def analyse(text):
    ins, meta = _kernel(text)
    bar = next(i for i, l in enumerate(ins) if l.startswith("s_barrier"))
    marker = next((i for i, l in enumerate(ins) if MARKER in l), None)
    vl = [i for i, l in enumerate(ins[:bar]) if VLOAD.match(l)]
    assert vl, "no vector load in front of the first s_barrier"
    end = marker if marker is not None else vl[-1]
    assert end < bar, "the marker stands behind the first s_barrier"
    region = ins[:end]
    labels = {l[:-1] for l in region if l.endswith(":")}
    stray = [l for l in region if re.match(r"s_c?branch", l) and l.split()[-1] not in labels]
    vm_waits = [l for l in ins[vl[0]:end] if l.startswith("s_waitcnt") and "vmcnt" in l]
    # a wait for kernel-argument loads: lgkmcnt(0) with an s_load outstanding (nothing else of that counter -- LDS, s_memtime -- is used up there)
    karg_waits, pending = 0, False
    for l in region:
        if l.startswith("s_load_"):
            pending = True
        elif l.startswith("s_waitcnt") and "lgkmcnt(0)" in l and pending:
            karg_waits += 1
            pending = False
    late = [l for l in ins[end:bar] if VLOAD.match(l)] if marker is not None else []
    scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
    return dict(marker=marker is not None, stray=stray, vm_waits=vm_waits, karg_waits=karg_waits, late=late, scratch=scratch, requests=len(vl))


def test_prologue_is_one_round_trip(kernel_text):
    r = analyse(kernel_text)
    print({k: (v if not isinstance(v, list) else len(v)) for k, v in r.items()})
    assert not r["stray"], "branches out of the prologue's text: %s" % r["stray"]
    assert not r["vm_waits"], "%d s_waitcnt vmcnt between the first vector load and the last request: %s" % (len(r["vm_waits"]), r["vm_waits"])
    assert r["karg_waits"] <= 1, "%d waits for kernel-argument loads in front of the last request" % r["karg_waits"]
    assert r["marker"], "the M-step half does not mark the end of its requests (%s)" % MARKER
    assert not r["late"], "vector loads between the marker and the first s_barrier: %s" % r["late"]


def test_no_scratch(kernel_text):
    assert analyse(kernel_text)["scratch"] == 0
