"""k_iter_fused_w0 (the one-launch iteration of chains whose step slots all fit wave 0) -- checked on the compiler's output, on the CPU.

tdlo_iter_fused.hip is compiled device-only to gfx950 assembly with the Makefile's flags, as tests/test_fused_prologue_isa.py does for k_iter_fused<float>.
For k_iter_fused_w0<float>:

  * no `s_waitcnt vmcnt(..)` stands between the kernel's first vector load and the line TDLO_FUSED_PROLOGUE_REQUESTED: everything the M-step half reads
    before the recursion is ONE memory round trip, as in k_iter_fused;
  * at most one wait for kernel-argument loads stands in front of that line;
  * the kernel uses no scratch memory;
  * its text holds fewer s_barrier than k_iter_fused<float>'s in the same assembly file (the barrier behind the records, the one in front of the new state,
    the E-step half's first one and the strided backward pass are not in it).

The region in front of the marker is straight-line but for forward branches over blocks inside it (the points' `n < N0`, the priors): every branch target
has to lie inside, so that reading the text line by line covers every path.
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
SYM_W0 = r"_ZN4tdlo15k_iter_fused_w0IfEE\w+"
SYM_OLD = r"_ZN4tdlo12k_iter_fusedIfEE\w+"


def _hipcc():
    for p in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if p and os.path.exists(p):
            return p
    return None


def _makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^GPU_ARCH\s*:=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(EXTRA)", "").split()
    rule = re.search(r"^build/tdlo_iter_fused\.o:.*\n\t.*\n\t(.*)$", mk, re.M).group(1)      # the object's own recipe: no further flags
    assert "$(FLAGS)" in rule and "-mllvm" not in rule, rule
    return ["--offload-arch=" + arch] + flags


@pytest.fixture(scope="module")
def asm_text(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa_w0") / "tdlo_iter_fused.s")
    subprocess.check_call([hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", "tdlo_iter_fused.hip", "-o", out], cwd=CSRC,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernel(text, sym):
    m = re.search(r"^(%s):" % sym, text, re.M)
    assert m, "%s not in the assembly" % sym
    end = text.index(".Lfunc_end", m.end())
    body = [l.strip() for l in text[m.end():end].splitlines()]
    meta = text[end:]
    return [l for l in body if l and (not l.startswith(";") or MARKER in l)], meta


def analyse(text, sym=SYM_W0):
    ins, meta = _kernel(text, sym)
    bar = next(i for i, l in enumerate(ins) if l.startswith("s_barrier"))
    marker = next((i for i, l in enumerate(ins) if MARKER in l), None)
    assert marker is not None, "the M-step half does not mark the end of its requests (%s)" % MARKER
    assert marker < bar, "an s_barrier stands in front of the marker"
    vl = [i for i, l in enumerate(ins[:marker]) if VLOAD.match(l)]
    assert vl, "no vector load in front of the marker"
    region = ins[:marker]
    labels = {l[:-1] for l in region if l.endswith(":")}
    stray = [l for l in region if re.match(r"s_c?branch", l) and l.split()[-1] not in labels]
    vm_waits = [l for l in ins[vl[0]:marker] if l.startswith("s_waitcnt") and "vmcnt" in l]
    karg_waits, pending = 0, False
    for l in region:
        if l.startswith("s_load_"):
            pending = True
        elif l.startswith("s_waitcnt") and "lgkmcnt(0)" in l and pending:
            karg_waits += 1
            pending = False
    scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
    return dict(stray=stray, vm_waits=vm_waits, karg_waits=karg_waits, scratch=scratch, requests=len(vl),
                barriers=sum(l.startswith("s_barrier") for l in ins))


def test_prologue_is_one_round_trip(asm_text):
    r = analyse(asm_text)
    print({k: (v if not isinstance(v, list) else len(v)) for k, v in r.items()})
    assert not r["stray"], "branches out of the prologue's text: %s" % r["stray"]
    assert not r["vm_waits"], "%d s_waitcnt vmcnt between the first vector load and the last request: %s" % (len(r["vm_waits"]), r["vm_waits"])
    assert r["karg_waits"] <= 1, "%d waits for kernel-argument loads in front of the last request" % r["karg_waits"]


def test_no_scratch(asm_text):
    assert analyse(asm_text)["scratch"] == 0


def test_fewer_barriers_than_k_iter_fused(asm_text):
    new = analyse(asm_text)["barriers"]
    old = sum(l.startswith("s_barrier") for l in _kernel(asm_text, SYM_OLD)[0])
    print("s_barrier in the text: k_iter_fused_w0<float> %d, k_iter_fused<float> %d" % (new, old))
    assert new < old, (new, old)
