"""Phase stamps of the M-step half of k_iter_fused (workgroup 0, thread 0) at the headline's shape (C2: N = 50 000, M = 50, 50 iterations).

Needs a library built with -DTDLO_CHAIN_STAMPS ALONE (-DTDLO_ESTEP_STAMPS uses two of the same words):
    bash scripts/build_variant.sh stamps -DTDLO_CHAIN_STAMPS
    TDLO_LIBRARY=scripts/tmp/libtrackdlo_stamps.so python scripts/gpu_fused_stamps.py
The fused kernel stamps into words 56 .. 63 of the slot's stamp block (tdlo_mstep_chain_body.h, CSTAMP): what is read back is the LAST launch of the loop.
Shader clocks (s_memtime), relative to stamp 0 = the M-step half's first statement.
A library built with BOTH -DTDLO_CHAIN_STAMPS and -DTDLO_ESTEP_STAMPS (the fused kernel's two halves stamp into different words: 56 .. 63 and 40 .. 48, the same
thread, the same clock) also gives the E-step half's stamps on the same axis: where the half starts, where it stands behind its first barrier (k_iter_fused) or at
the place of it (k_iter_fused_w0, which leaves it out), where its sums are on their way to memory.
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from trackdlo_amd import binding as B, synth

NAMES = ["entry", "requests out, state checked (one round trip)", "sums in LDS", "records in LDS", "forward pass", "gains + junction",
         "backward pass", "nodes, sigma2 sums"]


def main():
    P = synth.LAUNCH_PARAMS
    ctx = B.Context(max_points=1 << 16)
    X, Y0, _ = synth.scene(50000, 50, config=2)
    pr = B.make_params(P['beta'], P['lambda_'], P['lle_weight'], P['mu'], 50, 0.0, False)
    ctx.cpd_lle(X, Y0, 0.0, pr)
    rows, erows, have_e = [], [], True
    for _ in range(int(os.environ.get("REPS", "9"))):
        g = ctx.cpd_lle_resident(0, Y0, 0.0, pr)
        st = ctx.debug_stamps(64).astype(np.int64)
        rows.append(st[56:64] - st[56])
        erows.append(st[40:49] - st[56])
        have_e = have_e and st[41] != 0
    rows = np.array(rows)
    print("iterations", g["iters"], "loop_ms", g["loop_ms"])
    print("k_iter_fused, M-step half, clocks since entry (median of %d registrations; min .. max):" % len(rows))
    med = np.median(rows, axis=0).astype(np.int64)
    for i, n in enumerate(NAMES):
        print("  %d  %-48s %7d   (+%5d)   %d .. %d" % (i, n, med[i], med[i] - (med[i - 1] if i else 0), rows[:, i].min(), rows[:, i].max()))
    if have_e:
        erows = np.array(erows)
        emed = np.median(erows, axis=0).astype(np.int64)
        print("E-step half (workgroup 0, thread 0), clocks since the M-step half's entry:")
        for i, n in ((0, "first statement"), (1, "front done (behind / at the place of its first barrier)"), (7, "last stamp")):
            print("  E%d %-56s %7d   (+%5d since the M-step half's last stamp)   %d .. %d" % (i, n, emed[i], emed[i] - med[7], erows[:, i].min(), erows[:, i].max()))
    ctx.close()


if __name__ == "__main__":
    main()
