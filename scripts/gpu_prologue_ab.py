"""Short registrations, where the prologue is most of a call: cpd_lle with max_iter = 2 on clouds beyond the fused prologue's 16 384 points
(N = 50 000 and 20 000, M = 50, fp32 mode, sort reuse off), two resident (cloud, Y0) pairs registered alternately as bench.py does, 400 timed
calls per size behind 50 warm-up calls.  One JSON line: microseconds per call and per size, the calls the two-launch prologue served
(tdlo_debug_route_count 48; -1 from a library that lacks it) and a digest of the last results.

The library is the tree's, or TDLO_LIBRARY's (scripts/build_variant.sh); TDLO_PROLOGUE_SCAN=0 keeps the three-kernel prologue.  An A/B run
alternates the two in one GPU call (profiles/prologue_scan_ab.txt).
usage: python scripts/gpu_prologue_ab.py [--calls 400] [--warmup 50] [--iters 2]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from trackdlo_amd import binding as B, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--iters", type=int, default=2)
    a = ap.parse_args()
    P = synth.LAUNCH_PARAMS
    M = 50
    params = B.make_params(P["beta"], P["lambda_"], P["lle_weight"], P["mu"], max_iter=a.iters, tol=0.0, include_lle=False, alpha=0.0, k_vis=0.0,
                           visibility_threshold=P["visibility_threshold"], precision=B.PREC_F32)
    out = {"library": os.environ.get("TDLO_LIBRARY", "tree"), "scan_switch": os.environ.get("TDLO_PROLOGUE_SCAN", "unset"), "iters": a.iters, "calls": a.calls}
    for N in (50000, 20000):
        ctx = B.Context(device=0, max_frames=2, max_points=N, max_nodes=M, timing=False)
        ctx.set_sort_reuse(False)
        Ys = []
        for k in range(2):
            X, Y0, _ = synth.scene(N, M, config=2, frame=k)
            ctx.set_cloud(k, X)
            Ys.append(Y0)
        for i in range(a.warmup):
            ctx.cpd_lle_resident(i % 2, Ys[i % 2], 0.0, params)
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(a.calls):
            g = ctx.cpd_lle_resident(i % 2, Ys[i % 2], 0.0, params)
        ctx.synchronize()
        dt = time.perf_counter() - t0
        h = hashlib.sha256(np.ascontiguousarray(g["Y"]).tobytes() + np.float64(g["sigma2"]).tobytes()).hexdigest()[:16]
        out[f"us_per_call_N{N}"] = round(dt * 1e6 / a.calls, 3)
        out[f"digest_N{N}"] = f"{h}/{g['iters']}/{g['n_kept']}"
        out[f"scan_calls_N{N}"] = int(ctx.lib.tdlo_debug_route_count(ctx.h, 48))
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
