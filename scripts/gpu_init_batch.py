"""F trackers started in one call (tdlo_tracker_initialize_from_cloud_batch) against F single calls (profiles/init_batch_ab.txt is this script's output).

    python scripts/gpu_init_batch.py --parent-lib PATH/libtrackdlo_hip.so [--pairs 5] [--out profiles/init_batch_ab.txt]

Synthetic ropes near the origin (tests/init_ref.py, rope_cloud), a cloud of its own per slot: N = 5 000 / M = 45 and N = 500 / M = 45, mu 0.05, 100 iterations
of reg, F = 1, 2, 3, 8, 32.  The method of profiles/init_ab.txt: one child process per side and pair, alternating, five pairs; a child makes one context of 32
slots, puts the clouds into the slots once (tdlo_set_cloud; not timed), and per size and F makes two warm-up calls and then times `reps` calls with the host
clock -- every call returns with the stream waited for -- and reports their mean.  A line holds the five values, their median and their spread (max - min).
   batch   this tree's library under TDLO_INIT_BATCH_MIN=1: the batch launches at every F, F = 1 included
   single  F x tdlo_tracker_initialize_from_cloud(X = NULL), against the PARENT commit's library (--parent-lib, handed to the child through TDLO_LIBRARY);
           without --parent-lib this tree's library stands in, and the output says so
The rule for the library's default (csrc/tdlo_api.cpp, kInitBatchMin): the batch launches serve every F from the smallest F at which, at both sizes, their
median is below the single calls' by more than both spreads, and so for every larger F measured; printed at the end.  If there is no such F the batch ships
off by default.  Nothing here is a test gate.
This process touches no GPU itself: it starts the children one after the other, each under a time limit of its own, and stops at the first that fails."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((5000, 45), (500, 45))
FS = (1, 2, 3, 8, 32)
MU, ITERS, SLOTS = 0.05, 100, 32


def child(side, reps):
    import init_ref as R
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, max_frames=SLOTS, timing=False)
    out = {}
    for N, M in SIZES:
        for s in range(SLOTS):
            ctx.set_cloud(s, R.rope_cloud(N, seed=1000 * N + s))
        trk = [B.trackdlo(M, ctx=ctx, slot=s, precision=B.PREC_F64) for s in range(SLOTS)]
        tab = (C.c_void_p * SLOTS)(*[t.h for t in trk])
        s2 = np.zeros(SLOTS); rcs = np.zeros(SLOTS, dtype=np.int32)
        one = C.c_double(0.0)
        lib = ctx.lib

        def batch(F):
            ctx._chk(lib.tdlo_tracker_initialize_from_cloud_batch(C.cast(tab, C.c_void_p), F, MU, ITERS, s2.ctypes.data, rcs.ctypes.data))

        def single(F):
            for i in range(F):
                ctx._chk(lib.tdlo_tracker_initialize_from_cloud(trk[i].h, None, 0, MU, ITERS, C.byref(one)))

        fn = batch if side == "batch" else single
        for F in FS:
            fn(F); fn(F)
            t0 = time.perf_counter()
            for _ in range(reps):
                fn(F)
            out[f"{N}:{F}"] = (time.perf_counter() - t0) / reps * 1e3
        if side == "batch":
            out[f"{N}:routes"] = ctx.init_batch_route_counts()
        del trk
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_batch_ab.txt"))
    ap.add_argument("--child", default=None)
    o = ap.parse_args()
    if o.child:
        return child(o.child, o.reps)
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(o.reps)]
    env_b = dict(os.environ, TDLO_INIT_BATCH_MIN="1")
    env_s = dict(os.environ)
    if o.parent_lib:
        env_s["TDLO_LIBRARY"] = os.path.abspath(o.parent_lib)
    vals = {"batch": {}, "single": {}}
    text = ["F trackers started in one call (tdlo_tracker_initialize_from_cloud_batch, TDLO_INIT_BATCH_MIN=1) against F x tdlo_tracker_initialize_from_cloud on the "
            + ("PARENT commit's library" if o.parent_lib else "SAME library (no --parent-lib was given)") + ".\n"
            f"scripts/gpu_init_batch.py: one child process per side and pair, alternating, {o.pairs} pairs; ms per call, mean of {o.reps} calls after two warm-up calls;\n"
            f"rope clouds of tests/init_ref.py, one per slot, resident before the clock starts; mu {MU}, {ITERS} iterations.  Nothing here is a gate.\n"]
    failed = None
    for k in range(o.pairs):
        for side, env in (("batch", env_b), ("single", env_s)):
            print(f"pair {k + 1}, {side} ...", flush=True)
            try:
                r = subprocess.run(me + ["--child", side], env=env, capture_output=True, text=True, timeout=240)
            except subprocess.TimeoutExpired:
                failed = f"pair {k + 1}, {side}: ran into its time limit; nothing further was started\n"
                break
            res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not res:
                failed = f"pair {k + 1}, {side}: ended with {r.returncode}; nothing further was started\n{r.stderr[-3000:]}\n"
                break
            for key, v in json.loads(res[0][7:]).items():
                vals[side].setdefault(key, []).append(v)
        if failed:
            break
    if failed:
        text.append(failed)
    else:
        wins = {}
        for N, M in SIZES:
            text.append(f"== N = {N}, M = {M}   (frames of the batch side served by the batch launches / handed to the single call: {vals['batch'][f'{N}:routes'][-1]}) ==\n")
            for F in FS:
                b = np.array(vals["batch"][f"{N}:{F}"]); s = np.array(vals["single"][f"{N}:{F}"])
                sb, ss = float(b.max() - b.min()), float(s.max() - s.min())
                mb, ms = float(np.median(b)), float(np.median(s))
                text.append(f"   F = {F}\n")
                for label, v, m, sp in (("initialize_from_cloud_batch", b, mb, sb), (f"{F} x initialize_from_cloud", s, ms, ss)):
                    text.append(f"      {label:<32}" + "".join(f"{x:10.4f}" for x in v) + f"   median{m:10.4f}   spread{sp:8.4f}\n")
                won = ms - mb > max(sb, ss)
                wins[(N, F)] = won
                text.append(f"      batch / single = {mb / ms:.3f}; the batch's median below the single calls' by more than both spreads: {won}\n")
        first = next((F for F in FS if all(wins[(N, G)] for N, _ in SIZES for G in FS if G >= F)), None)
        text.append(f"kInitBatchMin by the rule (both sizes, every measured F from it on): {first if first else 'none -- the batch loses somewhere at every F: off by default'}\n")
    out = "".join(text)
    print(out)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(out)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
