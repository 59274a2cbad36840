"""What one cloud from K cameras costs in one call against what a caller had before (profiles/rig_ab.txt is this script's output).

    python scripts/gpu_rig.py [--rounds 5] [--reps 20] [--out profiles/rig_ab.txt]

trackdlo_amd.synth rope frames (depth + mask, 45 nodes) at 640 x 480 and 1280 x 720; K = 1, 2, 3, 4 cameras, each with images of its own and -- but the first --
a rotation and a translation to the common frame.  Sides, for planes in pageable HOST memory and in DEVICE memory:
   rig       tdlo_rig_to_cloud
   np+view   the composition with the SAME result a caller has without the rig call: R formed on the host by tests/rig_ref.py (numpy), then
             tdlo_cloud_view_voxel_grid on R (device planes are brought to the host first: that is what such a caller has to do)
   cpp+view  the same with R formed by the library's host helper tdlo_rig_points_host
   singles   K x tdlo_depth_to_cloud into K slots -- for scale only: a voxel grid per camera is ANOTHER result (host planes only: the single call takes host images)
Method: one child process per image size and round, `rounds` rounds; inside a child the sides alternate (every side once per repetition, `reps` repetitions
after two untimed ones), every call returns with the stream waited for, the host clock times it, the child reports each side's mean, the route counters
45 / 46 / 47 after the timed calls and a digest of the slot's cloud (uint64 views) per side; the digests of rig, np+view and cpp+view are compared here.
Nothing here is a test gate.  This process touches no GPU itself: it starts the children one after the other, each under a time limit of its own, and stops at
the first that fails."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M, KS, LEAF = 45, (1, 2, 3, 4), 0.008
SIZES = {"640x480": (480, 640, 400000), "1280x720": (720, 1280, 600000)}      # (rows, cols, surface samples), as scripts/gpu_cloud_batch.py
SIDES = {"host": ("rig", "np+view", "cpp+view", "singles"), "device": ("rig", "np+view", "cpp+view")}


def cameras(size):
    import rig_ref, rig_scenes
    from trackdlo_amd import synth
    rows, cols, samples = SIZES[size]
    cams = []
    for k in range(max(KS)):
        depth, mask, cam, _ = synth.depth_scene(M, config=31, frame=k, rows=rows, cols=cols, samples=samples)
        T = None if k == 0 else rig_scenes.about(rig_scenes.rotation(0.02 * k, (0.2, 1.0, 0.1)), (0.0, 0.0, 0.7), (0.001 * k, 0.0, 0.0005 * k))
        cams.append(rig_ref.Cam(depth, mask, cam=(cam["fx"], cam["fy"], cam["cx"], cam["cy"]), T=T))
    return cams


def digest(X):
    return hashlib.sha256(np.ascontiguousarray(X, dtype=np.float64).view(np.uint64).tobytes()).hexdigest()[:16]


def child(size, reps):
    import torch
    import rig_ref, rig_scenes
    from trackdlo_amd import binding as B
    cams = cameras(size)
    ctx = B.Context(device=0, max_frames=max(KS), max_points=1 << 15, max_nodes=64, timing=False)
    out = {}
    for loc in ("host", "device"):
        place = None if loc == "host" else (lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda())
        for K in KS:
            sub = cams[:K]
            bc = rig_scenes.binding_cams(B, sub, place)
            torch.cuda.synchronize()

            def fetch():
                """The planes on the host, as the compositions need them."""
                if loc == "host":
                    return sub
                return [c.replaced(depth=b.depth.cpu().numpy().view(np.uint16), mask=b.mask.cpu().numpy()) for c, b in zip(sub, bc)]
            sides = {
                "rig": lambda: ctx.rig_to_cloud(0, bc, LEAF, fetch=False),
                "np+view": lambda: ctx.voxel_grid_view(0, rig_ref.points(fetch()), LEAF, want_cloud=False),
                "cpp+view": lambda: ctx.voxel_grid_view(0, B.rig_points_host(rig_scenes.binding_cams(B, fetch())), LEAF, want_cloud=False),
                "singles": lambda: [ctx.depth_to_cloud(k, c.depth, c.mask, *c.cam, LEAF, fetch=False) for k, c in enumerate(sub)],
            }
            names = SIDES[loc]
            acc = {s: 0.0 for s in names}
            dig, res = {}, {}
            for rep in range(reps + 2):
                for s in names:
                    t0 = time.perf_counter()
                    r = sides[s]()
                    dt = time.perf_counter() - t0
                    if rep >= 2:
                        acc[s] += dt
                    if rep == 0:
                        res[s] = None if s == "singles" else [int(r[1]), int(r[2])]
                        dig[s] = digest(ctx.get_cloud(0))
            out["%s K=%d" % (loc, K)] = dict(ms={s: 1e3 * acc[s] / reps for s in names}, digest=dig, n=res)
    out["routes"] = ctx.rig_route_counts()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_ab.txt"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    lines = ["# scripts/gpu_rig.py --rounds %d --reps %d: milliseconds per call (host clock, stream waited for), median over the rounds [the rounds' values]" % (a.rounds, a.reps),
             "# rig: tdlo_rig_to_cloud; np+view / cpp+view: R on the host (numpy / tdlo_rig_points_host) + tdlo_cloud_view_voxel_grid, the SAME cloud; singles: K x tdlo_depth_to_cloud,",
             "# ANOTHER result, for scale.  bits: the digests of the slot's cloud after rig, np+view and cpp+view agree.  routes: counters 45 / 46 / 47 of the child's context at its end."]
    for size in SIZES:
        runs = []
        for rnd in range(a.rounds):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", size, "--reps", str(a.reps)], capture_output=True, text=True, timeout=420)
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not got:
                print(r.stdout[-2000:] + r.stderr[-4000:])
                print("child failed (%s, round %d): stopping" % (size, rnd))
                return 1
            runs.append(json.loads(got[-1][7:]))
        lines.append("%s  routes per round %s" % (size, [r["routes"] for r in runs]))
        for loc in ("host", "device"):
            for K in KS:
                key = "%s K=%d" % (loc, K)
                d = runs[0][key]
                same = all(len({r[key]["digest"][s] for s in ("rig", "np+view", "cpp+view")}) == 1 for r in runs)
                cells = []
                for s in SIDES[loc]:
                    v = [r[key]["ms"][s] for r in runs]
                    cells.append("%s %.3f [%s]" % (s, float(np.median(v)), " ".join("%.3f" % x for x in v)))
                lines.append("  %-6s K=%d  n=%d n_raw=%d  bits %s  |  %s" % (loc, K, d["n"]["rig"][0], d["n"]["rig"][1], "equal" if same else "DIFFER", "  |  ".join(cells)))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
