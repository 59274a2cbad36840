"""What the voxel grid on a cloud view costs beside the depth path's multi-launch form (profiles/voxel_view_ab.txt holds a run, or says that none was made).

  python scripts/gpu_voxel_view.py --mode ab [--parent-lib PATH]
      A 1280 x 720 rope frame (synth.depth_scene, ~30 000 masked pixels).  Side A (--mode depth, a child process): tdlo_depth_to_cloud on the images
      under TDLO_CLOUD_FUSED=0 (the multi-launch form; with --parent-lib the library of the parent commit, through TDLO_LIBRARY).  Side B (--mode view,
      a child process): tdlo_cloud_view_voxel_grid on the SAME points -- tests/voxel_ref.py's backproject of the frame, packed float32 -- from host
      memory and from a device tensor.  Host clock around calls that end in a stream wait, after warm-up; five alternating pairs on one box, every
      value printed (ms per call, mean of --calls calls).  B's outputs are compared on bits with the depth path before anything is timed.
  python scripts/gpu_voxel_view.py --mode alone
      The new call alone: 30 000 raw points (the rope's), 921 600 points (an organized 1280 x 720 cloud, NaN where the depth is 0, ~3 % selected by
      the mask), 2 000 000 kept points as packed float32 host, xyz_ device and float64 device.  Printed with the algorithmic bytes of the view-reading
      passes: 12 B per addressed float point per reading pass (bounding box, keys; the centroid pass reads the kept points once more), 16 B per
      padded point if whole lines are pulled.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o vv -- python scripts/gpu_voxel_view.py --mode alone --calls 5
  python scripts/gpu_voxel_view.py --mode summarize --trace DIR
      Per-kernel times from the kernel trace: total and share per kernel name (k_cloud_bbox / k_cloud_keys / k_cloud_centroid by source, the radix
      passes, k_scan_single -- its share at 2 000 000 points is the question the trace answers).
  python scripts/gpu_voxel_view.py --mode team-frames --frames FILE.npz
      Writes the frames of the one-launch route's measurement: organized clouds of 640 x 480 and 1280 x 720 (synth.depth_scene, the rope's radius chosen
      so that the mask keeps about 10 000 and 30 000 pixels -- and 36 000, more than the kernel takes: a call it passes on), no GPU needed.
  python scripts/gpu_voxel_view.py --mode team-ab --frames FILE.npz --parent-lib PATH
      The view route in ONE launch (k_cloud_team over the view) against the parent commit: per frame tdlo_cloud_view_voxel_grid and
      tdlo_tracker_frame_from_cloud_view on the organized cloud + mask, from a device tensor and from host memory, and beside them tdlo_depth_to_cloud and
      tdlo_tracker_frame_from_depth on the same frame (the figure the route is modelled on).  --rounds alternating pairs of child processes (--mode
      team-side; the parent's library through TDLO_LIBRARY), each under its own time limit; every value is printed, then per measured call whether every
      value of this tree lies below every value of the parent.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o vt -- python scripts/gpu_voxel_view.py --mode team-side --frames FILE.npz --calls 5
  python scripts/gpu_voxel_view.py --mode summarize --trace DIR
      k_cloud_team's view instantiations alone, in a run of their own.
Any HIP error raises: the process exits non-zero."""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("ab", "depth", "view", "alone", "summarize", "team-frames", "team-side", "team-ab"), required=True)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--leaf", type=float, default=0.008)
ap.add_argument("--parent-lib", default=None, help="ab: libtrackdlo_hip.so of the parent commit for side A")
ap.add_argument("--frames", default=None, help="team-*: the .npz of frames (team-frames writes it)")
ap.add_argument("--trace", default=None, help="summarize: the directory rocprofv3 wrote")
args = ap.parse_args()


def ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def rounds_of(alts, calls):
    for _, fn in alts:
        ms(fn, 3)
    rows = {name: [] for name, _ in alts}
    for _ in range(args.rounds):
        for name, fn in alts:
            rows[name].append(ms(fn, calls))
    for name, _ in alts:
        v = rows[name]
        print(f"  {name:44s} " + " ".join(f"{x:9.4f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:9.4f}")


def rope_frame():
    from trackdlo_amd import synth
    depth, mask, cam, _ = synth.depth_scene(45, config=4, rows=720, cols=1280)
    return depth, mask, cam


def depth_side():
    """Side A, one process: tdlo_depth_to_cloud in its multi-launch form (TDLO_CLOUD_FUSED=0 is set by the parent), whatever library TDLO_LIBRARY names."""
    from trackdlo_amd import binding as B
    depth, mask, cam = rope_frame()
    k = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    ctx = B.Context(device=0, max_points=1 << 16, timing=False)
    assert os.environ.get("TDLO_CLOUD_FUSED") == "0"
    X, n, n_raw = ctx.depth_to_cloud(0, depth, mask, *k, args.leaf)
    fn = lambda: ctx.depth_to_cloud(0, depth, mask, *k, args.leaf, fetch=False)
    ms(fn, 3)
    print(f"  A  depth_to_cloud, multi-launch form ({n_raw} -> {n}): {ms(fn, args.calls):9.4f} ms per call (mean of {args.calls})", flush=True)
    assert ctx.cloud_route_counts()[0] == 0
    ctx.close()


def view_side():
    """Side B, one process: tdlo_cloud_view_voxel_grid on the same points, checked on bits against the depth path of this library first."""
    import numpy as np
    import torch
    import voxel_ref as R
    from trackdlo_amd import binding as B
    depth, mask, cam = rope_frame()
    k = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    P = R.backproject(depth, mask, *k)
    Pd = torch.from_numpy(P).cuda()
    ctx = B.Context(device=0, max_frames=2, max_points=1 << 16, timing=False)
    Xa, n, n_raw = ctx.depth_to_cloud(1, depth, mask, *k, args.leaf)
    for name, src in (("B1 voxel_grid_view, packed float32 host", P), ("B2 voxel_grid_view, packed float32 device", Pd)):
        Xb, nb, nrawb = ctx.voxel_grid_view(0, src, args.leaf)
        assert (n, n_raw) == (nb, nrawb) and np.array_equal(Xa.view(np.uint64), Xb.view(np.uint64))
        fn = lambda: ctx.voxel_grid_view(0, src, args.leaf, want_cloud=False)
        ms(fn, 3)
        print(f"  {name} ({n_raw} -> {n}): {ms(fn, args.calls):9.4f} ms per call (mean of {args.calls})", flush=True)
    ctx.close()


def ab():
    """Alternating pairs of child processes on one box: A (the parent commit's library when --parent-lib names it), then B."""
    import subprocess
    me = [sys.executable, os.path.abspath(__file__), "--calls", str(args.calls), "--leaf", str(args.leaf)]
    env_a = dict(os.environ, TDLO_CLOUD_FUSED="0")
    if args.parent_lib:
        env_a["TDLO_LIBRARY"] = os.path.abspath(args.parent_lib)
    print(f"1280 x 720 rope frame, leaf {args.leaf}; side A library: {args.parent_lib or 'this tree'}")
    for r in range(args.rounds):
        print(f"pair {r + 1}", flush=True)
        subprocess.run(me + ["--mode", "depth"], env=env_a, check=True, timeout=300)
        subprocess.run(me + ["--mode", "view"], env=dict(os.environ), check=True, timeout=300)


def alone():
    import numpy as np
    import torch
    import voxel_ref as R
    from trackdlo_amd import binding as B, synth
    ctx = B.Context(device=0, max_points=1 << 16, timing=False)
    depth, mask, cam = rope_frame()
    k = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    rope = R.backproject(depth, mask, *k)
    org = R.backproject(depth, np.ones_like(mask), *k)
    org[(depth == 0).reshape(-1)] = np.nan
    big = np.concatenate([synth.scene(250000, 45, config=4, frame=f)[0] for f in range(8)], axis=0).astype(np.float32)
    xyz_ = np.full((big.shape[0], 4), np.nan, dtype=np.float32); xyz_[:, :3] = big
    cases = [("30 000 raw points, packed float32 host", rope, None, 1),
             ("30 000 raw points, packed float32 device", torch.from_numpy(rope).cuda(), None, 1),
             ("921 600 organized, ~3 % selected, host", org, mask.reshape(-1), 1),
             ("921 600 organized, ~3 % selected, device", torch.from_numpy(org).cuda(), torch.from_numpy(mask.reshape(-1).copy()).cuda(), 1),
             ("2 000 000 kept, packed float32 host", big, None, 4),
             ("2 000 000 kept, xyz_ device", torch.from_numpy(xyz_).cuda(), None, 4),
             ("2 000 000 kept, float64 device", torch.from_numpy(big.astype(np.float64)).cuda(), None, 4)]
    for name, src, sel, div in cases:
        N = int(src.shape[0])
        _, n, n_raw = ctx.voxel_grid_view(0, src, args.leaf, select=sel, want_cloud=False)
        print(f"{name}: N = {N}, kept {n_raw} -> {n} points; reading passes over the view: 2 x {12 * N} B addressed ({16 * N} B as whole 16-byte points) + {12 * n_raw} B gathered")
        rounds_of([("voxel_grid_view", lambda: ctx.voxel_grid_view(0, src, args.leaf, select=sel, want_cloud=False))], max(2, args.calls // div))
    ctx.close()


def summarize():
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {args.trace}"
    rows = list(csv.DictReader(open(files[0])))

    def col(*parts):
        for c in rows[0]:
            if all(p in c.lower() for p in parts):
                return c
        raise KeyError(parts)

    kn, ks, ke = col("kernel", "name"), col("start"), col("end")
    tot = {}
    for r in rows:
        name = r[kn].split("(")[0]
        t = tot.setdefault(name, [0, 0.0]); t[0] += 1; t[1] += (int(r[ke]) - int(r[ks])) * 1e-3
    whole = sum(t[1] for t in tot.values())
    for name, (cnt, us) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
        print(f"{us:12.1f} us {100 * us / whole:5.1f} %  {cnt:6d} x {us / cnt:9.2f} us  {name}")


TEAM_FRAMES = (("640x480", 480, 640), ("1280x720", 720, 1280))
TEAM_KEPT = (10000, 30000, 36000)      # the last: more kept points than the one-launch kernel takes (32 704) -- what a passed-on call costs, beside the condition


def team_frames():
    import numpy as np
    from trackdlo_amd import synth
    out = {}
    for tag, rows, cols in TEAM_FRAMES:
        for want in TEAM_KEPT:
            radius = 0.006
            for _ in range(4):
                depth, mask, cam, Y0 = synth.depth_scene(45, config=4, rows=rows, cols=cols, radius=radius, samples=3000000)
                got = int((mask != 0).sum())
                if abs(got - want) <= want // 20:
                    break
                radius *= want / got
            key = f"{tag}_{want}"
            print(f"{key}: radius {radius:.5f} m, the mask keeps {got} pixels")
            out[key + "_depth"] = depth; out[key + "_mask"] = mask; out[key + "_Y0"] = Y0
            out[key + "_cam"] = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]])
    np.savez_compressed(args.frames, **out)


def team_side():
    """One process, whatever library TDLO_LIBRARY names: RESULT <frame> <call> <ms per call> lines."""
    import numpy as np
    import torch
    import voxel_ref as R
    from trackdlo_amd import binding as B, synth
    z = np.load(args.frames)
    Pm = synth.LAUNCH_PARAMS
    ctx = B.Context(device=0, max_frames=2, max_points=1 << 16, timing=False)
    for tag, rows, cols in TEAM_FRAMES:
        for want in TEAM_KEPT:
            key = f"{tag}_{want}"
            depth, mask, Y0, k = z[key + "_depth"], z[key + "_mask"], z[key + "_Y0"], tuple(float(x) for x in z[key + "_cam"])
            org = R.backproject(depth, np.ones_like(mask), *k)
            sel = np.ascontiguousarray(mask.reshape(-1))
            org_d, sel_d = torch.from_numpy(org).cuda(), torch.from_numpy(sel.copy()).cuda()
            Xa, n, n_raw = ctx.depth_to_cloud(1, depth, mask, *k, args.leaf)
            for src, s in ((org, sel), (org_d, sel_d)):
                Xb, nb, nrawb = ctx.voxel_grid_view(0, src, args.leaf, select=s)
                assert (n, n_raw) == (nb, nrawb) and np.array_equal(Xa.view(np.uint64), Xb.view(np.uint64))
            M = Y0.shape[0]
            coord = synth.geodesic_coord(Y0)
            # (visibility threshold 5 cm: the thick ropes' visible surface lies up to 27 mm from the centreline the nodes start on)
            trk = B.trackdlo(M, 0.05, Pm["beta"], Pm["lambda_"], Pm["alpha"], Pm["k_vis"], Pm["mu"], 30, Pm["tol"], Pm["beta_pre_proc"],
                             Pm["lambda_pre_proc"], Pm["lle_weight"], ctx=ctx)
            trk.initialize_nodes(Y0); trk.initialize_geodesic_coord(coord)      # (the coordinates once: a second call appends, as the reference's does)

            def timed(name, fn, tracker=False):
                if tracker:
                    trk.initialize_nodes(Y0)
                ms(fn, 3)
                print(f"RESULT {key}({n_raw}->{n}) {name} {ms(fn, args.calls):.4f}", flush=True)

            timed("view_voxel_grid,device", lambda: ctx.voxel_grid_view(0, org_d, args.leaf, select=sel_d, want_cloud=False))
            timed("view_voxel_grid,host", lambda: ctx.voxel_grid_view(0, org, args.leaf, select=sel, want_cloud=False))
            timed("tracker_frame_from_cloud_view,device", lambda: trk.frame_from_cloud_view(org_d, args.leaf, 0.06, select=sel_d), True)
            timed("tracker_frame_from_cloud_view,host", lambda: trk.frame_from_cloud_view(org, args.leaf, 0.06, select=sel), True)
            timed("(model)depth_to_cloud", lambda: ctx.depth_to_cloud(1, depth, mask, *k, args.leaf, fetch=False))
            timed("(model)tracker_frame_from_depth", lambda: trk.frame_from_depth(depth, mask, *k, args.leaf, 0.06), True)
            del trk
    rc = [int(ctx.lib.tdlo_debug_route_count(ctx.h, w)) for w in (21, 27, 28, 29)]
    print(f"route counts 21 / 27 / 28 / 29: {rc}", flush=True)
    ctx.close()


def team_ab():
    import subprocess
    assert args.parent_lib and args.frames
    me = [sys.executable, os.path.abspath(__file__), "--calls", str(args.calls), "--leaf", str(args.leaf), "--frames", args.frames, "--mode", "team-side"]
    sides = (("parent", dict(os.environ, TDLO_LIBRARY=os.path.abspath(args.parent_lib))), ("this", dict(os.environ)))
    vals = {}
    for r in range(args.rounds):
        for side, env in sides:
            run = subprocess.run(me, env=env, timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            out = run.stdout
            if run.returncode != 0:
                print(f"pair {r + 1}, {side} tree: exit status {run.returncode}\n" + out, flush=True)
                sys.exit(1)
            print(f"pair {r + 1}, {side} tree:\n" + out, flush=True)
            for line in out.splitlines():
                if line.startswith("RESULT "):
                    _, frame, name, v = line.split()
                    vals.setdefault((frame, name), {}).setdefault(side, []).append(float(v))
    print("ms per call (mean of %d), every pair's value; below = every value of this tree below every value of the parent" % args.calls)
    for (frame, name), d in vals.items():
        p, t = d["parent"], d["this"]
        passed_on = int(frame.split("(")[1].split("-")[0]) > 32704
        verdict = "(model)" if name.startswith("(model)") else ("below" if max(t) < min(p) else "NOT BELOW") + (" (passed on: beside the condition)" if passed_on else "")
        print(f"  {frame:26s} {name:38s} parent " + " ".join(f"{x:7.4f}" for x in p) + "   this " + " ".join(f"{x:7.4f}" for x in t) + f"   {verdict}")


{"team-frames": team_frames, "team-side": team_side, "team-ab": team_ab, "ab": ab, "depth": depth_side, "view": view_side, "alone": alone, "summarize": summarize}[args.mode]()
