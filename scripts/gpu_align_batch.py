"""What aligning the raw depth of J cameras costs in ONE call against J single calls (profiles/align_batch_ab.txt is this script's output).

    python scripts/gpu_align_batch.py --parent-lib PATH/libtrackdlo_hip.so [--rounds 5] [--reps 20] [--out profiles/align_batch_ab.txt]

Dense depth images as a sensor delivers them (scripts/gpu_align.py's scene: a wall at 1.5 m with 10 % holes, a rope-like band at 0.8 m in front of it; job j's image
is the scene shifted by j pixels, a buffer of its own), a small rotation and a 15 mm baseline between the cameras; J = 1, 2, 3, 4, 8, 32 jobs.  Four lines:
640 x 480 -> 640 x 480 and 848 x 480 -> 1280 x 720, each from DEVICE depth and from PAGEABLE HOST depth.
   batch   this tree's library under TDLO_ALIGN_BATCH_MIN=1 (k_align_splat_batch / k_align_pack_batch at every J, J = 1 included): tdlo_align_depth_batch with
           counts, the planes left in the context's arena -- one host wait
   looped  the PARENT commit's library (--parent-lib, handed to the child through TDLO_LIBRARY; without it this tree's library stands in and the output says so):
           J x tdlo_align_depth, each with aligned_out in device memory -- the device-to-device copy a caller needs to keep its plane -- and its own host wait
The method of profiles/frame_view_batch_ab.txt: one child process per side and round, the sides alternating; a child calls every shape twice before it is timed,
then times `reps` calls with the host clock (every call returns with the stream waited for) and reports their mean.  Every compared pair is checked bit-equal:
each child reports a digest of the 32 planes and counts of every line's J = 32 call, and the two sides' digests are compared here before a value is used.
The rule for kAlignBatchMin (csrc/tdlo_api.cpp), set beforehand: the smallest J from which every batch value lies below every looped value on all four lines,
1025 where no J up to 32 does.
The rig frame (K = 3 cameras at 640 x 480, a rope of 45 nodes; no threshold, the record): tdlo_tracker_frame_from_rig_aligning (this tree) against the
composition by hand through the parent library (3 x tdlo_align_depth with a device aligned_out, then tdlo_tracker_frame_from_rig) and against
tdlo_tracker_frame_from_rig on planes aligned beforehand (what alignment adds to a rig frame).
This process touches no GPU itself; it starts the children one after the other, each under a time limit of its own, and stops at the first that fails.
--child prof: 20 calls of the J = 3 device line at 848 x 480 -> 1280 x 720, for a kernel trace (profiles/align_batch_kernel_stats.csv)."""
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

JS = (1, 2, 3, 4, 8, 32)
SHAPES = {"640x480->640x480": (480, 640, 480, 640), "848x480->1280x720": (480, 848, 720, 1280)}
LINES = [(s, src) for s in SHAPES for src in ("device", "host")]


def scene(rows_d, cols_d, rows_c, cols_c):
    import align_ref as AR
    s = AR.scene_rope(rows_d, cols_d, rows_c, cols_c)
    rng = np.random.default_rng(5)
    wall = (1500 + rng.integers(0, 8, (rows_d, cols_d))).astype(np.uint16)
    wall[rng.random((rows_d, cols_d)) < 0.1] = 0
    s["D"] = np.where(s["D"] != 0, s["D"], wall)
    return s


def timed_mean(fn, reps):
    fn(); fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def child_lines(side, reps):
    import torch
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, timing=False)
    out = {}
    for shape, dims in SHAPES.items():
        s = scene(*dims)
        p = B.make_align_params(**s["p"])
        imgs = [np.ascontiguousarray(np.roll(s["D"], j, axis=1)) for j in range(max(JS))]
        devs = [torch.from_numpy(d.view(np.int16)).cuda() for d in imgs]
        keep = [torch.zeros((dims[2], dims[3]), dtype=torch.int16, device="cuda") for _ in range(max(JS))]
        for src in ("device", "host"):
            views = [B.image_view(devs[j], format=B.IMG_U16C1) if src == "device" else B.image_view(imgs[j]) for j in range(max(JS))]
            jobs = [B.make_align_job(v, p) for v in views]
            for J in JS:
                if side == "batch":
                    fn = lambda: ctx.align_depth_batch(jobs[:J], out=None, counts=True)
                else:
                    def fn():
                        for j in range(J):
                            ctx.align_depth(views[j], p, out=keep[j].data_ptr())
                out[f"{shape}:{src}:{J}"] = timed_mean(fn, reps)
            h = hashlib.sha1()                                   # the J = 32 call's planes and counts
            if side == "batch":
                A, cnt, _ = ctx.align_depth_batch(jobs, out="host")
            else:
                A, cnt = [], []
                for j in range(max(JS)):
                    _, n, _ = ctx.align_depth(views[j], p, out=keep[j].data_ptr())
                    torch.cuda.synchronize()
                    A.append(keep[j].cpu().numpy().view(np.uint16)); cnt.append(n)
            for a, n in zip(A, cnt):
                h.update(np.ascontiguousarray(a).tobytes()); h.update(np.asarray(n, np.int64).tobytes())
            out[f"{shape}:{src}:digest"] = h.hexdigest()
            out[f"{shape}:{src}:used"] = int(cnt[0][1])
    if side == "batch":
        out["routes"] = ctx.align_batch_route_counts()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def child_rig(side, reps):
    """side: aligning (this tree's call) / hand (tdlo_align_depth x 3 + tdlo_tracker_frame_from_rig) / aligned (tdlo_tracker_frame_from_rig on planes aligned
    beforehand).  Every side makes the same 30 + 2 + reps calls, so the trackers' final states are comparable."""
    import torch
    import align_ref as AR
    import colour_ref
    from trackdlo_amd import binding as B, synth
    P = synth.LAUNCH_PARAMS
    M, rows, cols, K = 45, 480, 640, 3
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    depth, _, _, mask, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=1, rows=rows, cols=cols)
    a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    ctx = B.Context(device=0, timing=False)
    t = B.trackdlo(*args, ctx=ctx)
    t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
    raw_dev = torch.from_numpy(depth.view(np.int16)).cuda()
    mask_dev = torch.from_numpy(mask).cuda()
    ps, to_rig = [], []
    for k in range(K):
        pd = AR.params(rows, cols, a[:2], a[2:], rows, cols, a[:2], a[2:], AR.transform(AR.rot("z", 0.05 + 0.02 * k), (0.001, 0.0002 * k, 0.0)))
        ps.append(B.make_align_params(**pd))
        to_rig.append(np.hstack([np.eye(3), np.array([[0.0004 * k], [-0.0003 * k], [0.0002 * k]])]))
    view = B.image_view(raw_dev, format=B.IMG_U16C1)
    keep = [torch.zeros((rows, cols), dtype=torch.int16, device="cuda") for _ in range(K)]
    rc_raw = [B.RigCamera(None, mask=mask_dev, cam=a, cam_to_rig=to_rig[k]) for k in range(K)]
    rc_kept = [B.RigCamera(keep[k], mask=mask_dev, cam=a, cam_to_rig=to_rig[k]) for k in range(K)]
    raw = [B.make_align_job(view, ps[k]) for k in range(K)] if side == "aligning" else None
    for k in range(K):                                           # (the planes aligned beforehand)
        ctx.align_depth(view, ps[k], out=keep[k].data_ptr())

    def aligning():
        return t.frame_from_rig_aligning(rc_raw, raw, 0.008, 0.06)

    def hand():
        for k in range(K):
            ctx.align_depth(view, ps[k], out=keep[k].data_ptr())
        return t.frame_from_rig(rc_kept, 0.008, 0.06)

    def aligned():
        return t.frame_from_rig(rc_kept, 0.008, 0.06)

    fn = dict(aligning=aligning, hand=hand, aligned=aligned)[side]
    for _ in range(30):                                          # the tracker onto its rope: from here on both registrations stop early
        got = fn()
    ms = timed_mean(fn, reps)
    h = hashlib.sha1(np.ascontiguousarray(t.get_tracking_result()).view(np.uint64).tobytes())
    h.update(np.ascontiguousarray(ctx.get_cloud(0)).view(np.uint64).tobytes())
    ctx.close()
    print("RESULT " + json.dumps({"ms": ms, "digest": h.hexdigest(), "points": int(got[2])}), flush=True)


def child_prof():
    import torch
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, timing=False)
    dims = SHAPES["848x480->1280x720"]
    s = scene(*dims)
    p = B.make_align_params(**s["p"])
    devs = [torch.from_numpy(np.ascontiguousarray(np.roll(s["D"], j, axis=1)).view(np.int16)).cuda() for j in range(3)]
    jobs = [B.make_align_job(B.image_view(d, format=B.IMG_U16C1), p) for d in devs]
    for _ in range(22):
        ctx.align_depth_batch(jobs, out=None, counts=True)
    print("routes", ctx.align_batch_route_counts(), flush=True)
    ctx.close()


def run_child(me, mode, env, limit=240):
    try:
        r = subprocess.run(me + ["--child", mode], env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None, f"{mode}: ran into its time limit; nothing further was started\n"
    res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not res:
        return None, f"{mode}: ended with {r.returncode}; nothing further was started\n{r.stderr[-3000:]}\n"
    return json.loads(res[0][7:]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_batch_ab.txt"))
    ap.add_argument("--child", default=None)
    o = ap.parse_args()
    if o.child:
        if o.child == "prof":
            return child_prof()
        kind, side = o.child.split(":")
        return child_lines(side, o.reps) if kind == "lines" else child_rig(side, o.reps)
    assert o.rounds >= 5 and o.reps >= 20, "at least 5 rounds of at least 20 calls"
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(o.reps)]
    env_b = dict(os.environ, TDLO_ALIGN_BATCH_MIN="1")
    env_b.pop("TDLO_LIBRARY", None); env_b.pop("TDLO_ALIGN", None)
    env_s = dict(os.environ)
    env_s.pop("TDLO_ALIGN", None); env_s.pop("TDLO_ALIGN_BATCH_MIN", None)
    if o.parent_lib:
        env_s["TDLO_LIBRARY"] = os.path.abspath(o.parent_lib)
    who = "the PARENT commit's library" if o.parent_lib else "the SAME library (no --parent-lib was given)"
    text = [f"Raw depth aligned for J cameras in one call (tdlo_align_depth_batch under TDLO_ALIGN_BATCH_MIN=1: k_align_splat_batch / k_align_pack_batch, counts fetched, one "
            f"wait) against J x tdlo_align_depth with a device aligned_out (the copy a caller needs to keep its plane) through {who}.\n"
            f"scripts/gpu_align_batch.py: one child process per side and round, alternating, {o.rounds} rounds; ms per call, mean of {o.reps} calls after two warm-up calls;\n"
            "host clock around calls that return with the stream waited for; dense depth images.  Nothing here is a gate.\n"]
    failed = None
    vals = {"batch": {}, "looped": {}}
    for k in range(o.rounds):
        for side, env in (("batch", env_b), ("looped", env_s)):
            print(f"round {k + 1}, {side} ...", flush=True)
            res, failed = run_child(me, "lines:" + side, env)
            if failed:
                break
            for key, v in res.items():
                vals[side].setdefault(key, []).append(v)
        if failed:
            break
    wins = {}
    if not failed:
        same = {f"{s}:{src}": set(vals["batch"][f"{s}:{src}:digest"]) == set(vals["looped"][f"{s}:{src}:digest"]) and len(set(vals["batch"][f"{s}:{src}:digest"])) == 1 for s, src in LINES}
        text.append(f"the 32 planes and counts of the two sides equal bit for bit after the J = 32 call, per line: {same}\n"
                    f"what the batch child's calls add up to in the counters 61 / 62 / 63: {vals['batch']['routes'][-1]}\n")
        if not all(same.values()):
            failed = "the two sides' planes differ\n"
    if not failed:
        for s, src in LINES:
            text.append(f"== {s}, {src} depth ({vals['batch'][f'{s}:{src}:used'][-1]} used depth pixels a job)\n")
            for J in JS:
                b, l = np.array(vals["batch"][f"{s}:{src}:{J}"]), np.array(vals["looped"][f"{s}:{src}:{J}"])
                wins[(s, src, J)] = bool(b.max() < l.min())
                text.append(f"  J = {J:<3} batch " + "".join(f"{x:9.4f}" for x in b) + f"  median{np.median(b):9.4f}\n")
                text.append(f"  {'':<7} looped" + "".join(f"{x:9.4f}" for x in l) + f"  median{np.median(l):9.4f}   every batch value below every looped value: {wins[(s, src, J)]}\n")
        first = next((J for J in JS if all(wins[(s, src, G)] for s, src in LINES for G in JS if G >= J)), None)
        text.append(f"kAlignBatchMin by the rule (all four lines; every measured J from it on): {first if first else '1025 -- no such J up to 32: THE ROUTE LOST, the call loops by default'}\n")
        # ---- the rig frame: the record, no threshold
        rig = {"aligning": [], "hand": [], "aligned": []}
        dig = {}
        for k in range(o.rounds):
            for side, env in (("aligning", env_b), ("hand", env_s), ("aligned", env_b)):
                print(f"rig frame, round {k + 1}, {side} ...", flush=True)
                res, failed = run_child(me, "rig:" + side, env)
                if failed:
                    break
                rig[side].append(res["ms"]); dig.setdefault(side, set()).add(res["digest"]); pts = res["points"]
            if failed:
                break
        if not failed:
            text.append(f"== rig frame: K = 3 cameras at 640 x 480 -> 640 x 480, device depth and masks, a rope of 45 nodes at rest, {pts} cloud points; nodes and cloud after the same "
                        f"number of frames equal bit for bit on the three sides: {len(dig['aligning'] | dig['hand'] | dig['aligned']) == 1}\n")
            for side, what in (("aligning", "tdlo_tracker_frame_from_rig_aligning (this tree)"), ("hand", f"3 x tdlo_align_depth + tdlo_tracker_frame_from_rig by hand ({who})"),
                               ("aligned", "tdlo_tracker_frame_from_rig on planes aligned beforehand (this tree)")):
                v = np.array(rig[side])
                text.append(f"  {what}\n  {'':<9}" + "".join(f"{x:9.4f}" for x in v) + f"  median{np.median(v):9.4f}\n")
            text.append(f"  alignment adds {np.median(rig['aligning']) - np.median(rig['aligned']):.4f} ms to a rig frame through the aligning call, "
                        f"{np.median(rig['hand']) - np.median(rig['aligned']):.4f} ms by hand\n")
    if failed:
        text.append(failed)
    out = "".join(text)
    print(out)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(out)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
