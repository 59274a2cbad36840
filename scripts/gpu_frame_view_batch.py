"""What the clouds of F slots cost from image VIEWS in one call against F single view calls (profiles/frame_view_batch_ab.txt is this script's output).

    python scripts/gpu_frame_view_batch.py --parent-lib PATH/libtrackdlo_hip.so [--rounds 5] [--reps 20] [--out profiles/frame_view_batch_ab.txt]

trackdlo_amd.synth rope frames (depth + colour image, 45 nodes, the launch file's colour range) at 640 x 480 and 1280 x 720; F = 1, 2, 4, 8, 16, 32 images, each
a buffer of its own (eight distinct scenes, repeated).  Lines:
   rgba      device RGBA8 + 32FC1 views, [K, H, W, 4] uint8 and [K, H, W] float32 tensors (pitch a multiple of 16: one 16-byte load per four pixels)
   bgr       device bgr8 + 16UC1 views
   host      host bgr8 + 16UC1 views (pageable numpy arrays)
   shared    one rgba image shared by F frames under F colour ranges
   trackers  tdlo_tracker_frame_views_batch against F x tdlo_tracker_frame_view, rgba views, the trackers at rest on their ropes
The method of profiles/init_batch_ab.txt: one child process per side and round, the sides alternating, `rounds` rounds; a child makes one context of 32 slots,
calls every shape twice before it is timed, then times `reps` calls with the host clock -- every call returns with the stream waited for -- and reports their
mean; it also reports a digest of the 32 slots' clouds (uint64 views) after the F = 32 call of every line, and the two sides' digests are compared here.
   batch   this tree's library under TDLO_FRAME_VIEW_BATCH_MIN=1: the batch launches at every F, F = 1 included
   single  F x tdlo_frame_to_cloud_view / tdlo_tracker_frame_view through the PARENT commit's library (--parent-lib, handed to the child through
           TDLO_LIBRARY); without --parent-lib this tree's library stands in, and the output says so
The rule for the library's crossovers (csrc/tdlo_api.cpp), set beforehand: kFrameViewBatchMin is the smallest F from which on every batch value lies below
every single-calls value on the lines rgba, bgr, host and shared, at both sizes; kFrameViewBatchTrackerMin the same on the line trackers; 33 where no F up
to 32 does.  Nothing here is a test gate.  This process touches no GPU itself: it writes the frames to a scratch file once, starts the children one after
the other, each under a time limit of its own, and stops at the first that fails."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, FS, LEAF, D_VIS, NF, SCENES = 45, (1, 2, 4, 8, 16, 32), 0.008, 0.06, 32, 8
SIZES = {"640x480": (480, 640, 400000), "1280x720": (720, 1280, 600000)}      # (rows, cols, surface samples), as scripts/gpu_cloud_batch.py
RANGE = ([[90, 90, 30]], [[130, 255, 255]])
LINES = ("rgba", "bgr", "host", "shared", "trackers")
CLOUD_LINES = ("rgba", "bgr", "host", "shared")
vp = C.c_void_p


def write_frames(size, path):
    from trackdlo_amd import synth
    rows, cols, samples = SIZES[size]
    d, c, cams = [], [], []
    for i in range(SCENES):
        depth, colour, _, mask, cam, _ = synth.colour_scene(M, *RANGE, config=31, frame=i, rows=rows, cols=cols, samples=samples)
        d.append(depth); c.append(colour); cams.append((cam["fx"], cam["fy"], cam["cx"], cam["cy"]))
    np.savez(path, depth=np.stack(d), colour=np.stack(c), cam=np.array(cams))


def child(side, size, reps, frames_path):
    import torch
    from trackdlo_amd import binding as B, synth
    rows, cols, _ = SIZES[size]
    z = np.load(frames_path)
    pick = [i % SCENES for i in range(NF)]
    depth, colour, cams = z["depth"][pick], z["colour"][pick], [tuple(z["cam"][i]) for i in pick]
    ctx = B.Context(device=0, max_frames=NF, max_points=1 << 15, max_nodes=64, timing=False)
    lib = ctx.lib
    rgba = np.full((NF, rows, cols, 4), 255, np.uint8); rgba[..., :3] = colour
    t_rgba = torch.from_numpy(rgba).cuda(); t_f32 = torch.from_numpy((depth / 1000.0).astype(np.float32)).cuda()
    t_bgr = torch.from_numpy(colour).cuda(); t_u16 = torch.from_numpy(depth.view(np.int16).copy()).cuda()
    h_bgr = [np.ascontiguousarray(colour[i]) for i in range(NF)]; h_u16 = [np.ascontiguousarray(depth[i]) for i in range(NF)]
    torch.cuda.synchronize()
    images = dict(rgba=[dict(depth=t_f32[i], colour=t_rgba[i], cam=cams[i]) for i in range(NF)],
                  bgr=[dict(depth=B.image_view(t_u16[i], format=B.IMG_U16C1), colour=t_bgr[i], cam=cams[i]) for i in range(NF)],
                  host=[dict(depth=h_u16[i], colour=h_bgr[i], cam=cams[i]) for i in range(NF)])
    images["shared"] = images["rgba"][:1]
    images["trackers"] = images["rgba"]
    tabs = {k: B._view_images(v) for k, v in images.items()}
    launch = B.make_colour_params(*RANGE)
    # F ranges for the shared image, each inside the launch file's (a wider one would take in background colours one unit beside its bounds)
    inner = [B.make_colour_params([[90 + i % 8, 90 + i // 8, 30]], [[130 - i % 8, 255, 255]]) for i in range(NF)]
    params = {k: [inner[i] if k == "shared" else launch for i in range(NF)] for k in LINES}
    frames = {}
    for k in LINES:
        fr = (B.BatchFrame * NF)()
        for i in range(NF):
            fr[i].slot, fr[i].image, fr[i].colour_params = i, 0 if k == "shared" else i, C.addressof(params[k][i])
        frames[k] = fr
    n = np.zeros(NF, np.int32); nraw = np.zeros(NF, np.int32); rcs = np.zeros(NF, np.int32)
    n1 = C.c_int(0); nraw1 = C.c_int(0)
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], P["max_iter"], P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
    trk = []
    for i in range(NF):
        t = B.trackdlo(*args, ctx=ctx, slot=i)
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
        trk.append(t)
    ttab = (vp * NF)(*[t.h for t in trk])
    image_of = np.arange(NF, dtype=np.int32)
    cps = (vp * NF)(*[C.addressof(launch)] * NF)
    vis = np.zeros((NF, M), np.int32); ext = np.zeros((NF, M), np.int32); nv = np.zeros(NF, np.int32); ne = np.zeros(NF, np.int32)
    st = (B.Stats * (2 * NF))()
    nv1 = C.c_int(0); ne1 = C.c_int(0)

    def chk(rc):
        if rc:
            ctx._chk(rc)

    def batch(line, F):
        tab, K, r, c, _ = tabs[line]
        if line == "trackers":
            return chk(lib.tdlo_tracker_frame_views_batch(C.cast(ttab, vp), F, C.cast(tab, vp), K, r, c, image_of.ctypes.data, C.cast(cps, vp), LEAF, D_VIS, vis.ctypes.data,
                                                          nv.ctypes.data, ext.ctypes.data, ne.ctypes.data, n.ctypes.data, nraw.ctypes.data, C.cast(st, vp), rcs.ctypes.data))
        chk(lib.tdlo_frame_views_to_cloud_batch(ctx.h, C.cast(tab, vp), min(K, F), r, c, C.cast(frames[line], vp), F, LEAF, n.ctypes.data, nraw.ctypes.data, rcs.ctypes.data))

    def single(line, F):
        tab, K, r, c, _ = tabs[line]
        for i in range(F):
            im = tab[0 if line == "shared" else i]
            if line == "trackers":
                chk(lib.tdlo_tracker_frame_view(trk[i].h, C.byref(im.fv), C.byref(launch), r, c, im.fx, im.fy, im.cx, im.cy, LEAF, D_VIS, vis[i].ctypes.data, C.byref(nv1),
                                                ext[i].ctypes.data, C.byref(ne1), C.byref(n1), C.byref(nraw1), C.cast(st, vp)))
            else:
                chk(lib.tdlo_frame_to_cloud_view(ctx.h, i, C.byref(im.fv), C.byref(params[line][i]), r, c, im.fx, im.fy, im.cx, im.cy, LEAF, None, 0, C.byref(n1), C.byref(nraw1)))

    fn = batch if side == "batch" else single
    for _ in range(30):          # the trackers onto their ropes: from here on both registrations stop early
        fn("trackers", NF)
    out = {}
    for F in FS:
        for line in LINES:
            fn(line, F); fn(line, F)          # every shape before it is timed
            t0 = time.perf_counter()
            for _ in range(reps):
                fn(line, F)
            out[f"{line}:{F}"] = (time.perf_counter() - t0) / reps * 1e3
            if F == NF:
                if side == "batch":          # what one call of 32 frames adds to the counters 42 / 43 / 44
                    r0 = ctx.frame_view_batch_route_counts(); fn(line, F); r1 = ctx.frame_view_batch_route_counts()
                    out[f"{line}:routes"] = [b - a for a, b in zip(r0, r1)]
                h = hashlib.sha1()
                for s in range(NF):
                    h.update(np.ascontiguousarray(ctx.get_cloud(s)).view(np.uint64).tobytes())
                out[f"{line}:digest"] = h.hexdigest()
                if line == "rgba":
                    tot = sum(ctx.get_cloud(s).shape[0] for s in range(NF))
                    out["points"] = tot
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_view_batch_ab.txt"))
    ap.add_argument("--child", nargs=3, default=None, metavar=("SIDE", "SIZE", "FRAMES"))
    o = ap.parse_args()
    if o.child:
        return child(o.child[0], o.child[1], o.reps, o.child[2])
    assert o.rounds >= 5 and o.reps >= 20, "at least 5 rounds of at least 20 calls"
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(o.reps)]
    env_b = dict(os.environ, TDLO_FRAME_VIEW_BATCH_MIN="1")
    env_b.pop("TDLO_LIBRARY", None)
    env_s = dict(os.environ)
    if o.parent_lib:
        env_s["TDLO_LIBRARY"] = os.path.abspath(o.parent_lib)
    text = ["Image views for F slots in one call (tdlo_frame_views_to_cloud_batch / tdlo_tracker_frame_views_batch, TDLO_FRAME_VIEW_BATCH_MIN=1) against F single view calls "
            "(tdlo_frame_to_cloud_view / tdlo_tracker_frame_view) through "
            + ("the PARENT commit's library" if o.parent_lib else "the SAME library (no --parent-lib was given)") + ".\n"
            f"scripts/gpu_frame_view_batch.py: one child process per side and round, alternating, {o.rounds} rounds; ms per call, mean of {o.reps} calls after two warm-up calls;\n"
            "host clock around calls that return with the stream waited for.  Nothing here is a gate.\n"]
    failed = None
    wins = {}
    with tempfile.TemporaryDirectory() as tmp:
        for size in SIZES:
            rows, cols, _ = SIZES[size]
            P = rows * cols
            path = os.path.join(tmp, size + ".npz")
            write_frames(size, path)
            vals = {"batch": {}, "single": {}}
            for k in range(o.rounds):
                for side, env in (("batch", env_b), ("single", env_s)):
                    print(f"{size}, round {k + 1}, {side} ...", flush=True)
                    try:
                        r = subprocess.run(me + ["--child", side, size, path], env=env, capture_output=True, text=True, timeout=240)
                    except subprocess.TimeoutExpired:
                        failed = f"{size}, round {k + 1}, {side}: ran into its time limit; nothing further was started\n"
                        break
                    res = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                    if r.returncode != 0 or not res:
                        failed = f"{size}, round {k + 1}, {side}: ended with {r.returncode}; nothing further was started\n{r.stderr[-3000:]}\n"
                        break
                    for key, v in json.loads(res[0][7:]).items():
                        vals[side].setdefault(key, []).append(v)
                if failed:
                    break
            if failed:
                break
            same = {l: set(vals["batch"][f"{l}:digest"]) == set(vals["single"][f"{l}:digest"]) and len(set(vals["batch"][f"{l}:digest"])) == 1 for l in LINES}
            text.append(f"== {size}: {NF} rope frames ({SCENES} scenes), {vals['batch']['points'][-1]} cloud points in 32 slots, leaf {LEAF}; what a call of 32 frames adds to the counters 42 / 43 / 44 "
                        "(served / passed on / planes imported), per line: " + ", ".join(f"{l} {vals['batch'][f'{l}:routes'][-1]}" for l in LINES) + f"\n   the 32 slots' clouds of the two sides equal bit for bit after the F = 32 call, per line: {same}\n"
                        f"   the import launch's bytes per call (rgba: {P} pixels x (4 + 4 read, 3 + 2 written) per image; bgr: x (3 + 2 read, 3 + 2 written)): "
                        + ", ".join(f"F = {F}: {F * P * 13 / 1e6:.1f} / {F * P * 10 / 1e6:.1f} MB" for F in FS) + "; shared: one image's at every F; host: none (one copy)\n")
            if not all(same.values()):
                failed = f"{size}: the two sides' clouds differ\n"
                break
            for F in FS:
                text.append(f" F = {F}\n")
                for l in LINES:
                    b, s = np.array(vals["batch"][f"{l}:{F}"]), np.array(vals["single"][f"{l}:{F}"])
                    wins[(size, l, F)] = bool(b.max() < s.min())
                    text.append(f"  {l:<9} batch " + "".join(f"{x:9.4f}" for x in b) + f"  median{np.median(b):9.4f}\n")
                    text.append(f"  {'':<9} single" + "".join(f"{x:9.4f}" for x in s) + f"  median{np.median(s):9.4f}   every batch value below every single value: {wins[(size, l, F)]}\n")
    if failed:
        text.append(failed)
    else:
        def first(lines):
            return next((F for F in FS if all(wins[(sz, l, G)] for sz in SIZES for l in lines for G in FS if G >= F)), None)
        a, t = first(CLOUD_LINES), first(("trackers",))
        text.append(f"kFrameViewBatchMin by the rule (lines {', '.join(CLOUD_LINES)}; both sizes; every measured F from it on): {a if a else '33 -- no such F up to 32: off by default'}\n")
        text.append(f"kFrameViewBatchTrackerMin by the rule (line trackers): {t if t else '33 -- no such F up to 32: off by default'}\n")
    out = "".join(text)
    print(out)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(out)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
