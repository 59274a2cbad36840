"""What the colour read costs a frame: ms per steady-state frame of trackdlo.frame_from_colour (BGR + depth in, nodes out) or trackdlo.frame_from_depth
(mask given), at 640 x 480 and 1280 x 720, images in the context's pinned buffers and in pageable memory.  One JSON line.

  python scripts/gpu_colour_frame.py --kind colour                      # this tree
  python scripts/gpu_colour_frame.py --kind depth --root PARENT_TREE    # another build of the package (e.g. the parent commit's), for A/B pairs
  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/gpu_colour_frame.py --kind colour --frames 200 --shape 480x640 --pinned-only
                                                                        # kernels per frame: every kernel's Calls / (frames + 10 warm-up frames)
Both kinds run the same scene (synth.depth_scene(30, config=9, frame=3), bench.py's frame_from_depth scene); the colour image is synth.colour_scene's
for the launch file's range, so the segmentation is depth_scene's mask and the two kinds register the same cloud.
profiles/colour_frame_ab.txt holds the figures of five alternating pairs."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--kind", choices=("colour", "depth"), required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose trackdlo_amd package (and built library) is used")
ap.add_argument("--frames", type=int, default=2000)
ap.add_argument("--shape", default=None, help="ROWSxCOLS: that size only")
ap.add_argument("--pinned-only", action="store_true")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
from trackdlo_amd import binding as B, synth  # noqa: E402

P = synth.LAUNCH_PARAMS
M = 30
LOWER, UPPER = [[90, 90, 30]], [[130, 255, 255]]
ctx = B.Context(device=0, timing=False)
out = dict(kind=args.kind, library=os.path.join(args.root, "trackdlo_amd"), frames=args.frames)
shapes = [tuple(int(v) for v in args.shape.split("x"))] if args.shape else [(480, 640), (720, 1280)]
for shape in shapes:
    if args.kind == "colour":
        depth, colour, _, mask, cam, Y0 = synth.colour_scene(M, LOWER, UPPER, config=9, frame=3, rows=shape[0], cols=shape[1])
        params = B.make_colour_params(LOWER, UPPER)
        cpin, _ = ctx.colour_buffers(*shape)
        cpin[:] = colour
    else:
        depth, mask, cam, Y0 = synth.depth_scene(M, config=9, frame=3, rows=shape[0], cols=shape[1])
    a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    trk = B.trackdlo(M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"],
                     P["lle_weight"], ctx=ctx)
    trk.initialize_nodes(Y0); trk.initialize_geodesic_coord(synth.geodesic_coord(Y0))
    dpin, mpin = ctx.image_buffers(*shape)
    dpin[:] = depth; mpin[:] = mask
    res = dict(masked_pixels=int(np.count_nonzero(mask)))
    for tag in ("pinned",) if args.pinned_only else ("pinned", "pageable"):
        if args.kind == "colour":
            d_, c_ = (dpin, cpin) if tag == "pinned" else (depth, colour)
            frame = lambda: trk.frame_from_colour(d_, c_, params, None, *a, 0.008, 0.06)      # noqa: E731
        else:
            d_, m_ = (dpin, mpin) if tag == "pinned" else (depth, mask)
            frame = lambda: trk.frame_from_depth(d_, m_, *a, 0.008, 0.06)                     # noqa: E731
        for _ in range(10):
            frame()
        t0 = time.perf_counter()
        for _ in range(args.frames):
            frame()          # (returns with the frame's nodes on the host: every call ends in a hand-over from the device)
        res[f"ms_per_frame_{tag}"] = round((time.perf_counter() - t0) * 1e3 / args.frames, 4)
    res["iters"] = [s["iters"] for s in trk.last_stats]
    res["prepass_rides"] = ctx.cloud_vis_rides()
    if hasattr(ctx, "colour_route_counts"):
        res["colour_routes"] = ctx.colour_route_counts()
    out[f"{shape[1]}x{shape[0]}"] = res
ctx.close()
print(json.dumps(out))
