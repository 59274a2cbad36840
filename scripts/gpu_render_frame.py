"""What the tracking-result image costs a frame: ms per steady-state frame of trackdlo.frame_from_colour alone (--mode frame; also runs on a tree that
has no render call, e.g. the parent commit's) or followed by trackdlo.render_result (--mode render), at 640 x 480 and 1280 x 720, images in the context's
pinned buffers (result image: the pinned result buffer) and in pageable memory.  One JSON line.

  python scripts/gpu_render_frame.py --mode render                           # this tree
  python scripts/gpu_render_frame.py --mode frame --root PARENT_TREE         # another build of the package, for A/B pairs
  TDLO_RENDER_INPLACE=0 python scripts/gpu_render_frame.py --mode render     # the comparator of the output route: device image + copy
  python scripts/gpu_render_frame.py --mode render --copy-ref                # adds the event-timed torch device-to-device copy of a rows x cols x 3 uint8 tensor
  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/gpu_render_frame.py --mode render --frames 200 --pinned-only
                                                                             # k_render alone: its row of the kernel statistics
  TDLO_RENDER_INPLACE=0 rocprofv3 ... -- python scripts/gpu_render_frame.py --mode render --frames 200 --pageable-only
                                                                             # the same with every operand in device memory: what compares with the copy
The scene is scripts/gpu_colour_frame.py's (synth.colour_scene(30, launch range, config=9, frame=3), bench.py's frame_from_depth scene) with a rectangular
occluder.  profiles/render_frame_ab.txt holds the figures of five alternating pairs."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("frame", "render"), required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose trackdlo_amd package (and built library) is used")
ap.add_argument("--frames", type=int, default=2000)
ap.add_argument("--shape", default=None, help="ROWSxCOLS: that size only")
ap.add_argument("--pinned-only", action="store_true")
ap.add_argument("--pageable-only", action="store_true", help="with TDLO_RENDER_INPLACE=0: k_render reads and writes device memory only")
ap.add_argument("--copy-ref", action="store_true")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
from trackdlo_amd import binding as B, synth  # noqa: E402

P = synth.LAUNCH_PARAMS
M = 30
LOWER, UPPER = [[90, 90, 30]], [[130, 255, 255]]
ctx = B.Context(device=0, timing=False)
out = dict(mode=args.mode, library=os.path.join(args.root, "trackdlo_amd"), frames=args.frames, inplace_env=os.environ.get("TDLO_RENDER_INPLACE"))
shapes = [tuple(int(v) for v in args.shape.split("x"))] if args.shape else [(480, 640), (720, 1280)]
for shape in shapes:
    rows, cols = shape
    depth, colour, occ, mask, cam, Y0 = synth.colour_scene(M, LOWER, UPPER, config=9, frame=3, rows=rows, cols=cols, occluder=(0, rows // 8, 0, cols // 8))
    params = B.make_colour_params(LOWER, UPPER)
    cpin, opin = ctx.colour_buffers(*shape)
    cpin[:] = colour; opin[:] = occ
    dpin, _ = ctx.image_buffers(*shape)
    dpin[:] = depth
    a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    trk = B.trackdlo(M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"],
                     P["lle_weight"], ctx=ctx)
    trk.initialize_nodes(Y0); trk.initialize_geodesic_coord(synth.geodesic_coord(Y0))
    res = dict(masked_pixels=int(np.count_nonzero(mask)))
    for tag in ("pinned",) if args.pinned_only else ("pageable",) if args.pageable_only else ("pinned", "pageable"):
        d_, c_, o_ = (dpin, cpin, opin) if tag == "pinned" else (depth, colour, occ)
        if args.mode == "render":
            img = ctx.result_image_buffer(*shape) if tag == "pinned" else np.zeros(shape + (3,), dtype=np.uint8)

            def frame():
                trk.frame_from_colour(d_, c_, params, o_, *a, 0.008, 0.06)
                trk.render_result(out=img)
        else:
            def frame():
                trk.frame_from_colour(d_, c_, params, o_, *a, 0.008, 0.06)
        for _ in range(10):
            frame()
        t0 = time.perf_counter()
        for _ in range(args.frames):
            frame()          # (returns with the frame's nodes -- and the image -- on the host)
        res[f"ms_per_frame_{tag}"] = round((time.perf_counter() - t0) * 1e3 / args.frames, 4)
    res["iters"] = [s["iters"] for s in trk.last_stats]
    if hasattr(ctx, "render_route_counts"):
        res["render_routes"] = ctx.render_route_counts()
    if args.copy_ref:
        import torch
        src = torch.zeros(shape + (3,), dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        for _ in range(20):
            dst.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            dst.copy_(src)
        e1.record(); torch.cuda.synchronize()
        res["torch_d2d_copy_us"] = round(e0.elapsed_time(e1) * 1e3 / 200, 3)
    out[f"{cols}x{rows}"] = res
ctx.close()
print(json.dumps(out))
