"""What taking a frame's images as they arrive costs, and what k_image_import reaches (profiles/image_view_ab.txt holds a run).

  python scripts/gpu_image_view.py --mode e2e
      One process, 640 x 480 and 1280 x 720 frames of synth.colour_scene, a tracker per alternative.  Host clock around calls that end synchronised,
      after warm-up; the alternatives alternate, five rounds, every value printed (ms per frame, mean of --calls frames):
        (a) trackdlo.frame_view from device tensors, packed BGR8 + U16
        (b) trackdlo.frame_view from device tensors, RGBA8 + F32 metres
        (c) trackdlo.frame_view from a pitched host source (BGR8 + U16 with spare bytes behind every row)
        (d) trackdlo.frame_from_colour from the context's pinned buffers (read in place)
        (e) trackdlo.frame_from_colour from pageable arrays (copied to the device)
  python scripts/gpu_image_view.py --mode ab --parent scripts/tmp/libtrackdlo_parent.so
      The existing calls, parent commit's library against this tree's: one child process per library and pair (TDLO_LIBRARY), alternating,
      --pairs pairs; every child prints ms per frame of frame_from_colour and frame_from_depth (pinned buffers) at both sizes.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o iv -- python scripts/gpu_image_view.py --mode kernel
      Per size and layout: --calls device-view frames (k_image_import in front of the cloud kernel) and as many device-to-device copies of the
      canonical bytes (5 per pixel: depth + colour), the latter also timed in the process by stream events.
  python scripts/gpu_image_view.py --mode summarize --trace DIR
      k_image_import's time per size and layout from the kernel trace, the algorithmic bytes (the bytes of the views' rows + the canonical bytes
      written) over it, and the ratio to the copy of the canonical bytes.
Any HIP error raises: the process exits non-zero."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((480, 640), (720, 1280))
M = 30

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("e2e", "ab", "ab-child", "kernel", "summarize"), required=True)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "tmp", "libtrackdlo_parent.so"), help="ab: the parent commit's library")
ap.add_argument("--trace", default=None, help="summarize: the directory rocprofv3 wrote")
ap.add_argument("--manifest", default=os.path.join(ROOT, "scripts", "tmp", "image_view_kernel_manifest.json"), help="kernel mode writes, summarize reads")
args = ap.parse_args()


def ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def scene(rows, cols):
    from trackdlo_amd import binding as B, synth
    depth, colour, occ, mask, cam, Y0 = synth.colour_scene(M, *B.COLOUR_LAUNCH, config=9, frame=1, rows=rows, cols=cols, occluder=(rows // 3, rows // 2, cols // 3, cols // 3 + 12))
    return depth, colour, occ, mask, (cam["fx"], cam["fy"], cam["cx"], cam["cy"]), Y0


def tracker(B, synth, Y0):
    P = synth.LAUNCH_PARAMS
    ctx = B.Context(device=0, timing=False)
    t = B.trackdlo(M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 50, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"],
                   P["lle_weight"], ctx=ctx)
    t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
    return ctx, t


def table(title, alts, calls):
    for _, fn in alts:
        ms(fn, 5)
    rows = {name: [] for name, _ in alts}
    for _ in range(args.rounds):
        for name, fn in alts:
            rows[name].append(ms(fn, calls))
    print(title)
    for name, _ in alts:
        v = rows[name]
        print(f"  {name:52s} " + " ".join(f"{x:8.4f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:8.4f}  spread {min(v):.4f} .. {max(v):.4f}")
    sys.stdout.flush()


def device_views(B, torch, np, depth, colour, occ, layout):
    """(FrameView, owners) of the frame in device memory: 'packed' BGR8 + U16 as the camera driver delivers them, 'rgba-f32' RGBA8 + float metres
    with 64 spare bytes behind every row, as a renderer delivers them."""
    rows, cols = depth.shape
    if layout == "packed":
        d = B.image_view(torch.from_numpy(depth.view(np.int16)).cuda(), format=B.IMG_U16C1)
        return B.frame_view(d, torch.from_numpy(colour).cuda(), torch.from_numpy(occ).cuda())
    rgba = np.full((rows, cols + 16, 4), 255, dtype=np.uint8); rgba[:, :cols, :3] = colour
    met = np.zeros((rows, cols + 16), dtype=np.float32); met[:, :cols] = (depth / 1000.0).astype(np.float32)
    return B.frame_view(torch.from_numpy(met).cuda()[:, :cols], torch.from_numpy(rgba).cuda()[:, :cols], torch.from_numpy(occ).cuda())


def e2e():
    import numpy as np
    import torch
    from trackdlo_amd import binding as B, synth
    params = B.make_colour_params()
    for rows, cols in SHAPES:
        depth, colour, occ, _, a, Y0 = scene(rows, cols)
        made = [tracker(B, synth, Y0) for _ in range(5)]
        (ca, ta), (cb, tb), (cc, tc), (cd, td), (ce, te) = made
        fa = device_views(B, torch, np, depth, colour, occ, "packed")
        fb = device_views(B, torch, np, depth, colour, occ, "rgba-f32")
        hc = np.zeros((rows, cols * 3 + 64), dtype=np.uint8); hc[:, :cols * 3] = colour.reshape(rows, -1)
        hd = np.zeros((rows, cols + 32), dtype=np.uint16); hd[:, :cols] = depth
        vc = B.ImageView(hc.ctypes.data, B.IMG_U8C3, B.MEM_HOST, hc.strides[0], None); vc.rows, vc.cols, vc.owner = rows, cols, hc
        fc = B.frame_view(B.image_view(hd[:, :cols]), vc, occ)
        pd, _ = cd.image_buffers(rows, cols); pc, po = cd.colour_buffers(rows, cols)
        pd[:] = depth; pc[:] = colour; po[:] = occ
        alts = [("a frame_view, device tensors, BGR8 + U16 packed", lambda: ta.frame_view(fa, params, *a)),
                ("b frame_view, device tensors, RGBA8 + F32 pitched", lambda: tb.frame_view(fb, params, *a)),
                ("c frame_view, host, pitched BGR8 + U16", lambda: tc.frame_view(fc, params, *a)),
                ("d frame_from_colour, pinned buffers", lambda: td.frame_from_colour(pd, pc, params, po, *a)),
                ("e frame_from_colour, pageable arrays", lambda: te.frame_from_colour(depth, colour, params, occ, *a))]
        table(f"{cols} x {rows}  (ms per frame, mean of {args.calls} frames; {args.rounds} alternating rounds)", alts, args.calls)
        Y = [t.get_tracking_result() for _, t in made]
        assert all(np.array_equal(Y[0].view(np.uint64), y.view(np.uint64)) for y in Y[1:]), "the five routes' nodes differ"
        print(f"  (the five trackers' nodes are equal bit for bit after {5 + args.rounds * args.calls} frames each; routes of a: {ca.colour_route_counts()})")
        for c, _ in made:
            c.close()


def ab_child():
    import numpy as np
    from trackdlo_amd import binding as B, synth
    params = B.make_colour_params()
    out = {}
    for rows, cols in SHAPES:
        depth, colour, occ, mask, a, Y0 = scene(rows, cols)
        (cc, tc), (cm, tm) = tracker(B, synth, Y0), tracker(B, synth, Y0)
        pd, _ = cc.image_buffers(rows, cols); pc, po = cc.colour_buffers(rows, cols)
        pd[:] = depth; pc[:] = colour; po[:] = occ
        md, mm = cm.image_buffers(rows, cols)
        md[:] = depth; mm[:] = mask
        fc = lambda: tc.frame_from_colour(pd, pc, params, po, *a)
        fd = lambda: tm.frame_from_depth(md, mm, *a)
        ms(fc, 10); ms(fd, 10)
        out[f"{cols}x{rows}"] = dict(colour=ms(fc, args.calls), depth=ms(fd, args.calls), nodes=tc.get_tracking_result().view(np.uint64).sum().item())
        cc.close(); cm.close()
    print("AB " + json.dumps(out))


def ab():
    res = {"parent": [], "tree": []}
    for pair in range(args.pairs):
        for which, lib in (("parent", args.parent), ("tree", os.path.join(ROOT, "trackdlo_amd", "libtrackdlo_hip.so"))):
            env = dict(os.environ, TDLO_LIBRARY=lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "ab-child", "--calls", str(args.calls)], env=env, capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                print(r.stdout + r.stderr)
                sys.exit(r.returncode or 1)                  # (nothing more is started behind a child that failed)
            res[which].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("AB ")][-1][3:]))
    print(f"existing calls, pinned buffers, ms per frame (mean of {args.calls} frames after warm-up), {args.pairs} alternating pairs of processes")
    for shape in res["tree"][0]:
        for call in ("colour", "depth"):
            for which in ("parent", "tree"):
                v = [x[shape][call] for x in res[which]]
                print(f"  {shape:9s} frame_from_{call:6s} {which:6s} " + " ".join(f"{x:8.4f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:8.4f}  spread {min(v):.4f} .. {max(v):.4f}")
        assert len({x[shape]["nodes"] for w in res for x in res[w]}) == 1, "parent and tree give different nodes"
    print("  (parent's and tree's nodes after the timed frames are equal bit for bit)")


def kernel():
    import numpy as np
    import torch
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, timing=False)
    nothing = B.make_colour_params([[10, 10, 10]], [[5, 5, 5]])          # no pixel passes: the cloud kernel behind the import has an empty frame
    out = []
    for rows, cols in SHAPES:
        depth, colour, occ, _, a, _ = scene(rows, cols)
        P = rows * cols
        src = torch.zeros(5 * P, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        for layout, read in (("packed", 5), ("rgba-f32", 8)):
            full = device_views(B, torch, np, depth, colour, occ, layout)
            fv = B.frame_view(full.owners[0], full.owners[1])               # depth + colour: the canonical bytes are 5 per pixel
            rounds = []
            for r in range(args.rounds + 1):                                # (round 0 is the warm-up; the trace holds it too: summarize drops it)
                for _ in range(args.calls):
                    ctx.frame_to_cloud_view(0, fv, nothing, *a, 0.008, fetch=False)
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                for _ in range(args.calls):
                    dst.copy_(src, non_blocking=True)
                e[1].record()
                torch.cuda.synchronize()
                if r:
                    rounds.append(e[0].elapsed_time(e[1]) * 1e3 / args.calls)
            print(f"{cols} x {rows} {layout}: device-to-device copy of the canonical {5 * P} bytes, stream events, us per copy back to back: " + " ".join(f"{x:.2f}" for x in rounds))
            out.append(dict(rows=rows, cols=cols, layout=layout, calls=args.calls, rounds=args.rounds + 1, bytes=(read + 5) * P, canonical=5 * P))
    ctx.close()
    os.makedirs(os.path.dirname(args.manifest), exist_ok=True)
    with open(args.manifest, "w") as f:
        json.dump(out, f)


def column(row, *parts):
    for k in row:
        if all(p in k.lower() for p in parts):
            return k
    raise KeyError(parts)


def summarize():
    manifest = json.load(open(args.manifest))
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {args.trace}"
    rows = list(csv.DictReader(open(files[0])))
    ks, ke, kn = column(rows[0], "start"), column(rows[0], "end"), column(rows[0], "kernel", "name")
    rows.sort(key=lambda r: int(r[ks]))
    kern = [(int(r[ke]) - int(r[ks])) * 1e-3 for r in rows if "k_image_import" in r[kn]]
    copies = [(int(r[ke]) - int(r[ks])) * 1e-3 for r in rows if "rocclr_copyBuffer" in r[kn]]
    per = [m["calls"] * m["rounds"] for m in manifest]
    assert len(kern) == sum(per), (len(kern), per)
    have_copies = len(copies) == sum(per)
    if not have_copies:
        print(f"(the trace holds {len(copies)} dispatches of the runtime's copy kernel, not {sum(per)}: the copy's kernel times are not measured)")
    at = 0
    for m, n in zip(manifest, per):
        calls = m["calls"]
        k = kern[at + calls:at + n]; c = copies[at + calls:at + n] if have_copies else []
        at += n
        med_of = lambda v: [sorted(v[r * calls:(r + 1) * calls])[calls // 2] for r in range(m["rounds"] - 1)]
        meds = med_of(k); med = sorted(meds)[len(meds) // 2]
        print(f"{m['cols']} x {m['rows']} {m['layout']}: k_image_import, us per dispatch by round (median of {calls}): " + " ".join(f"{x:.2f}" for x in meds))
        print(f"    median {med:.2f} us -> {m['bytes'] / (med * 1e-6) / 1e12:.3f} TB/s over the algorithmic {m['bytes']} bytes (rows read + canonical bytes written)")
        if c:
            cm = med_of(c); cmed = sorted(cm)[len(cm) // 2]
            print(f"    device-to-device copy of the canonical {m['canonical']} bytes, us by round: " + " ".join(f"{x:.2f}" for x in cm) +
                  f"   median {cmed:.2f} us; import / copy = {med / cmed:.2f}")


{"e2e": e2e, "ab": ab, "ab-child": ab_child, "kernel": kernel, "summarize": summarize}[args.mode]()
