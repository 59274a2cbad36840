"""What aligning depth to the colour camera costs (writes profiles/align_ab.txt).  Three shapes, depth -> colour: 640 x 480 -> 640 x 480, 848 x 480 -> 1280 x 720,
1280 x 720 -> 1280 x 720; a dense depth image as a sensor delivers it (a wall at 1.5 m with 10 % holes, a rope-like band at 0.8 m in front of it), a small
rotation and a 15 mm baseline between the cameras.
Line 1: tdlo_align_depth from a depth image in DEVICE memory (no copy out: the plane stays in the context) against the comparator -- TDLO_ALIGN=host on the same
        box from pageable host memory, i.e. tdlo_align_depth_host plus the upload of its plane.
Line 2: tdlo_align_depth from PAGEABLE HOST depth (packed by the host, one upload, the two launches) against the same comparator.
Line 3: tdlo_align_depth_host alone (the statement on one core, no upload): what a caller's CPU pass costs.
Line 4 (640 x 480 only): what tdlo_tracker_frame_view_aligning adds to tdlo_tracker_frame_view on a frame that is aligned already (device views, 45 nodes).
Every compared pair is checked bit-equal before it is timed.  Host clock around calls that end in a stream wait; medians of REPS calls after WARM, the two sides
of a pair alternating call by call.  Every shape, and the tracker line, runs in a child process of its own under a time limit; the first that fails ends the run and is named in the file."""
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(480, 640, 480, 640), (480, 848, 720, 1280), (720, 1280, 720, 1280)]
REPS, WARM = 30, 5


def scene(rows_d, cols_d, rows_c, cols_c):
    import align_ref as AR
    s = AR.scene_rope(rows_d, cols_d, rows_c, cols_c)
    rng = np.random.default_rng(5)
    wall = (1500 + rng.integers(0, 8, (rows_d, cols_d))).astype(np.uint16)
    wall[rng.random((rows_d, cols_d)) < 0.1] = 0
    s["D"] = np.where(s["D"] != 0, s["D"], wall)
    return s


def ctx_under(B, host):
    old = os.environ.pop("TDLO_ALIGN", None)
    if host:
        os.environ["TDLO_ALIGN"] = "host"
    try:
        return B.Context(device=0, timing=False)
    finally:
        os.environ.pop("TDLO_ALIGN", None)
        if old is not None:
            os.environ["TDLO_ALIGN"] = old


def timed(fn):
    t0 = time.perf_counter(); out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def pair_ms(fa, fb):
    ta, tb = [], []
    for k in range(WARM + REPS):
        _, da = timed(fa); _, db = timed(fb)
        if k >= WARM:
            ta.append(da); tb.append(db)
    return float(np.median(ta)), float(np.median(tb)), float(np.min(ta)), float(np.max(ta))


def one(i):
    from trackdlo_amd import binding as B
    import torch
    import align_ref as AR
    rows_d, cols_d, rows_c, cols_c = SHAPES[i]
    tag = f"{cols_d} x {rows_d} -> {cols_c} x {rows_c}"
    s = scene(rows_d, cols_d, rows_c, cols_c)
    D, p = s["D"], B.make_align_params(**s["p"])
    A, n = AR.align(D, s["p"])
    cd, ch = ctx_under(B, False), ctx_under(B, True)
    dev = B.image_view(torch.from_numpy(D.view(np.int16)).cuda(), format=B.IMG_U16C1)
    for c, src in ((cd, dev), (cd, D), (ch, D)):
        G, gn, _ = c.align_depth(src, p)
        assert np.array_equal(G, A) and gn == n, tag
    assert cd.align_route_counts() == [2, 0] and ch.align_route_counts() == [0, 1]
    H, hn = B.align_depth_host(D, p)
    assert np.array_equal(H, A) and hn == n
    head = f"{tag}  {n[0]} depth pixels, {n[1]} used"
    d, h, lo, hi = pair_ms(lambda: cd.align_depth(dev, p, out=None), lambda: ch.align_depth(D, p, out=None))
    print(f"line 1  {head}  device depth: tdlo_align_depth {d:.3f} ms (min {lo:.3f}, max {hi:.3f})   host statement + upload {h:.3f} ms   bit-equal", flush=True)
    d, h, lo, hi = pair_ms(lambda: cd.align_depth(D, p, out=None), lambda: ch.align_depth(D, p, out=None))
    print(f"line 2  {head}  pageable host depth: tdlo_align_depth {d:.3f} ms (min {lo:.3f}, max {hi:.3f})   host statement + upload {h:.3f} ms   bit-equal", flush=True)
    t = [timed(lambda: B.align_depth_host(D, p))[1] for _ in range(WARM + REPS)][WARM:]
    print(f"line 3  {head}  tdlo_align_depth_host alone {float(np.median(t)):.3f} ms", flush=True)
    cd.close(); ch.close()


def tracker_line():
    from trackdlo_amd import binding as B
    import torch
    import align_ref as AR
    import colour_ref
    tag = "640 x 480 -> 640 x 480"
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    M, rows, cols = 45, 480, 640
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    cp = B.make_colour_params(*colour_ref.LAUNCH_RANGE)
    depth, colour, _, _, cam, Y0 = synth.colour_scene(M, *colour_ref.LAUNCH_RANGE, config=9, frame=1, rows=rows, cols=cols)
    a = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    pd = AR.params(rows, cols, a[:2], a[2:], rows, cols, a[:2], a[2:], AR.transform(AR.rot("z", 0.05), (0.001, 0.0, 0.0)))
    p = B.make_align_params(**pd)
    A, _ = AR.align(depth, pd)
    ca, cb = B.Context(device=0, timing=False), B.Context(device=0, timing=False)
    ta, tb = B.trackdlo(*args, ctx=ca), B.trackdlo(*args, ctx=cb)
    for t in (ta, tb):
        t.initialize_nodes(Y0); t.initialize_geodesic_coord(synth.geodesic_coord(Y0))
    rgba = torch.from_numpy(np.concatenate([colour, np.full((rows, cols, 1), 255, np.uint8)], axis=2)).cuda()
    raw = B.image_view(torch.from_numpy(depth.view(np.int16)).cuda(), format=B.IMG_U16C1)
    aligned = B.image_view(torch.from_numpy(A.view(np.int16)).cuda(), format=B.IMG_U16C1)
    fa = B.aligning_frame_view(raw, B.image_view(rgba))
    fb = B.frame_view(aligned, B.image_view(rgba))
    got = ta.frame_view_aligning(fa, p, cp, 0.008, 0.06)
    want = tb.frame_view(fb, cp, *a, 0.008, 0.06)
    same = lambda: np.array_equal(np.ascontiguousarray(ta.get_tracking_result()).view(np.uint64), np.ascontiguousarray(tb.get_tracking_result()).view(np.uint64))
    assert list(got[0]) == list(want[0]) and got[2:4] == want[2:] and same()
    d, h, lo, hi = pair_ms(lambda: ta.frame_view_aligning(fa, p, cp, 0.008, 0.06), lambda: tb.frame_view(fb, cp, *a, 0.008, 0.06))
    assert same()
    print(f"line 4  {tag}  tracker frame, device views, {M} nodes, {got[2]} points: aligning call {d:.3f} ms (min {lo:.3f}, max {hi:.3f})   "
          f"tdlo_tracker_frame_view on the aligned frame {h:.3f} ms   aligning adds {d - h:.3f} ms   bit-equal", flush=True)
    ca.close(); cb.close()


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one(int(sys.argv[2])) if int(sys.argv[2]) < len(SHAPES) else tracker_line()
        return
    text = ""
    for i in range(len(SHAPES) + 1):                   # (the last child: the tracker line)
        with subprocess.Popen([sys.executable, os.path.abspath(__file__), "--one", str(i)], stdout=subprocess.PIPE, text=True) as child:
            timer = threading.Timer(240.0, child.kill)
            timer.start()
            for line in child.stdout:
                print(line, end="", flush=True)
                text += line
            rc = child.wait()
            timer.cancel()
        if rc:
            text += f"child {i} ended with status {rc}: the lines that follow it are NOT MEASURED\n"
            break
    open(os.path.join(ROOT, "profiles", "align_ab.txt"), "w").write(text)
    sys.exit(rc)


if __name__ == "__main__":
    main()
