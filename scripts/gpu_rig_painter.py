"""What the self-occlusion test under a rig costs on the device against the host statement.  profiles/rig_painter_ab.txt is this script's output.

    python scripts/gpu_rig_painter.py [--rounds 5] [--reps 20] [--out profiles/rig_painter_ab.txt]

(a) tdlo_rig_self_occlusion_batch (one upload, one launch of k_rig_painter_batch, one wait) against F calls of tdlo_rig_self_occlusion_visible: every frame a
    self-crossing rope (the generator of tests/test_abi.py's self-occlusion test) under K = 3 cameras, F = 1, 2, 4, 8, 16, 32, at M = 45 and M = 300.  The
    sets and the per-camera words are compared on both sides before a line is printed: a difference ends the run.
(b) tdlo_tracker_frames_from_rig_batch for 32 trackers of 45 nodes under a rig of 3 cameras (trackdlo_amd.synth rope frames, 640 x 480), through one library:
    the switch on in a context made under TDLO_RIG_PAINTER_MIN=1 (the kernel), on in a context made under a value above every batch (the host statement), and off.
The ways alternate inside every round; a value is the mean of `reps` calls timed with the host clock (time.perf_counter) around calls that return with the
stream waited for; a line holds every round's value and their median, in ms.  The entry points are called through ctypes with arguments marshalled once.

The rule for kRigPainterMin (csrc/tdlo_api.cpp), set before the measurement: the smallest F K from which on -- at that F and every larger measured F -- the
kernel's value lies below the host statement's at both M; if there is none, a value above any batch, and the tracker calls run the host statement by default.
The last lines state what the rule gives on this run."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("TDLO_RIG_BATCH_MIN", "1")
os.environ.setdefault("TDLO_TRACKER_BATCH_MIN", "2")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, FS, NF, LEAF, D_VIS, WIDTH = 3, (1, 2, 4, 8, 16, 32), 32, 0.008, 0.06, 10
vp = C.c_void_p


def line(out, label, rounds):
    med = float(np.median(rounds))
    text = f"{label:<58s} " + " ".join(f"{v:8.4f}" for v in rounds) + f"   median {med:8.4f} ms"
    print(text, flush=True); out.append(text)
    return med


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def part_a(B, ctx, out, rounds, reps):
    import rig_painter_scenes as PS
    lib = ctx.lib
    wins = {}
    for M in (45, 300):
        rng = np.random.default_rng(100 + M)
        scenes = [PS.random_scene(rng, M, K, f"rope {f}") for f in range(NF)]
        W = (M + 31) // 32
        keep = []
        tab = (B.RigPainterFrameC * NF)()
        for f, s in enumerate(scenes):
            Y = np.asfortranarray(s.Y); ct, _ = B._painter_cams(s.cams); T = B._painter_matrices(s.mats, K); nd = np.ascontiguousarray(s.dist)
            keep += [Y, ct, T, nd]
            tab[f].Y = Y.ctypes.data; tab[f].M = M; tab[f].cams = C.cast(ct, vp).value; tab[f].rig_to_cam = None if T is None else T.ctypes.data
            tab[f].K = K; tab[f].dlo_pixel_width = s.w; tab[f].node_dist = nd.ctypes.data; tab[f].visibility_threshold = s.thr
        vis_k = np.zeros((NF, M), np.int32); nv_k = np.zeros(NF, np.int32); seen_k = np.zeros((NF, K, W), np.uint32); hid_k = np.zeros_like(seen_k)
        vis_h = np.zeros((NF, M), np.int32); nv_h = np.zeros(NF, np.int32); seen_h = np.zeros((NF, K, W), np.uint32); hid_h = np.zeros_like(seen_h)
        p = lambda a: a.ctypes.data_as(vp)
        nvp = [C.cast(nv_h.ctypes.data + 4 * f, C.POINTER(C.c_int)) for f in range(NF)]
        args_h = [(tab[f].Y, M, tab[f].cams, tab[f].rig_to_cam, K, PS.ROWS, PS.COLS, tab[f].dlo_pixel_width, tab[f].node_dist, tab[f].visibility_threshold,
                   vis_h[f].ctypes.data, nvp[f], seen_h[f].ctypes.data, hid_h[f].ctypes.data) for f in range(NF)]
        for F in FS:
            def kernel():
                rc = lib.tdlo_rig_self_occlusion_batch(ctx.h, F, C.cast(tab, vp), PS.ROWS, PS.COLS, p(vis_k), p(nv_k), p(seen_k), p(hid_k))
                assert rc == 0, rc

            def host():
                for f in range(F):
                    assert lib.tdlo_rig_self_occlusion_visible(*args_h[f]) == 0
            kernel(); host()
            same = np.array_equal(nv_k[:F], nv_h[:F]) and np.array_equal(seen_k[:F], seen_h[:F]) and np.array_equal(hid_k[:F], hid_h[:F]) and \
                all(np.array_equal(vis_k[f, :nv_k[f]], vis_h[f, :nv_h[f]]) for f in range(F))
            if not same:
                raise SystemExit(f"M = {M}, F = {F}: the kernel's sets or words differ from the host statement's")
            a, b = [], []
            for _ in range(rounds):
                a.append(timed(kernel, reps)); b.append(timed(host, reps))
            ka = line(out, f"(a) M = {M:3d} K = {K} F = {F:2d} ({F * K:2d} jobs)  kernel, one call", a)
            hb = line(out, f"(a) M = {M:3d} K = {K} F = {F:2d} ({F * K:2d} jobs)  host statement, F calls", b)
            wins[(M, F)] = max(a) < min(b)
        del keep
    return wins


def part_b(B, out, rounds, reps):
    import rig_scenes
    from trackdlo_amd import synth
    M = 45
    P = synth.LAUNCH_PARAMS
    targs = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    cams, mats = [], []
    for k in range(K):
        depth, mask, cam, _ = synth.depth_scene(M, config=31, frame=0)
        T = None if k == 0 else np.concatenate([np.eye(3), np.array([[0.0004 * k], [-0.0003 * k], [0.0002 * k]])], axis=1)
        cams.append(B.RigCamera(np.ascontiguousarray(depth), mask=np.ascontiguousarray(mask), cam=(cam["fx"], cam["fy"], cam["cx"], cam["cy"]), cam_to_rig=T))
        mats.append(None if T is None else np.concatenate([np.eye(3), -T[:, 3:]], axis=1))
    ways = {}
    for name, env, switch in (("switch on, kernel (TDLO_RIG_PAINTER_MIN=1)", "1", True), ("switch on, host statement (TDLO_RIG_PAINTER_MIN=2^20)", str(1 << 20), True),
                              ("switch off", "1", False)):
        os.environ["TDLO_RIG_PAINTER_MIN"] = env
        ctx = B.Context(device=0, max_frames=NF, max_points=1 << 15, max_nodes=64, timing=False)
        del os.environ["TDLO_RIG_PAINTER_MIN"]
        Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
        tr = []
        for i in range(NF):
            t = B.trackdlo(*targs, ctx=ctx, slot=i)
            t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
            if switch:
                t.set_rig_self_occlusion(mats, K, WIDTH)
            tr.append(t)
        ways[name] = (ctx, tr)
    rigs = [cams] * NF
    res = {name: [] for name in ways}
    sets = {}
    for name, (ctx, tr) in ways.items():
        sets[name] = B.frames_from_rig_batch(tr, rigs, LEAF, D_VIS)[1]
    on = [n for n in ways if n.startswith("switch on")]
    if not all(np.array_equal(a, b) for a, b in zip(sets[on[0]], sets[on[1]])):
        raise SystemExit("(b): the two routes give different visible sets")
    for _ in range(rounds):
        for name, (ctx, tr) in ways.items():
            res[name].append(timed(lambda: B.frames_from_rig_batch(tr, rigs, LEAF, D_VIS), max(reps // 4, 3)))
    for name in ways:
        line(out, f"(b) 32 trackers, K = {K}, 640 x 480: {name}", res[name])
    out.append(f"(b) counters 51 / 52: " + "; ".join(f"{name}: {ways[name][0].rig_painter_route_counts()}" for name in ways))
    print(out[-1], flush=True)
    for ctx, tr in ways.values():
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_painter_ab.txt"))
    a = ap.parse_args()
    from trackdlo_amd import binding as B
    out = [f"# scripts/gpu_rig_painter.py --rounds {a.rounds} --reps {a.reps}: host clock (time.perf_counter) around calls that end in a stream wait; ms per call;",
           "# the ways alternate inside every round; every line: the rounds' values and their median"]
    ctx = B.Context(device=0, max_frames=4, max_points=1 << 15, max_nodes=64, timing=False)
    wins = part_a(B, ctx, out, a.rounds, a.reps)
    ctx.close()
    part_b(B, out, a.rounds, a.reps)
    rule = None
    for F in FS:
        if all(wins[(M, G)] for M in (45, 300) for G in FS if G >= F):
            rule = F * K
            break
    out.append("# the rule: kRigPainterMin = " + (f"{rule} jobs (the kernel wins on every value from F = {rule // K} on at both M)" if rule else
                                                  "a value above any batch (no F from which the kernel wins on every value at both M): the host statement by default"))
    print(out[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
