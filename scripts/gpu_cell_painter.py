"""What the painter test over a cell of ropes costs on the device against the host statement, and what it adds to a frame of the shared-cloud tracker call.
profiles/cell_painter_ab.txt is this script's output.

    python scripts/gpu_cell_painter.py [--rounds 5] [--reps 20] [--out profiles/cell_painter_ab.txt]

(a) tdlo_cell_occlusion_batch (one upload, k_cell_project + k_cell_cover, one wait) against tdlo_cell_occlusion_visible on ONE cell: F = 2, 4, 8 and 32
    self-crossing ropes of 45 nodes (the generator of tests/rig_painter_scenes.py) and 16 ropes of 1024 nodes (the largest cell of
    tests/cell_painter_scenes.py), each under K = 1 and K = 3 cameras.  The sets and the per-camera words are compared on both sides before a line is printed:
    a difference ends the run.
(b) tdlo_tracker_frames_from_shared_cloud_occluded_batch for F = 2, 4, 8, 32 crossing ropes of 45 nodes and 750 F points (the scene of
    tests/test_cell_painter_gpu.py) at K = 1 and K = 3, through one library: in a context made under TDLO_CELL_PAINTER_MIN=0 (the kernels), in one made under
    a value above any cell (the host statement), and tdlo_tracker_frames_from_shared_cloud_batch (no test) at the same commit.  The two routes' sets and nodes
    are compared after every call of the first round.
The ways alternate inside every round; a value is the mean of `reps` calls timed with the host clock (time.perf_counter) around calls that return with the
stream waited for, after one call that is not timed; a line holds every round's value and their median, in ms.

The rule for kCellPainterMin (csrc/tdlo_api.cpp), set before the measurement: the smallest measured N K (flat nodes x cameras) at and above which the kernels
are faster on every measured line of (a) -- every round's value below every round's value of the host statement; if there is none, a value above any cell,
and the tracker call runs the host statement by default.  The last line states what the rule gives on this run."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("TDLO_TRACKER_BATCH_MIN", "2")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D_VIS, D_MAX, HUGE = 0.06, 0.02, 1 << 40
vp = C.c_void_p


def line(out, label, rounds):
    med = float(np.median(rounds))
    text = f"{label:<76s} " + " ".join(f"{v:10.4f}" for v in rounds) + f"   median {med:10.4f} ms"
    print(text, flush=True); out.append(text)
    return med


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def cells_of_part_a():
    import cell_painter_scenes as CS
    import rig_painter_scenes as PS
    out = []
    for K in (1, 3):
        for F in (2, 4, 8, 32):
            rng = np.random.default_rng(1000 + 10 * F + K)
            cams, mats = PS.random_rig(rng, K)
            out.append(CS.Cell(f"F = {F:2d} M =   45 K = {K}", [PS.rope(rng, 45) for _ in range(F)], cams, mats, w=10, dists=[rng.uniform(0, 0.016, 45) for _ in range(F)]))
        big = CS.scene_largest()
        shift = lambda k: np.array([[1.0, 0, 0, 0.01 * k], [0, 1.0, 0, -0.01 * k], [0, 0, 1.0, 0.0]])
        out.append(CS.Cell(f"F = 16 M = 1024 K = {K}", [r[0] for r in big.ropes], big.cams * K, None if K == 1 else [None] + [shift(k) for k in range(1, K)],
                           rows=big.rows, cols=big.cols, w=big.w))
    return out


def part_a(B, ctx, out, rounds, reps):
    lib = ctx.lib
    wins = {}
    for s in cells_of_part_a():
        rt, F, N, Ms, keep = B._cell_ropes(s.ropes)
        ct, K = B._painter_cams(s.cams); T = B._painter_matrices(s.mats, K)
        W, Mmax = (N + 31) // 32, max(Ms)
        cell = B.CellC(C.cast(rt, vp).value, F, C.cast(ct, vp).value, None if T is None else T.ctypes.data, K, s.w)
        vis_k = np.zeros((F, Mmax), np.int32); nv_k = np.zeros(F, np.int32); seen_k = np.zeros((K, W), np.uint32); hid_k = np.zeros_like(seen_k)
        vis_h = np.zeros((F, Mmax), np.int32); nv_h = np.zeros(F, np.int32); seen_h = np.zeros((K, W), np.uint32); hid_h = np.zeros_like(seen_h)
        rows_h = (vp * F)(*[vis_h[f].ctypes.data for f in range(F)])
        p = lambda a: a.ctypes.data_as(vp)

        def kernel():
            rc = lib.tdlo_cell_occlusion_batch(ctx.h, 1, C.cast(C.pointer(cell), vp), s.rows, s.cols, p(vis_k), p(nv_k), p(seen_k), p(hid_k))
            assert rc == 0, rc

        def host():
            rc = lib.tdlo_cell_occlusion_visible(C.cast(rt, vp), F, C.cast(ct, vp), None if T is None else T.ctypes.data, K, s.rows, s.cols, s.w, C.cast(rows_h, vp),
                                                 p(nv_h), p(seen_h), p(hid_h))
            assert rc == 0, rc
        kernel(); host()
        same = np.array_equal(nv_k, nv_h) and np.array_equal(seen_k, seen_h) and np.array_equal(hid_k, hid_h) and \
            all(np.array_equal(vis_k[f, :nv_k[f]], vis_h[f, :nv_h[f]]) for f in range(F))
        if not same:
            raise SystemExit(f"{s.name}: the kernels' sets or words differ from the host statement's")
        r = reps if N * K < 10000 else max(reps // 10, 2)
        a, b = [], []
        for _ in range(rounds):
            a.append(timed(kernel, r)); b.append(timed(host, r))
        hidden = int(sum(bin(int(v)).count("1") for v in hid_k.ravel()))
        line(out, f"(a) {s.name} (N K = {N * K:5d}, {hidden:4d} hidden bits)  kernels, one call", a)
        line(out, f"(a) {s.name} (N K = {N * K:5d}, {hidden:4d} hidden bits)  host statement", b)
        wins.setdefault(N * K, []).append(max(a) < min(b))
        del keep
    return wins


def part_b(B, out, rounds, reps):
    from test_cell_painter_gpu import crossing_cell, VIEW_CAM, VIEW_W
    from test_assign_gpu import shared_trackers
    import cell_painter_scenes as CS
    M = 45
    for K in (1, 3):
        cams = [VIEW_CAM] * K
        mats = None if K == 1 else [None] + [np.array([[1.0, 0, 0, 0.01 * k], [0, 1.0, 0, -0.01 * k], [0, 0, 1.0, 0.0]]) for k in range(1, K)]
        for F in (2, 4, 8, 32):
            Y0, coords, clouds = crossing_cell(F, M, frames=1)
            X = clouds[0]
            ways = {}
            for name, env in (("occluded, kernels (TDLO_CELL_PAINTER_MIN=0)", "0"), ("occluded, host statement", str(HUGE)), ("tdlo_tracker_frames_from_shared_cloud_batch", "0")):
                os.environ["TDLO_CELL_PAINTER_MIN"] = env
                ctx = B.Context(device=0, max_frames=F + 1, max_points=1 << 15, max_nodes=64, timing=False)
                del os.environ["TDLO_CELL_PAINTER_MIN"]
                ctx.set_cloud(F, X)
                ways[name] = (ctx, shared_trackers(ctx, Y0, coords, M))
            names = list(ways)

            def call(name):
                ctx, tr = ways[name]
                if name == names[2]:
                    return B.frames_from_shared_cloud_batch(tr, F, D_MAX, D_VIS, check=False)
                return B.frames_from_shared_cloud_occluded_batch(tr, F, D_MAX, D_VIS, cams, mats, 4096, 4096, VIEW_W, check=False)      # (an image that holds all 32 ropes)

            def check():
                a, b = call(names[0]), call(names[1])
                ta, tb = ways[names[0]][1], ways[names[1]][1]
                ok = a[0] == b[0] == [0] * F and all(np.array_equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2])) and \
                    all(np.array_equal(x.get_tracking_result().view(np.uint64), y.get_tracking_result().view(np.uint64)) and x.get_sigma2() == y.get_sigma2() for x, y in zip(ta, tb))
                if not ok:
                    raise SystemExit(f"(b) F = {F} K = {K}: the two routes differ")
                call(names[2])
            res = {name: [] for name in ways}
            r = max(reps // 4, 3)
            for rd in range(rounds):
                if rd == 0:
                    for _ in range(r + 1):
                        check()                                        # (the first round, untimed: every call of both routes compared)
                for name in names:
                    res[name].append(timed(lambda: call(name), r))
            for name in names:
                line(out, f"(b) F = {F:2d} M = 45 K = {K} ({750 * F:5d} points): {name}", res[name])
            out.append(f"(b) F = {F:2d} K = {K} counters 57 / 58: " + "; ".join(f"{ways[n][0].cell_painter_route_counts()}" for n in names))
            print(out[-1], flush=True)
            for ctx, tr in ways.values():
                ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_painter_ab.txt"))
    a = ap.parse_args()
    from trackdlo_amd import binding as B
    out = [f"# scripts/gpu_cell_painter.py --rounds {a.rounds} --reps {a.reps}: host clock (time.perf_counter) around calls that end in a stream wait; ms per call;",
           "# the ways alternate inside every round; every line: the rounds' values and their median"]
    ctx = B.Context(device=0, max_frames=2, max_points=1 << 12, max_nodes=64, timing=False)
    wins = part_a(B, ctx, out, a.rounds, a.reps)
    ctx.close()
    part_b(B, out, a.rounds, a.reps)
    rule = None
    for v in sorted(wins):
        if all(all(wins[u]) for u in wins if u >= v):
            rule = v
            break
    out.append("# the rule: kCellPainterMin = " + (f"{rule} flat nodes x cameras (the kernels win on every measured line of (a) with N K >= {rule})" if rule else
                                                   "a value above any cell (no N K at and above which the kernels win on every line): the host statement by default"))
    print(out[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
