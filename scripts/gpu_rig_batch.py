"""What the rigs of F slots cost in one call against F single calls.  profiles/rig_batch_ab.txt is this script's output.

    python scripts/gpu_rig_batch.py [--rounds 5] [--reps 10] [--out profiles/rig_batch_ab.txt] [--trace SIZE]

trackdlo_amd.synth rope frames (45 nodes) under K = 3 cameras -- each with images of its own and, but the first, a rotation and a translation to the common
frame -- at 640 x 480 and 1280 x 720; F = 1, 2, 4, 8, 16, 32.  One context of 64 slots: slots 0 .. 31 are filled by the batch calls, slots 32 .. 63 by the
single calls, whose code this change does not touch.  The two ways alternate inside every round; every value is the mean of `reps` calls, timed with the host
clock (time.perf_counter) around calls that return with the stream waited for; a line holds every round's value and their median, in ms.  The entry points are
called through ctypes with arguments marshalled once.  The process runs under TDLO_RIG_BATCH_MIN=1 and TDLO_TRACKER_BATCH_MIN=2 (unless the variables are set),
so that the batch launches are on record at every F.  Every line is printed only after the clouds of the batch slots and of the single slots have been
compared on bits (uint64 views): a difference ends the run.

   (a) shared-dev   F ropes under ONE rig: the K depth planes are shared, every frame brings K mask planes of its own; device planes
   (b) shared-host  the same from pageable host planes
   (c) own-dev      F rigs with planes of their own (3 F depth planes, 3 F mask planes); device planes
   (d) trackers     tdlo_tracker_frames_from_rig_batch against F x tdlo_tracker_frame_from_rig, the rigs of (a)

The rule for the library's constants (csrc/tdlo_api.cpp), set before the measurement: kRigBatchMin is the smallest F from which on -- at that F and every
larger measured F -- every batch value lies below every single-calls value on the lines (a) to (c) at both sizes; none up to 32: 33, the calls loop over the
single calls.  kRigBatchTrackerMin is the same rule over line (d).  The last lines of the output state what the rule gives on this run.

--trace SIZE (640x480 | 1280x720): instead of the lines, ten calls of F = 32 of (a) at that size, to be run under `rocprofv3 --kernel-trace --stats
--output-format csv -d DIR -- python scripts/gpu_rig_batch.py --trace SIZE` in a run of its own (the kernel alone: k_cloud_rig_batch in DIR's kernel_stats
file; profiles/rig_batch_kernel_stats.csv holds those rows of both sizes)."""
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

M, K, FS, LEAF, D_VIS, NF = 45, 3, (1, 2, 4, 8, 16, 32), 0.008, 0.06, 32
SIZES = {"640x480": (480, 640, 400000), "1280x720": (720, 1280, 600000)}      # (rows, cols, surface samples), as scripts/gpu_rig.py
vp = C.c_void_p


class Bench:
    def __init__(self, size):
        import torch
        import rig_scenes
        from trackdlo_amd import binding as B, synth
        self.B, self.torch = B, torch
        rows, cols, samples = SIZES[size]
        self.rows, self.cols = rows, cols
        self.ctx = ctx = B.Context(device=0, max_frames=2 * NF, max_points=1 << 15, max_nodes=64, timing=False)
        self.lib = ctx.lib
        base = []
        for k in range(K):
            depth, mask, cam, _ = synth.depth_scene(M, config=31, frame=k, rows=rows, cols=cols, samples=samples)
            T = None if k == 0 else rig_scenes.about(rig_scenes.rotation(0.02 * k, (0.2, 1.0, 0.1)), (0.0, 0.0, 0.7), (0.001 * k, 0.0, 0.0005 * k))
            base.append((np.ascontiguousarray(depth), np.ascontiguousarray(mask), (cam["fx"], cam["fy"], cam["cx"], cam["cy"]), T))
        self.kept = sum(int(np.count_nonzero(b[1])) for b in base)
        dev = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
        self.keep = []

        def rigs(shared_depth, place):
            """NF rigs: the depth planes shared or copied per frame, the mask planes copied per frame (frame f's with a few of its pixels cleared)."""
            depths = [place(b[0]) for b in base]
            out = []
            for f in range(NF):
                cams = []
                for k, (d, m, cam, T) in enumerate(base):
                    mk = m.copy(); mk.reshape(-1)[f::97] = 0
                    cams.append(B.RigCamera(depths[k] if shared_depth else place(d.copy()), mask=place(mk), cam=cam, cam_to_rig=T))
                out.append(cams)
            return out
        self.cases = {"(a) shared-dev": rigs(True, dev), "(b) shared-host": rigs(True, lambda a: a), "(c) own-dev": rigs(False, dev)}
        torch.cuda.synchronize()
        self.tabs = {}
        for name, rg in self.cases.items():
            bt, _, _, _, k1 = B._rig_frames([(f, rg[f]) for f in range(NF)])
            singles = [B._rig_cameras(rg[f]) for f in range(NF)]
            self.tabs[name] = (bt, singles)
            self.keep += [k1, singles]
        self.n = np.zeros(NF, np.int32); self.nraw = np.zeros(NF, np.int32); self.rcs = np.zeros(NF, np.int32)
        self.n1 = C.c_int(0); self.nraw1 = C.c_int(0)
        P = synth.LAUNCH_PARAMS
        args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], P["max_iter"], P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
        Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
        self.trk = []
        for i in range(2 * NF):
            t = B.trackdlo(*args, ctx=ctx, slot=i)
            t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
            self.trk.append(t)
        self.tab_a = (vp * NF)(*[t.h for t in self.trk[:NF]])
        self.vis = np.zeros((NF, M), np.int32); self.ext = np.zeros((NF, M), np.int32); self.nv = np.zeros(NF, np.int32); self.ne = np.zeros(NF, np.int32)
        self.st = (B.Stats * (2 * NF))()
        self.v1 = np.zeros(M, np.int32); self.e1 = np.zeros(M, np.int32); self.nv1 = C.c_int(0); self.ne1 = C.c_int(0); self.st1 = (B.Stats * 2)()

    def chk(self, rc):
        if rc:
            self.ctx._chk(rc)

    def batch(self, name, F):
        self.chk(self.lib.tdlo_rig_to_cloud_batch(self.ctx.h, C.cast(self.tabs[name][0], vp), F, self.rows, self.cols, LEAF, self.n.ctypes.data, self.nraw.ctypes.data,
                                                  self.rcs.ctypes.data))

    def single(self, name, F):
        for f in range(F):
            tab, Kc, rows, cols, _ = self.tabs[name][1][f]
            self.chk(self.lib.tdlo_rig_to_cloud(self.ctx.h, NF + f, C.cast(tab, vp), Kc, rows, cols, LEAF, None, 0, C.byref(self.n1), C.byref(self.nraw1)))

    def trackers_batch(self, F):
        p = lambda a: a.ctypes.data
        rc = self.lib.tdlo_tracker_frames_from_rig_batch(C.cast(self.tab_a, vp), F, C.cast(self.tabs["(a) shared-dev"][0], vp), self.rows, self.cols, LEAF, D_VIS, p(self.vis),
                                                         p(self.nv), p(self.ext), p(self.ne), p(self.n), p(self.nraw), C.cast(self.st, vp), p(self.rcs))
        self.chk(rc)

    def trackers_single(self, F):
        for f in range(F):
            tab, Kc, rows, cols, _ = self.tabs["(a) shared-dev"][1][f]
            self.chk(self.lib.tdlo_tracker_frame_from_rig(self.trk[NF + f].h, C.cast(tab, vp), Kc, rows, cols, LEAF, D_VIS, self.v1.ctypes.data, C.byref(self.nv1),
                                                          self.e1.ctypes.data, C.byref(self.ne1), C.byref(self.n1), C.byref(self.nraw1), C.cast(self.st1, vp)))

    def same_clouds(self, F):
        for f in range(F):
            a, b = self.ctx.get_cloud(f), self.ctx.get_cloud(NF + f)
            if a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
                return False
        return True


def timed(fn, reps):
    fn(); fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def rule(lines):
    """The smallest measured F from which on every batch value of every line lies below every single-calls value; 33 if none."""
    ok = {F: all(max(b) < min(s) for (FF, b, s) in lines if FF == F) for F in FS}
    best = 33
    for F in reversed(FS):
        if not ok[F]:
            break
        best = F
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_batch_ab.txt"))
    ap.add_argument("--trace", default=None, choices=list(SIZES))
    a = ap.parse_args()
    if a.trace:
        b = Bench(a.trace)
        for _ in range(10):
            b.batch("(a) shared-dev", NF)
        print("%s: ten calls of F = %d of (a); counters 49 / 50: %s" % (a.trace, NF, b.ctx.rig_batch_route_counts()))
        b.ctx.close()
        return 0
    out = ["# scripts/gpu_rig_batch.py --rounds %d --reps %d: ms per call (host clock, stream waited for): median [the rounds' values], batch call | F single calls" % (a.rounds, a.reps),
           "# K = %d cameras, rope frames of %d nodes; bits: the clouds of the batch slots and of the single slots compared as uint64 before a line is printed" % (K, M)]
    cloud_lines, tracker_lines = [], []
    for size in SIZES:
        b = Bench(size)
        out.append("%s  kept pixels of the rig: %d" % (size, b.kept))
        for name in list(b.cases) + ["(d) trackers"]:
            for F in FS:
                fb = (lambda: b.trackers_batch(F)) if name.startswith("(d)") else (lambda: b.batch(name, F))
                fs = (lambda: b.trackers_single(F)) if name.startswith("(d)") else (lambda: b.single(name, F))
                before = b.ctx.rig_batch_route_counts()
                vb, vs = [], []
                for _ in range(a.rounds):
                    vb.append(timed(fb, a.reps)); vs.append(timed(fs, a.reps))
                if not name.startswith("(d)"):                   # (the trackers of the two sides move on their own: their clouds are those of line (a))
                    fb(); fs()
                    if not b.same_clouds(F):
                        print("\n".join(out))
                        print("%s %s F=%d: the clouds DIFFER: stopping" % (size, name, F))
                        return 1
                after = b.ctx.rig_batch_route_counts()
                out.append("  %-16s F=%2d  batch %.3f [%s]  |  singles %.3f [%s]  |  served / passed per call %s" % (
                    name, F, float(np.median(vb)), " ".join("%.3f" % x for x in vb), float(np.median(vs)), " ".join("%.3f" % x for x in vs),
                    [round((x - y) / (a.rounds * (a.reps + 2) + (0 if name.startswith("(d)") else 1)), 2) for x, y in zip(after, before)]))
                (tracker_lines if name.startswith("(d)") else cloud_lines).append((F, vb, vs))
        b.ctx.close()
    out.append("the rule over (a) - (c), both sizes: kRigBatchMin = %d;  over (d): kRigBatchTrackerMin = %d" % (rule(cloud_lines), rule(tracker_lines)))
    text = "\n".join(out) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
