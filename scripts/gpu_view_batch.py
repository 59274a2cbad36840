"""What the cloud views of F slots cost in one call against F single calls.  profiles/view_batch_ab.txt and profiles/view_batch_ab_run2.txt are this script's
output, two runs, as it wrote them; profiles/view_batch_notes.txt is written by hand (what a further run showed whose output was not kept).

    python scripts/gpu_view_batch.py [--rounds 5] [--reps 20] [--out profiles/view_batch_ab.txt] [--trace DIR]

trackdlo_amd.synth rope frames (640 x 480, 45 nodes) as CLOUDS, F = 1, 2, 3, 4, 8, 16, 32 distinct frames.  One context of 64 slots: slots 0 .. 31 are filled by
the batch calls, slots 32 .. 63 by the single calls -- whose code is the parent commit's, so the single-calls lines ARE the parent.  The two ways alternate
inside every round; every value is the mean of `reps` calls, timed with the host clock (time.perf_counter) around calls that return with the stream waited
for; a line holds every round's value and their median.  The entry points are called through ctypes with arguments marshalled once.  The process runs under
TDLO_VIEW_BATCH_MIN=1 and TDLO_TRACKER_BATCH_MIN=2 (unless the variables are set), so that the batch launches are on record at every size.

   voxel-dev   tdlo_cloud_view_voxel_grid_batch on F packed float32 device views of 5 000 rope points   against  F x tdlo_cloud_view_voxel_grid
   voxel-host  ... on F host views at PointXYZRGB's stride (8 floats a point), 5 000 points               against  the same
   organized   ... on F organized device clouds of 640 x 480 points under device selection bytes that keep a rope's worth   against  the same
   shared      ... on ONE organized device cloud named by all F frames, each with selection bytes of its own that keep the cloud's rope   against  the same
   import-dev  tdlo_set_cloud_view_batch on F packed float32 device views of 5 000 points   against  F x tdlo_set_cloud_view
   import-host ... on F host views at PointXYZRGB's stride   against  the same
   trackers    tdlo_tracker_frames_from_cloud_view_batch (device views of 5 000 points)   against  F x tdlo_tracker_frame_from_cloud_view, trackers at rest

The rule for the library's crossovers (csrc/tdlo_api.cpp), set before the measurement: the smallest F from which on -- at that F and every larger measured F
-- every batch value lies below every single-calls value on every line; none up to 32: 33, the calls loop over the single calls.  Taken over all lines it gave
one switch; the data asked for two (the issue allows it): kViewBatchMin for the two calls by themselves is the rule over the voxel and import lines,
kViewBatchTrackerMin for the tracker calls the rule over the trackers line, the largest value over the runs on record.

The measurement is a process of its own under a time limit of its own (this process starts it and touches no GPU itself).
--trace DIR: one more step, under `rocprofv3 --kernel-trace --stats` into DIR -- ten calls of F = 32 of voxel-dev, organized and import-dev; the two batch
kernels' durations per grid are read from the kernel trace and go to the end of the output."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("TDLO_VIEW_BATCH_MIN", "1")
os.environ.setdefault("TDLO_TRACKER_BATCH_MIN", "2")
sys.path.insert(0, ROOT)

M, FS, LEAF, D_VIS, NF, NPTS = 45, (1, 2, 3, 4, 8, 16, 32), 0.008, 0.06, 32, 5000
ROWS, COLS = 480, 640
vp = C.c_void_p


def backproject(depth, fx, fy, cx, cy):
    """Every pixel's float32 point, row-major (the arithmetic of trackdlo_node.cpp:219-224)."""
    i, j = np.mgrid[0:depth.shape[0], 0:depth.shape[1]]
    z = depth.astype(np.float64) / 1000.0
    return np.stack([((j - cx) * z / fx), ((i - cy) * z / fy), z], axis=2).reshape(-1, 3).astype(np.float32)


class Bench:
    def __init__(self):
        import torch
        from trackdlo_amd import binding as B, synth
        self.B, self.torch = B, torch
        self.ctx = ctx = B.Context(device=0, max_frames=2 * NF, max_points=1 << 15, max_nodes=64, timing=False)
        self.lib = ctx.lib
        self.keep = []
        org, sel, rope = [], [], []
        for i in range(NF):
            depth, mask, cam, _ = synth.depth_scene(M, config=31, frame=i, rows=ROWS, cols=COLS, samples=400000)
            P = backproject(depth, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
            m = np.ascontiguousarray(mask).reshape(-1)
            R = P[m != 0]
            rope.append(np.ascontiguousarray(R[np.linspace(0, len(R) - 1, NPTS).astype(np.int64)]))
            org.append(P); sel.append(m.copy())
        self.masked = [int(np.count_nonzero(s)) for s in sel]
        dev = lambda a: torch.from_numpy(a).cuda()
        self.rope_dev = [dev(R) for R in rope]
        self.rope_host = []
        for R in rope:
            h = np.zeros((NPTS, 8), dtype=np.float32); h[:, :3] = R
            self.rope_host.append(h)
        self.org_dev = [dev(P) for P in org]
        self.sel_dev = [dev(s) for s in sel]
        self.sel_shared = [dev(sel[0].copy()) for _ in range(NF)]      # cloud 0's own rope, F times over: every frame of `shared` keeps a rope's worth of ONE cloud
        torch.cuda.synchronize()
        cv = B.cloud_view
        self.v_rope_dev = [cv(t) for t in self.rope_dev]
        self.v_rope_host = [cv(h) for h in self.rope_host]
        self.v_org = [cv(t) for t in self.org_dev]
        self.sp = [t.data_ptr() for t in self.sel_dev]
        self.sp_shared = [t.data_ptr() for t in self.sel_shared]

        def table(views, selects, first):
            tab = (B.ViewFrame * NF)()
            for i in range(NF):
                tab[i].slot, tab[i].view, tab[i].N, tab[i].select = first + i, C.addressof(views[i]), int(views[i].N), selects[i] if selects else None
            return tab
        self.t_dev = table(self.v_rope_dev, None, 0); self.t_host = table(self.v_rope_host, None, 0)
        self.t_org = table(self.v_org, self.sp, 0); self.t_shared = table([self.v_org[0]] * NF, self.sp_shared, 0)
        self.slots = np.arange(NF, dtype=np.int32)
        self.Ns = np.full(NF, NPTS, dtype=np.int32)
        self.pv_dev = (vp * NF)(*[C.addressof(v) for v in self.v_rope_dev]); self.pv_host = (vp * NF)(*[C.addressof(v) for v in self.v_rope_host])
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

    def _voxel_batch(self, tab, F):
        self.chk(self.lib.tdlo_cloud_view_voxel_grid_batch(self.ctx.h, C.cast(tab, vp), F, LEAF, self.n.ctypes.data, self.nraw.ctypes.data, self.rcs.ctypes.data))

    def _voxel_single(self, views, selects, F):
        for i in range(F):
            self.chk(self.lib.tdlo_cloud_view_voxel_grid(self.ctx.h, NF + i, C.byref(views[i]), int(views[i].N), selects[i] if selects else None, LEAF, None, 0,
                                                         C.byref(self.n1), C.byref(self.nraw1)))

    def b_voxel_dev(self, F): self._voxel_batch(self.t_dev, F)
    def s_voxel_dev(self, F): self._voxel_single(self.v_rope_dev, None, F)
    def b_voxel_host(self, F): self._voxel_batch(self.t_host, F)
    def s_voxel_host(self, F): self._voxel_single(self.v_rope_host, None, F)
    def b_organized(self, F): self._voxel_batch(self.t_org, F)
    def s_organized(self, F): self._voxel_single(self.v_org, self.sp, F)
    def b_shared(self, F): self._voxel_batch(self.t_shared, F)
    def s_shared(self, F): self._voxel_single([self.v_org[0]] * NF, self.sp_shared, F)

    def _import_batch(self, pv, F):
        self.chk(self.lib.tdlo_set_cloud_view_batch(self.ctx.h, self.slots.ctypes.data, C.cast(pv, vp), self.Ns.ctypes.data, F, self.rcs.ctypes.data))

    def _import_single(self, views, F):
        for i in range(F):
            self.chk(self.lib.tdlo_set_cloud_view(self.ctx.h, NF + i, C.byref(views[i]), NPTS))

    def b_import_dev(self, F): self._import_batch(self.pv_dev, F)
    def s_import_dev(self, F): self._import_single(self.v_rope_dev, F)
    def b_import_host(self, F): self._import_batch(self.pv_host, F)
    def s_import_host(self, F): self._import_single(self.v_rope_host, F)

    def b_trackers(self, F):
        self.chk(self.lib.tdlo_tracker_frames_from_cloud_view_batch(C.cast(self.tab_a, vp), F, C.cast(self.t_dev, vp), LEAF, D_VIS, self.vis.ctypes.data, self.nv.ctypes.data,
                                                                    self.ext.ctypes.data, self.ne.ctypes.data, self.n.ctypes.data, self.nraw.ctypes.data,
                                                                    C.cast(self.st, vp), self.rcs.ctypes.data))

    def s_trackers(self, F):
        for i in range(F):
            self.chk(self.lib.tdlo_tracker_frame_from_cloud_view(self.trk[NF + i].h, C.byref(self.v_rope_dev[i]), NPTS, None, LEAF, D_VIS, self.v1.ctypes.data, C.byref(self.nv1),
                                                                 self.e1.ctypes.data, C.byref(self.ne1), C.byref(self.n1), C.byref(self.nraw1), C.cast(self.st1, vp)))


def timed(fn, F, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(F)
    return (time.perf_counter() - t0) / reps * 1e3


def line(label, vals):
    print(f"  {label:<66}" + "".join(f"{v:10.4f}" for v in vals) + f"   median{np.median(vals):10.4f}", flush=True)


PAIRS = (("voxel-dev", "voxel", "tdlo_cloud_view_voxel_grid_batch, device float32 views, 5 000 points", "F x tdlo_cloud_view_voxel_grid, the same views"),
         ("voxel-host", "voxel", "tdlo_cloud_view_voxel_grid_batch, host PointXYZRGB views, 5 000", "F x tdlo_cloud_view_voxel_grid, the same views"),
         ("organized", "voxel", "tdlo_cloud_view_voxel_grid_batch, 640 x 480 organized, selections", "F x tdlo_cloud_view_voxel_grid, the same views"),
         ("shared", "voxel", "tdlo_cloud_view_voxel_grid_batch, ONE organized cloud, F selections", "F x tdlo_cloud_view_voxel_grid, the same view"),
         ("import-dev", "import", "tdlo_set_cloud_view_batch, device float32 views, 5 000 points", "F x tdlo_set_cloud_view, the same views"),
         ("import-host", "import", "tdlo_set_cloud_view_batch, host PointXYZRGB views, 5 000 points", "F x tdlo_set_cloud_view, the same views"),
         ("trackers", "trackers", "tdlo_tracker_frames_from_cloud_view_batch, device views", "F x tdlo_tracker_frame_from_cloud_view, the same views"))


def fn(b, side, key):
    return getattr(b, f"{side}_{key.replace('-', '_')}")


def step_measure(rounds, reps):
    b = Bench()
    for _ in range(30):          # the trackers onto their ropes: from here on both registrations stop early
        b.b_trackers(NF); b.s_trackers(NF)
    same = {}
    for key, _, _, _ in PAIRS[:6]:
        fn(b, "b", key)(NF); fn(b, "s", key)(NF)
        same[key] = all(np.array_equal(b.ctx.get_cloud(i).view(np.uint64), b.ctx.get_cloud(NF + i).view(np.uint64)) for i in range(NF))
    r0 = b.ctx.view_batch_route_counts()
    b.b_voxel_dev(NF); b.b_organized(NF); b.b_import_dev(NF)
    r1 = b.ctx.view_batch_route_counts()
    print(f"== {NF} rope frames of {ROWS} x {COLS}: masked pixels {min(b.masked)} .. {max(b.masked)}, rope clouds of {NPTS} points, leaf {LEAF}; calls of {NF} frames (voxel-dev, "
          f"organized, import-dev): counters 38 .. 41 moved by {[x - y for x, y in zip(r1, r0)]}; slots of the two sides equal bit for bit: {same}; "
          f"TDLO_VIEW_BATCH_MIN {os.environ['TDLO_VIEW_BATCH_MIN']}, TDLO_TRACKER_BATCH_MIN {os.environ['TDLO_TRACKER_BATCH_MIN']}")
    print(f"   ms per call, mean of {reps} calls; {rounds} alternating rounds")
    wins = {}
    for F in FS:
        rows = {}
        for key, _, _, _ in PAIRS:
            fn(b, "b", key)(F); fn(b, "s", key)(F)          # every shape once before it is timed
        for _ in range(rounds):
            for key, _, _, _ in PAIRS:
                rows.setdefault(("b", key), []).append(timed(fn(b, "b", key), F, reps))
                rows.setdefault(("s", key), []).append(timed(fn(b, "s", key), F, reps))
        print(f" F = {F}")
        for key, _, lb, ls in PAIRS:
            line(lb, rows[("b", key)]); line(ls, rows[("s", key)])
        wins[F] = {key: max(rows[("b", key)]) < min(rows[("s", key)]) for key, _, _, _ in PAIRS}
        print(f"   every batch value below every single-calls value: {all(wins[F].values())}  " +
              "  ".join(f"{key}: {np.median(rows[('b', key)]):.4f} / {np.median(rows[('s', key)]):.4f} ({np.median(rows[('b', key)]) / np.median(rows[('s', key)]):.2f})"
                        for key, _, _, _ in PAIRS))

    def first(keys):
        return next((F for F in FS if all(wins[G][k] for G in FS if G >= F for k in keys)), 0)
    for group in ("voxel", "import", "trackers"):
        keys = [k for k, g, _, _ in PAIRS if g == group]
        f = first(keys)
        print(f"   the {group} lines alone ({', '.join(keys)}): " + (f"the batch wins from F = {f} on" if f else f"no F <= {NF} from which the batch wins throughout"))
    f = first([k for k, _, _, _ in PAIRS])
    print(f"   every line: the batch wins from F = {f} on" if f else f"   every line: no F <= {NF} from which the batch wins throughout")
    bare = first([k for k, g, _, _ in PAIRS if g != "trackers"])
    print(f"CROSSOVER {f} {bare} {first(['trackers'])}", flush=True)
    b.ctx.close()


def step_trace():
    b = Bench()
    for _ in range(10):
        b.b_voxel_dev(NF); b.b_organized(NF); b.b_import_dev(NF)
    b.ctx.close()
    print("trace step done: 10 calls of 32 frames of voxel-dev, organized and import-dev")


def trace_lines(trace_dir):
    """The two batch kernels' durations per grid, from the kernel trace rocprofv3 left under trace_dir."""
    import csv
    import glob
    per = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                for k in ("k_cloud_view_batch", "k_cloud_import_batch"):
                    if k in name:
                        wx, gx, gy = int(r["Workgroup_Size_X"]), int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])
                        per.setdefault((k, gx // wx, gy, wx), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return [f"  {k}, grid ({bx}, {by}) x {wx} threads: {len(v)} launches, min {min(v):.1f} / median {np.median(v):.1f} / max {max(v):.1f} us\n"
            for (k, bx, by, wx), v in sorted(per.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_batch_ab.txt"))
    ap.add_argument("--trace", default=None)
    ap.add_argument("--step", default=None)
    o = ap.parse_args()
    if o.step == "trace":
        return step_trace()
    if o.step:
        return step_measure(o.rounds, o.reps)
    text = ["Cloud views for F slots in one call against F single calls; host clock around calls that return with the stream waited for (scripts/gpu_view_batch.py)\n"]
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(o.rounds), "--reps", str(o.reps)]
    print("step measure ...", flush=True)
    ok = False
    try:
        r = subprocess.run(me + ["--step", "measure"], capture_output=True, text=True, timeout=420)
        text.append(r.stdout)
        if r.returncode != 0:
            text.append(f"the measurement ended with {r.returncode}\n{r.stderr[-3000:]}\n")
        else:
            cross = [int(l.split()[1]) for l in r.stdout.splitlines() if l.startswith("CROSSOVER")]
            ok = len(cross) == 1
            if ok:
                none = "above 32: no such F -- 33, the calls loop over the single calls"
                text.append(f"by the rule, every line: {cross[0] if cross[0] else none}\n")
                bare, trk = (int(x) for x in r.stdout.splitlines()[[l.startswith("CROSSOVER") for l in r.stdout.splitlines()].index(True)].split()[2:4])
                text.append(f"kViewBatchMin by the rule (the voxel and import lines: the two calls by themselves): {bare if bare else none}\n")
                text.append(f"kViewBatchTrackerMin by the rule (the trackers line: the tracker calls), this run: {trk if trk else none}\n")
    except subprocess.TimeoutExpired:
        text.append("the measurement ran into its time limit; nothing further was started\n")
    if ok and o.trace:
        print("step trace ...", flush=True)
        try:
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", o.trace, "--"] + me + ["--step", "trace"],
                               capture_output=True, text=True, timeout=300)
            text.append(f"rocprofv3 --kernel-trace --stats, 10 calls of 32 frames of voxel-dev, organized and import-dev: exit {r.returncode}\n")
            text += trace_lines(o.trace)
        except subprocess.TimeoutExpired:
            text.append("the rocprofv3 step ran into its time limit\n")
    out = "".join(text)
    print(out)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
