"""What the clouds of F slots cost in one call against F single calls (profiles/cloud_batch_ab.txt is this script's output).

    python scripts/gpu_cloud_batch.py [--rounds 5] [--reps 20] [--out profiles/cloud_batch_ab.txt] [--trace DIR]

trackdlo_amd.synth rope frames (depth image + mask, 45 nodes) at 640 x 480 and 1280 x 720, F = 1, 2, 3, 4, 8, 16, 32 distinct frames.  One context of 64 slots:
slots 0 .. 31 are filled by the batch calls, slots 32 .. 63 by the single calls.  The two ways alternate inside every round; every value is the mean of `reps`
calls, timed with the host clock (time.perf_counter) around calls that return with the stream waited for; a line holds every round's value and their median.
The entry points are called through ctypes with arguments marshalled once.  The process runs under TDLO_CLOUD_BATCH_MIN=1 and TDLO_TRACKER_BATCH_MIN=2 (unless
the variables are set), so that the batch launch is on record at every size and the library's crossover can be read from the lines.

   pageable  tdlo_depth_to_cloud_batch (K = F images in ordinary host memory)   against  F x tdlo_depth_to_cloud (the default, team route) on the same arrays
   pinned    the batch call on F images in page-locked host memory of the caller's  against  F x tdlo_depth_to_cloud on the context's pinned image buffers,
             read in place (tdlo_image_buffers; the same image F times, nothing copied into them inside the timed loop: the single side at its cheapest)
   shared    (not part of the rule) the batch call with ONE pageable image shared by the F frames: one camera, F ropes -- the images go up once
   trackers  tdlo_tracker_frames_batch   against  F x tdlo_depth_to_cloud + tdlo_tracker_frame_batch, pageable images, the trackers at rest on their ropes

The rule for the library's crossover (csrc/tdlo_api.cpp, kCloudBatchMin): the smallest F from which on every batch value of `pageable`, `pinned` and
`trackers` lies below every single-calls value of the same line pair, at both sizes; printed at the end of each size and over both.

Every size is a process of its own under a time limit of its own (this process starts them and touches no GPU itself); the first step that fails ends the run.
--trace DIR: one more step, under `rocprofv3 --kernel-trace --stats` into DIR -- ten batch calls of F = 32 at each size, for the batch kernel's duration."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("TDLO_CLOUD_BATCH_MIN", "1")
os.environ.setdefault("TDLO_TRACKER_BATCH_MIN", "2")
sys.path.insert(0, ROOT)

M, FS, LEAF, D_VIS, NF = 45, (1, 2, 3, 4, 8, 16, 32), 0.008, 0.06, 32
SIZES = {"640x480": (480, 640, 400000), "1280x720": (720, 1280, 600000)}      # (rows, cols, surface samples: about 8 470 and 32 300 masked pixels -- the kernel takes 32 704)
vp = C.c_void_p


def frames_of(size):
    from trackdlo_amd import synth
    rows, cols, samples = SIZES[size]
    out = []
    for i in range(NF):
        depth, mask, cam, _ = synth.depth_scene(M, config=31, frame=i, rows=rows, cols=cols, samples=samples)
        out.append((np.ascontiguousarray(depth), np.ascontiguousarray(mask), (cam["fx"], cam["fy"], cam["cx"], cam["cy"])))
    return out


class Bench:
    def __init__(self, size):
        import torch
        from trackdlo_amd import binding as B, synth
        self.B = B
        self.rows, self.cols, _ = SIZES[size]
        self.fr = frames_of(size)
        self.ctx = ctx = B.Context(device=0, max_frames=2 * NF, max_points=1 << 15, max_nodes=64, timing=False)
        self.lib = ctx.lib
        self.cam = self.fr[0][2]
        pageable = [dict(depth=d, mask=m, cam=cam) for d, m, cam in self.fr]
        self.pin = [(torch.from_numpy(d.view(np.int16).copy()).pin_memory(), torch.from_numpy(m.copy()).pin_memory()) for d, m, _ in self.fr]
        pinned = [dict(depth=d, mask=m, cam=cam) for (d, m), (_, _, cam) in zip(self.pin, self.fr)]
        self.tab_page = B._batch_images(pageable); self.tab_pin = B._batch_images(pinned); self.tab_one = B._batch_images(pageable[:1])
        self.frames = (B.BatchFrame * NF)(); self.frames_one = (B.BatchFrame * NF)()
        for i in range(NF):
            self.frames[i].slot, self.frames[i].image = i, i
            self.frames_one[i].slot, self.frames_one[i].image = i, 0
        self.n = np.zeros(NF, np.int32); self.nraw = np.zeros(NF, np.int32); self.rcs = np.zeros(NF, np.int32)
        self.n1 = C.c_int(0); self.nraw1 = C.c_int(0)
        self.pd = [vp(d.ctypes.data) for d, _, _ in self.fr]; self.pm = [vp(m.ctypes.data) for _, m, _ in self.fr]
        bd, bm = ctx.image_buffers(self.rows, self.cols)
        bd[:] = self.fr[0][0]; bm[:] = self.fr[0][1]
        self.bd, self.bm = vp(bd.ctypes.data), vp(bm.ctypes.data)
        # trackers: 0 .. 31 on the batch side, 32 .. 63 on the single side
        P = synth.LAUNCH_PARAMS
        args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], P["max_iter"], P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
        Y0 = synth.nodes(M); coord = synth.geodesic_coord(Y0)
        self.trk = []
        for i in range(2 * NF):
            t = B.trackdlo(*args, ctx=ctx, slot=i)
            t.initialize_nodes(Y0); t.initialize_geodesic_coord(coord)
            self.trk.append(t)
        self.tab_a = (vp * NF)(*[t.h for t in self.trk[:NF]]); self.tab_b = (vp * NF)(*[t.h for t in self.trk[NF:]])
        self.image_of = np.arange(NF, dtype=np.int32)
        self.vis = np.zeros((NF, M), np.int32); self.ext = np.zeros((NF, M), np.int32); self.nv = np.zeros(NF, np.int32); self.ne = np.zeros(NF, np.int32)
        self.st = (B.Stats * (2 * NF))()

    def chk(self, rc):
        if rc:
            self.ctx._chk(rc)

    def _batch(self, tab, frames, F):
        t, K, rows, cols, _ = tab
        self.chk(self.lib.tdlo_depth_to_cloud_batch(self.ctx.h, C.cast(t, vp), min(K, F), rows, cols, C.cast(frames, vp), F, LEAF, self.n.ctypes.data, self.nraw.ctypes.data,
                                                    self.rcs.ctypes.data))

    def batch_pageable(self, F):
        self._batch(self.tab_page, self.frames, F)

    def batch_pinned(self, F):
        self._batch(self.tab_pin, self.frames, F)

    def batch_shared(self, F):
        self._batch(self.tab_one, self.frames_one, F)

    def single_pageable(self, F, first=NF):
        for i in range(F):
            self.chk(self.lib.tdlo_depth_to_cloud(self.ctx.h, first + i, self.pd[i], self.pm[i], self.rows, self.cols, *self.fr[i][2], LEAF, None, 0, C.byref(self.n1), C.byref(self.nraw1)))

    def single_pinned(self, F):
        for i in range(F):
            self.chk(self.lib.tdlo_depth_to_cloud(self.ctx.h, NF + i, self.bd, self.bm, self.rows, self.cols, *self.cam, LEAF, None, 0, C.byref(self.n1), C.byref(self.nraw1)))

    def trackers_batch(self, F):
        t, K, rows, cols, _ = self.tab_page
        self.chk(self.lib.tdlo_tracker_frames_batch(C.cast(self.tab_a, vp), F, C.cast(t, vp), K, rows, cols, self.image_of.ctypes.data, None, LEAF, D_VIS, self.vis.ctypes.data,
                                                    self.nv.ctypes.data, self.ext.ctypes.data, self.ne.ctypes.data, self.n.ctypes.data, self.nraw.ctypes.data,
                                                    C.cast(self.st, vp), self.rcs.ctypes.data))

    def trackers_single(self, F):
        self.single_pageable(F)
        self.chk(self.lib.tdlo_tracker_frame_batch(C.cast(self.tab_b, vp), F, D_VIS, self.vis.ctypes.data, self.nv.ctypes.data, self.ext.ctypes.data, self.ne.ctypes.data,
                                                   C.cast(self.st, vp), self.rcs.ctypes.data))


def timed(fn, F, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(F)
    return (time.perf_counter() - t0) / reps * 1e3


def line(label, vals):
    print(f"  {label:<58}" + "".join(f"{v:10.4f}" for v in vals) + f"   median{np.median(vals):10.4f}", flush=True)


PAIRS = (("pageable", "batch_pageable", "single_pageable", "tdlo_depth_to_cloud_batch, pageable images", "F x tdlo_depth_to_cloud, pageable images"),
         ("pinned", "batch_pinned", "single_pinned", "tdlo_depth_to_cloud_batch, caller-pinned images", "F x tdlo_depth_to_cloud, the context's pinned buffers"),
         ("trackers", "trackers_batch", "trackers_single", "tdlo_tracker_frames_batch", "F x tdlo_depth_to_cloud + tdlo_tracker_frame_batch"))


def step_measure(size, rounds, reps):
    b = Bench(size)
    for _ in range(30):          # the trackers onto their ropes: from here on both registrations stop early
        b.trackers_batch(NF); b.trackers_single(NF)
    b.batch_pageable(NF); b.single_pageable(NF)
    same = all(np.array_equal(b.ctx.get_cloud(i).view(np.uint64), b.ctx.get_cloud(NF + i).view(np.uint64)) for i in range(NF))
    r0 = b.ctx.cloud_batch_route_counts()
    b.batch_pageable(NF)
    r1 = b.ctx.cloud_batch_route_counts()
    print(f"== {size}: {NF} rope frames, masked pixels {min(int(np.count_nonzero(m)) for _, m, _ in b.fr)} .. {max(int(np.count_nonzero(m)) for _, m, _ in b.fr)}, "
          f"cloud points {int(b.n.min())} .. {int(b.n.max())}, leaf {LEAF}; a call of {NF} frames: {r1[0] - r0[0]} served by the batch launch, {r1[1] - r0[1]} passed on; "
          f"slots of the two sides equal bit for bit: {same}; TDLO_CLOUD_BATCH_MIN {os.environ['TDLO_CLOUD_BATCH_MIN']}, TDLO_TRACKER_BATCH_MIN {os.environ['TDLO_TRACKER_BATCH_MIN']}")
    print(f"   ms per call, mean of {reps} calls; {rounds} alternating rounds")
    wins = {}
    for F in FS:
        rows = {}
        for _, fb, fs, _, _ in PAIRS:
            getattr(b, fb)(F); getattr(b, fs)(F)          # every shape once before it is timed
        b.batch_shared(F)
        for _ in range(rounds):
            for _, fb, fs, _, _ in PAIRS:
                rows.setdefault(fb, []).append(timed(getattr(b, fb), F, reps))
                rows.setdefault(fs, []).append(timed(getattr(b, fs), F, reps))
            rows.setdefault("batch_shared", []).append(timed(b.batch_shared, F, reps))
        print(f" F = {F}")
        for _, fb, fs, lb, ls in PAIRS:
            line(lb, rows[fb]); line(ls, rows[fs])
        line("tdlo_depth_to_cloud_batch, one pageable image shared", rows["batch_shared"])
        wins[F] = all(max(rows[fb]) < min(rows[fs]) for _, fb, fs, _, _ in PAIRS)
        print(f"   every batch value below every single-calls value: {wins[F]}  " +
              "  ".join(f"{k}: {np.median(rows[fb]):.4f} / {np.median(rows[fs]):.4f} ({np.median(rows[fb]) / np.median(rows[fs]):.2f})" for k, fb, fs, _, _ in PAIRS))
    first = next((F for F in FS if all(wins[G] for G in FS if G >= F)), None)
    print(f"   {size}: the batch wins from F = {first} on" if first else f"   {size}: no F <= {NF} from which the batch wins throughout")
    print(f"CROSSOVER {size} {first if first else 0}", flush=True)
    b.ctx.close()


def step_trace():
    for size in SIZES:
        b = Bench(size)
        for _ in range(10):
            b.batch_pageable(NF)
        b.ctx.close()
    print("trace step done: 10 calls of 32 frames at each size")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_batch_ab.txt"))
    ap.add_argument("--trace", default=None)
    ap.add_argument("--step", default=None)
    o = ap.parse_args()
    if o.step == "trace":
        return step_trace()
    if o.step:
        return step_measure(o.step, o.rounds, o.reps)
    text = ["Clouds for F slots in one call against F single calls; host clock around calls that return with the stream waited for (scripts/gpu_cloud_batch.py)\n"]
    cross = []
    me = [sys.executable, os.path.abspath(__file__), "--rounds", str(o.rounds), "--reps", str(o.reps)]
    for size in SIZES:
        print(f"step {size} ...", flush=True)
        try:
            r = subprocess.run(me + ["--step", size], capture_output=True, text=True, timeout=360)
        except subprocess.TimeoutExpired:
            text.append(f"step {size} ran into its time limit; nothing further was started\n")
            break
        text.append(r.stdout)
        if r.returncode != 0:
            text.append(f"step {size} ended with {r.returncode}\n{r.stderr[-3000:]}\n")
            break
        cross += [int(l.split()[2]) for l in r.stdout.splitlines() if l.startswith("CROSSOVER")]
    else:
        ok = len(cross) == len(SIZES) and all(cross)
        text.append(f"kCloudBatchMin by the rule (both sizes): {max(cross) if ok else 'above 32: no such F at both sizes'}\n")
        if o.trace:
            print("step trace ...", flush=True)
            try:
                r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", o.trace, "--"] + me + ["--step", "trace"],
                                   capture_output=True, text=True, timeout=300)
                text.append(f"rocprofv3 --kernel-trace --stats, 10 calls of 32 frames at each size: exit {r.returncode}; the kernel statistics are in {os.path.relpath(o.trace, ROOT)}\n")
            except subprocess.TimeoutExpired:
                text.append("the rocprofv3 step ran into its time limit\n")
    out = "".join(text)
    print(out)
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
