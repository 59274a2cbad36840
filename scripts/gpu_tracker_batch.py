"""What stepping F trackers in one call costs against stepping them one by one (profiles/tracker_batch_ab.txt is this script's output).

    python scripts/gpu_tracker_batch.py [--rounds 5] [--reps 30]

Production size: N = 5 000 points, M = 45 nodes, steady state (the trackers have converged onto their clouds: both registrations stop in their first
iteration) -- once with every node visible, once with the middle third of the chain hidden.  One process, one context of 64 slots: trackers 0 .. 31 are
stepped by the batch calls, trackers 32 .. 63 (the same nodes on the same clouds) by the single calls.  F = 1, 2, 3, 4, 8, 16, 32; the two ways alternate
inside every round; every value is the mean of `reps` calls, timed with the host clock (time.perf_counter) around calls that return with the stream
waited for; the line holds every round's value and their median.  The entry points are called through ctypes with arguments marshalled once, so the
figures are the library's, not the Python binding's.  The process runs under TDLO_TRACKER_BATCH_MIN=2 (unless the variable is set): the tracker calls take the
batch route from two trackers on, so that both sides are on record at every size and the library's default crossover can be read from the lines.

   frame    tdlo_tracker_frame_batch            against  F x (tdlo_visibility_prepass + tdlo_tracker_tracking_step)
   prepass  tdlo_visibility_prepass_batch       against  F x tdlo_visibility_prepass
   step     tdlo_tracker_tracking_step_batch against F x tdlo_tracker_tracking_step on given visible sets; the batch call's wall time less its batches' own
            host time (tdlo_stats.host_ms, summed over the pre-processing groups and the main batches) is what the host spends between and around them -- guide nodes, F sets of priors (traverse_euclidean), marshalling -- while
            the GPU has nothing to do
   priors   F x the two tdlo_traverse_euclidean calls of an all-visible tracker, on their own: the part of that a device form would take over"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

os.environ.setdefault("TDLO_TRACKER_BATCH_MIN", "2")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trackdlo_amd import binding as B, synth      # noqa: E402

N, M, FS, D_VIS = 5000, 45, (1, 2, 3, 4, 8, 16, 32), 0.06
vp = C.c_void_p


def ptr(a):
    return a.ctypes.data_as(vp)


class Side:
    """F trackers and everything their calls need, marshalled once."""
    def __init__(self, ctx, first_slot, clouds, args):
        Y0 = synth.nodes(M); self.coord = np.ascontiguousarray(synth.geodesic_coord(Y0))
        self.ctx = ctx; self.lib = ctx.lib
        self.trk = []
        for i, X in enumerate(clouds):
            t = B.trackdlo(*args, ctx=ctx, slot=first_slot + i)
            t.initialize_nodes(Y0); t.initialize_geodesic_coord(self.coord)
            ctx.set_cloud(first_slot + i, X)
            self.trk.append(t)
        F = len(clouds)
        self.slots = np.arange(first_slot, first_slot + F, dtype=np.int32)
        self.tab = (vp * F)(*[t.h for t in self.trk])
        self.vis = np.zeros((F, M), dtype=np.int32); self.ext = np.zeros((F, M), dtype=np.int32)
        self.nv = np.zeros(F, dtype=np.int32); self.ne = np.zeros(F, dtype=np.int32)
        self.pv = (vp * F)(*[self.vis[i].ctypes.data for i in range(F)]); self.pe = (vp * F)(*[self.ext[i].ctypes.data for i in range(F)])
        ip = C.POINTER(C.c_int)
        self.pnv = [C.cast(vp(self.nv[i:].ctypes.data), ip) for i in range(F)]; self.pne = [C.cast(vp(self.ne[i:].ctypes.data), ip) for i in range(F)]
        self.st = (B.Stats * (2 * F))(); self.rcs = np.zeros(F, dtype=np.int32)
        self.Y = np.zeros((F, 3 * M)); self.dist = np.zeros((F, M)); self.coords = np.ascontiguousarray(np.tile(self.coord, (F, 1)))
        self.thr = args[1]
        # every pointer the timed calls pass, made once (a ctypes conversion costs about a microsecond)
        self.p = {k: ptr(getattr(self, k)) for k in ("vis", "nv", "ext", "ne", "rcs", "slots", "Y", "coords", "dist", "coord")}
        self.p.update(tab=C.cast(self.tab, vp), st=C.cast(self.st, vp), pv=C.cast(self.pv, vp), pe=C.cast(self.pe, vp))
        self.pY = [vp(self.Y[i].ctypes.data) for i in range(F)]; self.pdist = [vp(self.dist[i].ctypes.data) for i in range(F)]
        self.pst = [C.cast(C.byref(self.st, 2 * i * C.sizeof(B.Stats)), vp) for i in range(F)]
        self.islot = [int(x) for x in self.slots]; self.h = [t.h for t in self.trk]

    def nodes(self, F):
        for i in range(F):
            self.lib.tdlo_tracker_get_tracking_result(self.h[i], self.pY[i])

    def chk(self, rc):
        if rc:
            self.ctx._chk(rc)

    # ---- the batch calls
    def frame_batch(self, F):
        p = self.p
        self.chk(self.lib.tdlo_tracker_frame_batch(p["tab"], F, D_VIS, p["vis"], p["nv"], p["ext"], p["ne"], p["st"], p["rcs"]))

    def prepass_batch(self, F):
        p = self.p
        self.chk(self.lib.tdlo_visibility_prepass_batch(self.ctx.h, F, p["slots"], p["Y"], M, self.thr, D_VIS, p["coords"], p["dist"], p["vis"], p["nv"], p["ext"], p["ne"]))

    def step_batch(self, F):
        p = self.p
        self.chk(self.lib.tdlo_tracker_tracking_step_batch(p["tab"], F, p["pv"], p["nv"], p["pe"], p["ne"], None, p["st"], p["rcs"]))

    # ---- the single calls, one tracker after the other
    def prepass_single(self, F):
        for i in range(F):
            self.chk(self.lib.tdlo_visibility_prepass(self.ctx.h, self.islot[i], self.pY[i], M, self.thr, D_VIS, self.p["coord"], self.pdist[i],
                                                      self.pv[i], self.pnv[i], self.pe[i], self.pne[i]))

    def frame_single(self, F):
        lib = self.lib
        for i in range(F):
            h = self.h[i]
            lib.tdlo_tracker_get_tracking_result(h, self.pY[i])
            self.chk(lib.tdlo_visibility_prepass(self.ctx.h, self.islot[i], self.pY[i], M, self.thr, D_VIS, self.p["coord"], self.pdist[i],
                                                 self.pv[i], self.pnv[i], self.pe[i], self.pne[i]))
            self.chk(lib.tdlo_tracker_tracking_step(h, None, 0, self.pv[i], int(self.nv[i]), self.pe[i], int(self.ne[i]), None, self.pst[i]))

    def step_single(self, F):
        for i in range(F):
            self.chk(self.lib.tdlo_tracker_tracking_step(self.h[i], None, 0, self.pv[i], int(self.nv[i]), self.pe[i], int(self.ne[i]), None, self.pst[i]))

    def host_ms(self, F):
        """(pre-processing, main) host time of the last batch call's run_frames calls: one per distinct chain length; one or two main batches."""
        pre, main = {}, {}
        for i in range(F):
            pre.setdefault(int(self.ne[i]), self.st[2 * i].host_ms)
            main.setdefault(int(self.ne[i]) == M, self.st[2 * i + 1].host_ms)
        return sum(pre.values()), sum(main.values())

    def iters(self, F):
        return sorted({(self.st[2 * i].iters, self.st[2 * i + 1].iters) for i in range(F)})


def timed(fn, F, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn(F)
    return (time.perf_counter() - t0) / reps * 1e3


def priors_alone(side, F, reps):
    fn = side.lib.tdlo_traverse_euclidean
    Y0 = np.asfortranarray(synth.nodes(M)); ve = np.arange(M, dtype=np.int32); out = np.zeros(4 * (M + 2))
    pc, py, pvv, po = ptr(side.coord), ptr(Y0), ptr(ve), ptr(out)
    t0 = time.perf_counter()
    for _ in range(reps):
        for _ in range(F):
            fn(pc, M, py, M, pvv, M, 0, -1, po)
            fn(pc, M, py, M, pvv, M, 1, -1, po)
    return (time.perf_counter() - t0) / reps * 1e3


def line(label, vals):
    print(f"  {label:<44}" + "".join(f"{v:10.4f}" for v in vals) + f"   median{np.median(vals):10.4f}", flush=True)


def scene(name, occlude, rounds, reps):
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], P["max_iter"], P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    ctx = B.Context(device=0, max_frames=64, max_points=8192, max_nodes=64, timing=False)
    clouds = [synth.scene(N, M, config=77, frame=i, occlude=occlude)[0] for i in range(32)]
    a, b = Side(ctx, 0, clouds, args), Side(ctx, 32, clouds, args)
    for _ in range(40):          # onto the clouds: from here on both registrations stop in their first iteration
        a.frame_batch(32); b.frame_single(32)
    same = all(np.array_equal(x.get_tracking_result(), y.get_tracking_result()) for x, y in zip(a.trk, b.trk))
    print(f"== {name}: N = {len(clouds[0])} .. {max(len(c) for c in clouds)} points, M = {M}; visible_nodes_extended {sorted(set(int(x) for x in a.ne))} of {M}; "
          f"(pre-processing, main) iterations batch {a.iters(32)} single {b.iters(32)}; nodes after the warm-up equal bit for bit: {same} "
          f"(TDLO_ESTEP2 {os.environ.get('TDLO_ESTEP2', 'unset: a batch that fills the GPU takes k_estep2, a frame alone k_estep')}; "
          f"TDLO_TRACKER_BATCH_MIN {os.environ['TDLO_TRACKER_BATCH_MIN']})")
    print(f"   ms per call, mean of {reps} calls; {rounds} alternating rounds")
    res = {}
    for F in FS:
        rows = {k: [] for k in ("frame batch", "frame single", "prepass batch", "prepass single", "step batch", "step single", "host_ms pre", "host_ms main", "priors alone")}
        a.frame_batch(F); b.frame_single(F); a.nodes(F); a.prepass_batch(F); a.step_batch(F); b.frame_single(F); b.step_single(F); a.frame_batch(F)      # every shape once before it is timed
        for _ in range(rounds):
            rows["frame batch"].append(timed(a.frame_batch, F, reps))
            rows["frame single"].append(timed(b.frame_single, F, reps))
            a.nodes(F); b.nodes(F)
            rows["prepass batch"].append(timed(a.prepass_batch, F, reps))
            rows["prepass single"].append(timed(b.prepass_single, F, reps))
            rows["step batch"].append(timed(a.step_batch, F, reps))
            hp, hm = a.host_ms(F)
            rows["host_ms pre"].append(hp); rows["host_ms main"].append(hm)
            rows["step single"].append(timed(b.step_single, F, reps))
            rows["priors alone"].append(priors_alone(a, F, reps))
        print(f" F = {F}")
        line("tdlo_tracker_frame_batch", rows["frame batch"])
        line("F x (prepass + tracking_step)", rows["frame single"])
        line("tdlo_visibility_prepass_batch", rows["prepass batch"])
        line("F x tdlo_visibility_prepass", rows["prepass single"])
        line("tdlo_tracker_tracking_step_batch", rows["step batch"])
        line("F x tdlo_tracker_tracking_step", rows["step single"])
        line("  the batch call's pre-processing batches", rows["host_ms pre"])
        line("  the batch call's main batches", rows["host_ms main"])
        line("  the rest: host between / around the batches", [s - p - m for s, p, m in zip(rows["step batch"], rows["host_ms pre"], rows["host_ms main"])])
        line("F x 2 tdlo_traverse_euclidean, on their own", rows["priors alone"])
        res[F] = [np.median(rows[k]) for k in ("frame batch", "frame single", "prepass batch", "prepass single", "step batch", "step single")]
    print("   summary (medians): F | frame batch / single (ratio) | prepass batch / single (ratio) | step batch / single (ratio)")
    for F, (fb, fs, pb, ps, sb, ss) in res.items():
        print(f"   {F:3d} | {fb:8.4f} / {fs:8.4f} ({fb / fs:5.2f}) | {pb:8.4f} / {ps:8.4f} ({pb / ps:5.2f}) | {sb:8.4f} / {ss:8.4f} ({sb / ss:5.2f})")
    del a, b
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    o = ap.parse_args()
    print("Trackers stepped in one call against one by one; host clock around calls that return with the stream waited for (scripts/gpu_tracker_batch.py)")
    scene("every node visible", None, o.rounds, o.reps)
    scene("the middle third of the chain hidden", (0.34, 0.66), o.rounds, o.reps)


if __name__ == "__main__":
    main()
