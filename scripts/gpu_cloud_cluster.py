"""What starting F same-coloured ropes from one cloud costs (writes profiles/cloud_cluster_ab.txt).  F = 2, 4, 8, 32 ropes of 45 nodes 10 cm apart, a source of
5 000 F points interleaved point by point (the scene family of scripts/gpu_cloud_assign.py, no far points), tol = 3 voxel leaves of 8 mm = 24 mm: the ropes are
more than 3 tol apart and the cloud has exactly F clusters.
Line 1: tdlo_tracker_initialize_from_shared_cloud_batch against the host composition through the same library -- tdlo_get_cloud + tdlo_cloud_cluster_host + F
        tdlo_set_cloud + tdlo_tracker_initialize_from_cloud_batch.  The host statement's own time is on line 2: it is the plain ALL-PAIRS statement, not a tuned
        host clustering, so the ratio of line 1 flatters the device.
Line 3: tdlo_cloud_cluster alone, the device route against the host route (TDLO_CLUSTER=host) -- the pair the route rule of include/trackdlo_hip.h is about.
Line 4: tdlo_tracker_initialize_from_cloud_batch alone on clouds split beforehand: line 1's device figure minus this is what clustering adds to a start-up,
        and it is the number that matters.
Every compared pair is checked bit-equal before it is timed.  Medians; the two sides of a pair alternate call by call; the host sides of the large scenes
(seconds to minutes per call) are timed over fewer calls, the checked call among them; the count is on the line.  Every F runs in a child process of its own under a time limit; the first that fails
ends the run."""
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M, TOL, MIN_SIZE, MU, ITERS = 45, 0.024, 50, 0.05, 30
REPS, WARM = 20, 3


def scene(F):
    import assign_ref as AR
    X, _, _ = AR.cloud_scene(5000 * F, (M,) * F, seed=F, far=0.0)
    X = np.array(X, order="F")
    X[:, 1] += 0.05 * (np.arange(len(X)) % F)          # rope k at height 0.10 k instead of 0.05 k
    return X


def ctx_under(B, host, F):
    old = os.environ.pop("TDLO_CLUSTER", None)
    if host:
        os.environ["TDLO_CLUSTER"] = "host"
    try:
        return B.Context(device=0, timing=False, max_frames=F + 1, max_points=5000 * F, max_nodes=64)
    finally:
        os.environ.pop("TDLO_CLUSTER", None)
        if old is not None:
            os.environ["TDLO_CLUSTER"] = old


def trackers(B, c, F):
    from trackdlo_amd import synth
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    return [B.trackdlo(*args, ctx=c, slot=i) for i in range(F)]


def timed(fn):
    t0 = time.perf_counter(); out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def pair_ms(fa, fb, reps_b, tb=()):
    """Medians of fa and fb, alternating: REPS calls of fa, reps_b <= REPS of fb spread among them (tb: samples of fb taken already -- the call that was
    checked bit-equal counts where a call takes seconds)."""
    ta, tb = [], list(tb)
    every = max(1, REPS // max(reps_b, 1))
    for k in range(WARM + REPS):
        _, dt = timed(fa)
        if k >= WARM:
            ta.append(dt)
            if (k - WARM) % every == 0 and len(tb) < reps_b:
                tb.append(timed(fb)[1])
    return float(np.median(ta)), float(np.median(tb))


def one(F):
    from trackdlo_amd import binding as B
    import assign_ref as AR
    X = scene(F)
    n = len(X)
    reps_host = REPS if n <= 10000 else 5 if n <= 20000 else 2 if n <= 40000 else 1
    slots = list(range(F))
    ca, cb, cc, ch = ctx_under(B, False, F), ctx_under(B, False, F), ctx_under(B, False, F), ctx_under(B, True, F)
    ta, tb, tc = trackers(B, ca, F), trackers(B, cb, F), trackers(B, cc, F)
    for c in (ca, cb, ch):
        c.set_cloud(F, X)
    host_ms = []

    def device():
        return B.initialize_from_shared_cloud_batch(ta, F, TOL, MIN_SIZE, MU, ITERS)

    def host():
        Xh = cb.get_cloud(F)
        t0 = time.perf_counter()
        own = B.cloud_cluster_host(Xh, F, TOL, MIN_SIZE)[0]
        host_ms.append((time.perf_counter() - t0) * 1e3)
        for f in range(F):
            cb.set_cloud(f, Xh[own == f])
        return B.initialize_from_cloud_batch(tb, MU, ITERS)

    def state(ts):
        return [(AR.bits(t.get_tracking_result()).tolist(), AR.bits(t.get_guide_nodes()).tolist()) for t in ts]
    a = device(); b, first = timed(host)
    assert a[2] == F and a[0] == b[0] == [0] * F and np.array_equal(AR.bits(a[1]), AR.bits(b[1])) and state(ta) == state(tb), F
    d, h = pair_ms(device, host, reps_host, [first])
    print(f"line 1  F={F:2d}  n={n:6d}  tracker call {d:.3f} ms   host composition {h:.3f} ms ({reps_host} calls)   bit-equal", flush=True)
    print(f"line 2  F={F:2d}  n={n:6d}  of which tdlo_cloud_cluster_host, the all-pairs statement: {float(np.median(host_ms)):.3f} ms", flush=True)

    ra = ca.cloud_cluster(F, slots, TOL, MIN_SIZE, owners=True); rh, first = timed(lambda: ch.cloud_cluster(F, slots, TOL, MIN_SIZE, owners=True))
    assert ra[:3] == rh[:3] and np.array_equal(ra[3], rh[3]) and all(np.array_equal(AR.bits(ca.get_cloud(f)), AR.bits(ch.get_cloud(f))) for f in slots), F
    assert ca.cluster_route_counts()[1] == 0 and ch.cluster_route_counts()[0] == 0
    d2, h2 = pair_ms(lambda: ca.cloud_cluster(F, slots, TOL, MIN_SIZE), lambda: ch.cloud_cluster(F, slots, TOL, MIN_SIZE), reps_host, [first])
    print(f"line 3  F={F:2d}  n={n:6d}  tdlo_cloud_cluster device route {d2:.3f} ms   host route {h2:.3f} ms ({reps_host} calls)   bit-equal", flush=True)

    for f in slots:
        cc.set_cloud(f, ca.get_cloud(f))
    c3 = B.initialize_from_cloud_batch(tc, MU, ITERS)
    assert c3[0] == [0] * F and np.array_equal(AR.bits(c3[1]), AR.bits(a[1])) and state(tc) == state(ta), F
    d3, d1 = pair_ms(lambda: B.initialize_from_cloud_batch(tc, MU, ITERS), device, REPS)
    print(f"line 4  F={F:2d}  n={n:6d}  initialize_from_cloud_batch on pre-split clouds {d3:.3f} ms   tracker call {d1:.3f} ms   clustering adds {d1 - d3:.3f} ms   bit-equal",
          flush=True)
    for c in (ca, cb, cc, ch):
        c.close()


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one(int(sys.argv[2]))
        return
    text = ""
    for F in (2, 4, 8, 32):
        with subprocess.Popen([sys.executable, os.path.abspath(__file__), "--one", str(F)], stdout=subprocess.PIPE, text=True) as child:
            timer = threading.Timer(600.0, child.kill)
            timer.start()
            for line in child.stdout:                  # (shown as it comes: a line of the large scenes takes minutes)
                print(line, end="", flush=True)
                text += line
            rc = child.wait()
            timer.cancel()
        if rc:
            sys.exit(rc)
    open(os.path.join(ROOT, "profiles", "cloud_cluster_ab.txt"), "w").write(text)


if __name__ == "__main__":
    main()
