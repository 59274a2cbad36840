"""What dealing one cloud out among F trackers costs (writes profiles/cloud_assign_ab.txt).  F = 2, 4, 8, 32 ropes of 45 nodes, a source of 5 000 F points.
Line 1: tdlo_tracker_frames_from_shared_cloud_batch against the host composition through the same library -- tdlo_get_cloud + tdlo_cloud_assign_host + F
tdlo_set_cloud + tdlo_tracker_frame_batch.  Line 2: the pre-pass riding in the split (TDLO_ASSIGN_RIDE=1) against ride off, on tdlo_cloud_assign_visibility.
Every compared pair is checked bit-equal before it is timed; medians of 30 calls after 5 warm-up calls, the pairs interleaved.  The route rule was set before
measuring (include/trackdlo_hip.h): the ride becomes the default only if it is no slower on every line."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from trackdlo_amd import binding as B, synth      # noqa: E402
import assign_ref as AR                             # noqa: E402

M, REPS, WARM = 45, 30, 5


def ctx_under(ride, F):
    old = os.environ.pop("TDLO_ASSIGN_RIDE", None)
    if ride:
        os.environ["TDLO_ASSIGN_RIDE"] = "1"
    try:
        return B.Context(device=0, timing=False, max_frames=F + 1, max_points=5000 * F, max_nodes=64)
    finally:
        os.environ.pop("TDLO_ASSIGN_RIDE", None)
        if old is not None:
            os.environ["TDLO_ASSIGN_RIDE"] = old


def trackers(c, ropes, coords):
    P = synth.LAUNCH_PARAMS
    args = (M, P["visibility_threshold"], P["beta"], P["lambda_"], P["alpha"], P["k_vis"], P["mu"], 30, P["tol"], P["beta_pre_proc"], P["lambda_pre_proc"], P["lle_weight"])
    out = []
    for i, Y in enumerate(ropes):
        t = B.trackdlo(*args, ctx=c, slot=i)
        t.initialize_nodes(Y); t.initialize_geodesic_coord(coords[i])
        out.append(t)
    return out


def median_ms(fn, reset):
    ts = []
    for k in range(WARM + REPS):
        reset()
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        if k >= WARM:
            ts.append(dt * 1e3)
    return float(np.median(ts))


def main():
    lines = []
    for F in (2, 4, 8, 32):
        X, ropes, coords = AR.cloud_scene(5000 * F, (M,) * F, seed=F, far=0.05)
        ca, cb = ctx_under(False, F), ctx_under(False, F)
        ta, tb = trackers(ca, ropes, coords), trackers(cb, ropes, coords)
        ca.set_cloud(F, X); cb.set_cloud(F, X)

        def reset():
            for t, Y in zip(ta + tb, ropes + ropes):
                t.initialize_nodes(Y)

        def device():
            return B.frames_from_shared_cloud_batch(ta, F, 0.02, 0.06)

        def host():
            Xh = cb.get_cloud(F)
            own = B.cloud_assign_host(Xh, [t.get_tracking_result() for t in tb], 0.02)[0]
            for f in range(F):
                cb.set_cloud(f, Xh[own == f])
            return B.frame_batch(tb, 0.06)
        reset(); a = device(); b = host()
        same = a[0] == b[0] and all(np.array_equal(x.get_tracking_result(), y.get_tracking_result()) and x.get_sigma2() == y.get_sigma2() for x, y in zip(ta, tb))
        assert same, F
        lines.append(f"line 1  F={F:2d}  n={5000 * F:6d}  tracker call {median_ms(device, reset):.3f} ms   host composition {median_ms(host, reset):.3f} ms   bit-equal")
        ca.close(); cb.close()
        cr, cn = ctx_under(True, F), ctx_under(False, F)
        cr.set_cloud(F, X); cn.set_cloud(F, X)
        rl = list(zip(range(F), ropes))
        ra = cr.cloud_assign_visibility(F, rl, 0.02, 0.008, 0.06, coords); rb = cn.cloud_assign_visibility(F, rl, 0.02, 0.008, 0.06, coords)
        assert ra[:2] == rb[:2] and all(np.array_equal(AR.bits(p), AR.bits(q)) for p, q in zip(ra[2], rb[2])) and cr.assign_route_counts()[1] == 1
        lines.append(f"line 2  F={F:2d}  n={5000 * F:6d}  ride on {median_ms(lambda: cr.cloud_assign_visibility(F, rl, 0.02, 0.008, 0.06, coords), lambda: None):.3f} ms   "
                     f"ride off {median_ms(lambda: cn.cloud_assign_visibility(F, rl, 0.02, 0.008, 0.06, coords), lambda: None):.3f} ms   bit-equal")
        cr.close(); cn.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    open(os.path.join(ROOT, "profiles", "cloud_assign_ab.txt"), "w").write(text)


if __name__ == "__main__":
    main()
