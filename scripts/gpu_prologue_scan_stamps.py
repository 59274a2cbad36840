"""Phase stamps of the two-launch prologue (shader clocks, s_memtime; instrumented build: bash scripts/build_variant.sh stamps -DTDLO_CHAIN_STAMPS):
launch A, node workgroup (setup_body<FUSED>): 0 start | 1, 2, 3 (scan: not here) | 4 nodes staged, centroid, coord | 5 nodes, accumulators cleared,
   chain links | 6 G / LLE records (none without the LLE term) | 7 end
launch B, workgroup 0 (k_scatter_scan):        0 start | 1 counts gathered, in LDS (barrier) | 2 offsets, ranks (barrier) | 3 scattered | 4 iteration-0 state written
and how long after the node workgroup's end workgroup 0 of launch B started: the point workgroups' remainder, if any, plus the kernel boundary.
With TDLO_PROLOGUE_SCAN=0 the same build stamps k_setup (0 start | 1 first pass | 2 offsets of the nodes | 3 second pass | 4 .. 7 as above)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from trackdlo_amd import binding as B, synth  # noqa: E402

_v = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tmp", "libtrackdlo_stamps.so")
if not os.environ.get("TDLO_LIBRARY") and os.path.exists(_v):
    B._lib = B.load_library(_v)
P = synth.LAUNCH_PARAMS
for N, M in ((50000, 50), (20000, 50), (65536, 64)):
    ctx = B.Context(max_points=N, max_nodes=64, timing=False)
    ctx.set_sort_reuse(False)
    X, Y0, _ = synth.scene(N, M, config=2)
    pr = B.make_params(P["beta"], P["lambda_"], P["lle_weight"], P["mu"], 1, 0.0, False)
    ctx.set_cloud(0, X)
    rows = []
    for rep in range(11):
        ctx.cpd_lle_resident(0, Y0, 0.0, pr)
        st = ctx.debug_stamps(64).astype(np.int64)
        rows.append(np.concatenate([st[16:24] - st[16], st[24:29] - st[24], [st[24] - st[23]]]))
    r = np.median(np.array(rows[2:]), axis=0).astype(int)
    print(f"N={N} M={M} scan calls {int(ctx.lib.tdlo_debug_route_count(ctx.h, 48))}: node wg {r[:8].tolist()}  launch B wg0 {r[8:13].tolist()}  "
          f"(launch B's wg0 started {r[13]} clocks after the node wg's end)", flush=True)
    ctx.close()
