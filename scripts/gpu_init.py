"""What starting a tracker from its first cloud costs (profiles/init_ab.txt holds a run).  N = 5 000 / M = 45 and N = 50 000 / M = 50, mu 0.05, 100
iterations of reg (the prototype's call values), a synthetic rope near the origin.  Host clock around calls that end synchronised, after warm-up.

  python scripts/gpu_init.py --mode ab --parent scripts/tmp/libtrackdlo_parent.so
      What ordering and installing add on top of reg: this tree's trackdlo.initialize_from_cloud against the PARENT commit's tdlo_reg alone, same
      cloud and iteration count.  One child process per library and pair (TDLO_LIBRARY), alternating, --pairs pairs; every value and the medians.
  python scripts/gpu_init.py --mode routes
      The device order against TDLO_INIT_SORT=host (read when the context is made: one child process per route and pair, alternating).
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o init -- python scripts/gpu_init.py --mode kernel
      k_sort_pts alone: --calls tdlo_sort_pts calls at M = 45, 300 and 1024 (shuffled ropes of tests/init_ref.py); the kernel's time is read off
      the trace's statistics (k_sort_pts<true> serves M = 45, k_sort_pts<false> the other two: run one M per trace with --nodes to tell those apart).
Any HIP error raises: the process exits non-zero."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = ((5000, 45), (50000, 50))
MU, ITERS = 0.05, 100

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("ab", "routes", "child", "kernel"), required=True)
ap.add_argument("--what", choices=("init", "reg"), default="init", help="child: the call that is timed")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--nodes", type=int, nargs="*", default=[45, 300, 1024], help="kernel: the node counts")
ap.add_argument("--parent", default=os.path.join(ROOT, "scripts", "tmp", "libtrackdlo_parent.so"), help="ab: the parent commit's library")
args = ap.parse_args()


def child():
    """Prints one line per size: ms per call (mean of --calls calls after two warm-up calls)."""
    import init_ref as R
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, timing=False)
    for N, M in SIZES:
        X = R.rope_cloud(N, seed=N + M)
        if args.what == "init":
            trk = B.trackdlo(M, ctx=ctx)
            fn = lambda: trk.initialize_from_cloud(X, MU, ITERS)
        else:
            fn = lambda: ctx.reg(X, M, MU, ITERS)
        fn(); fn()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        print(f"RESULT {N} {M} {(time.perf_counter() - t0) * 1e3 / args.calls:.4f}", flush=True)
    ctx.close()


def run_child(what, env_extra):
    env = dict(os.environ, **env_extra)
    for k in ("TDLO_INIT_SORT", "TDLO_LIBRARY"):
        if k not in env_extra:
            env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "child", "--what", what, "--calls", str(args.calls)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
    return {(int(a), int(b)): float(c) for _, a, b, c in (line.split() for line in r.stdout.splitlines() if line.startswith("RESULT"))}


def compare(name_a, a, name_b, b):
    rows = {s: ([], []) for s in SIZES}
    for _ in range(args.pairs):
        for which, (what, env) in enumerate((a, b)):
            for s, v in run_child(what, env).items():
                rows[s][which].append(v)
    for (N, M), (va, vb) in rows.items():
        print(f"N = {N}, M = {M}, {ITERS} iterations, ms per call:")
        print(f"   {name_a:44s} {' '.join(f'{v:8.4f}' for v in va)}   median {statistics.median(va):8.4f}  spread {max(va) - min(va):.4f}")
        print(f"   {name_b:44s} {' '.join(f'{v:8.4f}' for v in vb)}   median {statistics.median(vb):8.4f}  spread {max(vb) - min(vb):.4f}")
        print(f"   difference of the medians {statistics.median(va) - statistics.median(vb):+.4f} ms")


if args.mode == "child":
    child()
elif args.mode == "ab":
    if not os.path.exists(args.parent):
        sys.exit(f"{args.parent}: build the parent commit's library there first (a git worktree of the parent, make -C trackdlo_amd/csrc)")
    compare("this tree: initialize_from_cloud", ("init", {}), "parent commit: tdlo_reg alone", ("reg", {"TDLO_LIBRARY": args.parent}))
elif args.mode == "routes":
    compare("k_sort_pts behind reg (default)", ("init", {}), "TDLO_INIT_SORT=host", ("init", {"TDLO_INIT_SORT": "host"}))
else:
    import init_ref as R
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, timing=False)
    for M in args.nodes:
        Y = R._shuffled(R._curve(M, 40 + M), (M * 5) // 7, 200 + M)[0]
        t0 = time.perf_counter()
        for _ in range(args.calls):
            ctx.sort_pts(Y)
        print(f"M = {M}: {args.calls} tdlo_sort_pts calls, {(time.perf_counter() - t0) * 1e3 / args.calls:.4f} ms per call on the host clock (upload, kernel, read-back, wait)")
    ctx.close()
