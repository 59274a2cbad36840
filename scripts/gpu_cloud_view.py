"""What taking a cloud as it arrives costs, and what k_cloud_import reaches (profiles/cloud_view_ab.txt holds a run).

  python scripts/gpu_cloud_view.py --mode e2e
      One process, N = 5 000, 50 000 and 2 000 000, packed row-major float32 source.  Host clock around calls that end in a stream wait, after
      warm-up; the alternatives alternate, five rounds, every value printed (ms per call, mean of --calls calls):
        (a) the caller's widening pass (binding._f64: float64, column-major) + Context.set_cloud, the two parts apart
        (b) Context.set_cloud_view from host memory (packed in pinned memory as float32, widened by the kernel reading that block in place)
        (c) Context.set_cloud_view from a device tensor
        (d) as (b) with the packed block copied to the device in front of the kernel (a context made under TDLO_VIEW_INPLACE=0)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cv -- python scripts/gpu_cloud_view.py --mode kernel
      Per size: --calls device-view imports (k_cloud_import) and as many device-to-device hipMemcpyAsync of the algorithmic 36 N bytes (12 read +
      24 written per point), both also timed in the process by stream events.
  python scripts/gpu_cloud_view.py --mode summarize --trace DIR
      k_cloud_import's time per size from the kernel trace: achieved bytes/s over 36 N, its share of the measured HBM copy rate and of the HBM
      peak (MI355X: 6.29 TB/s measured by a float4 copy, 8 TB/s specified), and the ratio to the device-to-device copy of the same bytes.
Any HIP error raises: the process exits non-zero."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (5000, 50000, 2000000)
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("e2e", "kernel", "summarize"), required=True)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--trace", default=None, help="summarize: the directory rocprofv3 wrote")
ap.add_argument("--manifest", default=os.path.join(ROOT, "scripts", "tmp", "cloud_view_kernel_manifest.json"), help="kernel mode writes, summarize reads: sizes and dispatch counts")
args = ap.parse_args()


def cloud(N):
    import numpy as np
    from trackdlo_amd import synth
    chunk = 250000
    X = np.concatenate([synth.scene(min(chunk, N - lo), 45, config=4, frame=lo // chunk)[0] for lo in range(0, N, chunk)], axis=0)
    return np.ascontiguousarray(X.astype(np.float32))


def ms(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def e2e():
    import numpy as np
    import torch
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, max_points=SIZES[-1], timing=False)
    os.environ["TDLO_VIEW_INPLACE"] = "0"
    copied = B.Context(device=0, max_points=SIZES[-1], timing=False)
    del os.environ["TDLO_VIEW_INPLACE"]
    for N in SIZES:
        X32 = cloud(N)
        Xd = torch.from_numpy(X32).cuda()
        X64 = B._f64(X32)
        calls = args.calls if N <= 50000 else max(3, args.calls // 4)
        alts = [("a1 widen on the host (_f64)", lambda: B._f64(X32)),
                ("a2 set_cloud (float64)", lambda: ctx.set_cloud(0, X64)),
                ("b  set_cloud_view host", lambda: ctx.set_cloud_view(0, X32)),
                ("c  set_cloud_view device", lambda: ctx.set_cloud_view(0, Xd)),
                ("d  set_cloud_view host, copy form", lambda: copied.set_cloud_view(0, X32))]
        for _, fn in alts:
            ms(fn, 3)
        rows = {name: [] for name, _ in alts}
        for _ in range(args.rounds):
            for name, fn in alts:
                rows[name].append(ms(fn, calls))
        print(f"N = {N}  (ms per call, mean of {calls} calls; {args.rounds} alternating rounds)")
        for name, _ in alts:
            v = rows[name]
            print(f"  {name:34s} " + " ".join(f"{x:9.4f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:9.4f}")
        a = [x + y for x, y in zip(rows[alts[0][0]], rows[alts[1][0]])]
        print(f"  {'a  = a1 + a2':34s} " + " ".join(f"{x:9.4f}" for x in a) + f"   median {sorted(a)[len(a) // 2]:9.4f}")
        want = np.asfortranarray(X32.astype(np.float64))
        for c in (ctx, copied):
            assert np.array_equal(c.get_cloud(0).view(np.uint64), want.view(np.uint64))
    ctx.close(); copied.close()


def kernel():
    import torch
    from trackdlo_amd import binding as B
    ctx = B.Context(device=0, max_points=SIZES[-1], timing=False)
    ext = torch.cuda.ExternalStream(ctx.stream_ptr())
    out = []
    for N in SIZES:
        Xd = torch.from_numpy(cloud(N)).cuda()
        src = torch.empty(36 * N, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        src.zero_()
        view = B.cloud_view(Xd, asynchronous=True)
        torch.cuda.synchronize()
        rounds = []
        for r in range(args.rounds + 1):                  # (round 0 is the warm-up; the trace holds it too: summarize drops it)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            with torch.cuda.stream(ext):
                e[0].record()
                for _ in range(args.calls):
                    ctx.set_cloud_view(0, view)
                e[1].record()
            ctx.synchronize()
            e[2].record()
            for _ in range(args.calls):
                dst.copy_(src, non_blocking=True)
            e[3].record()
            torch.cuda.synchronize()
            if r:
                rounds.append((e[0].elapsed_time(e[1]) * 1e3 / args.calls, e[2].elapsed_time(e[3]) * 1e3 / args.calls))
        print(f"N = {N}: stream events, us per call back to back (import | device-to-device copy of {36 * N} bytes): " + "  ".join(f"{a:.2f}|{b:.2f}" for a, b in rounds))
        out.append(dict(N=N, calls=args.calls, rounds=args.rounds + 1))
    ctx.close()
    os.makedirs(os.path.dirname(args.manifest), exist_ok=True)
    with open(args.manifest, "w") as f:
        json.dump(out, f)


def column(row, *parts):
    for k in row:
        if all(p in k.lower() for p in parts):
            return k
    raise KeyError(parts)


def summarize():
    manifest = json.load(open(args.manifest))

    def durations(pattern, keep):
        files = glob.glob(os.path.join(args.trace, "**", pattern), recursive=True)
        assert files, f"no {pattern} under {args.trace}"
        rows = list(csv.DictReader(open(files[0])))
        ks, ke = column(rows[0], "start"), column(rows[0], "end")
        rows = [r for r in rows if keep(r)]
        rows.sort(key=lambda r: int(r[ks]))
        return [(int(r[ke]) - int(r[ks])) * 1e-3 for r in rows]                    # us

    kern = durations("*kernel_trace.csv", lambda r: "k_cloud_import" in r[column(r, "kernel", "name")])
    # (the runtime serves a device-to-device hipMemcpyAsync with a kernel of its own: it is in the kernel trace, not among the memory copies)
    copies = durations("*kernel_trace.csv", lambda r: "rocclr_copyBuffer" in r[column(r, "kernel", "name")])
    per = [m["calls"] * m["rounds"] for m in manifest]
    assert len(kern) == sum(per), (len(kern), per)
    have_copies = len(copies) == sum(per)
    if not have_copies:
        print(f"(the trace holds {len(copies)} dispatches of the runtime's copy kernel, not {sum(per)}: copy times below are left out)")
    at = 0
    for m, n in zip(manifest, per):
        N, calls = m["N"], m["calls"]
        k = kern[at + calls:at + n]; c = copies[at + calls:at + n] if have_copies else []
        at += n
        line = f"N = {N}: k_cloud_import, us per dispatch by round (median of {calls}):"
        meds = []
        for r in range(m["rounds"] - 1):
            part = sorted(k[r * calls:(r + 1) * calls]); meds.append(part[len(part) // 2])
        med = sorted(meds)[len(meds) // 2]
        rate = 36.0 * N / (med * 1e-6)
        print(line + " " + " ".join(f"{x:.2f}" for x in meds))
        print(f"    median {med:.2f} us -> {rate / 1e12:.3f} TB/s over 36 N = {36 * N} bytes: {100 * rate / HBM_MEASURED:.1f} % of the measured HBM copy rate (6.29 TB/s), "
              f"{100 * rate / HBM_SPEC:.1f} % of the specified peak (8 TB/s)")
        if c:
            cm = []
            for r in range(m["rounds"] - 1):
                part = sorted(c[r * calls:(r + 1) * calls]); cm.append(part[len(part) // 2])
            cmed = sorted(cm)[len(cm) // 2]
            print(f"    device-to-device hipMemcpyAsync of the same bytes, us by round: " + " ".join(f"{x:.2f}" for x in cm) +
                  f"   median {cmed:.2f} us; kernel / copy = {med / cmed:.2f} (rounds' spread: kernel {min(meds):.2f} .. {max(meds):.2f}, copy {min(cm):.2f} .. {max(cm):.2f})")


{"e2e": e2e, "kernel": kernel, "summarize": summarize}[args.mode]()
