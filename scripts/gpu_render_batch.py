"""Result images for K images in one call (tdlo_render_result_batch, k_render_batch) against K single calls (tdlo_render_result, k_render), and what the
two-level search costs as the ropes over one image grow.  Writes profiles/render_batch_ab.txt in the format of profiles/cloud_batch_ab.txt.

Host clock around calls that return with the stream waited for; per value the mean of 20 calls; 5 rounds in which the sides alternate; medians.  The single
call is the yardstick: the new call is never measured against itself.  Before anything is timed both sides must have written equal bytes.
    python scripts/gpu_render_batch.py [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import render_cases as K          # noqa: E402
import render_batch_cases as BC   # noqa: E402
from trackdlo_amd import binding as B   # noqa: E402

CALLS, ROUNDS = 20, 5
KS = (1, 2, 4, 8, 16, 32)


def timed(fn):
    fn(); fn()                       # warm: arenas grown, pages touched
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    return (time.perf_counter() - t0) / CALLS * 1e3


def alternate(sides):
    """sides: [(label, fn)] -> {label: [ROUNDS values]}, the sides taking turns within every round."""
    out = {label: [] for label, _ in sides}
    for _ in range(ROUNDS):
        for label, fn in sides:
            out[label].append(timed(fn))
    return out


def line(label, vals):
    return "  %-60s" % label + "".join("%10.4f" % v for v in vals) + "   median%10.4f" % float(np.median(vals))


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "render_batch_ab.txt")
    ctx = B.Context(device=0, timing=False)
    rows_out = ["Result images for K images in one call against K single calls; host clock around calls that return with the stream waited for (scripts/gpu_render_batch.py)"]
    for rows, cols in ((480, 640), (720, 1280)):
        c = K.bench_frame(rows, cols)
        rng = np.random.default_rng(rows)
        Kmax = max(KS)
        rope45 = [BC.random_rope(rng, rows, cols, 45, k) for k in range(Kmax)]
        colour_h = [np.ascontiguousarray(np.roll(c["colour"], 7 * k, axis=1)) for k in range(Kmax)]
        occ_h = [c["occluder"]] * Kmax
        colour_d = [torch.from_numpy(colour_h[0]).cuda()]          # the one resident frame of the device-resident sides
        occ_d = torch.from_numpy(np.ascontiguousarray(c["occluder"])).cuda()
        out_d = torch.zeros((Kmax, rows, cols, 3), dtype=torch.uint8, device="cuda")          # 3 P is a multiple of 4 at both sizes: every image in place
        out_h = [np.zeros((rows, cols, 3), dtype=np.uint8) for _ in range(Kmax)]
        one_d = torch.zeros((Kmax, rows, cols, 3), dtype=torch.uint8, device="cuda")
        one_h = [np.zeros((rows, cols, 3), dtype=np.uint8) for _ in range(Kmax)]
        torch.cuda.synchronize()

        def batch(Kn, device):
            # (device-resident: every image is drawn over ONE resident frame, as the single call's colour == NULL draws over the last colour call's images)
            imgs = [dict(colour=colour_d[0] if device else colour_h[k], occluder=occ_d if device else occ_h[k], out=out_d[k] if device else out_h[k]) for k in range(Kn)]
            return lambda: ctx.render_result_batch(imgs, rope45[:Kn], shape=(rows, cols))

        def singles(Kn, device):
            def run():
                for k in range(Kn):
                    r = rope45[k]
                    if device:          # (the single call's device-resident form: the images the last colour call left on the device)
                        ctx.render_result(None, None, r["Y"], r["proj"], r["vis"], shape=(rows, cols), out=one_d[k])
                    else:
                        ctx.render_result(colour_h[k], occ_h[k], r["Y"], r["proj"], r["vis"], out=one_h[k])
            return run

        # both sides write equal bytes, corners included
        b = ctx.render_result_batch([dict(colour=colour_h[k], occluder=occ_h[k], out=out_h[k]) for k in range(Kmax)], rope45, shape=(rows, cols))
        same = True
        for k in range(Kmax):
            r = rope45[k]
            img, cor = ctx.render_result(colour_h[k], occ_h[k], r["Y"], r["proj"], r["vis"], out=one_h[k])
            same = same and np.array_equal(img, b[0][k]) and cor == b[1][k]
        ctx.colour_mask(colour_h[0], B.make_colour_params([[90, 90, 30]], [[130, 255, 255]]), occ_h[0])          # leaves colour_h[0] and its occluder resident
        batch(Kmax, True)(); singles(Kmax, True)()
        torch.cuda.synchronize()
        same = same and bool(torch.equal(out_d, one_d))
        if not same:
            raise SystemExit("the two sides wrote different bytes: nothing is timed")
        rows_out.append(f"== {cols}x{rows}: one 45-node rope per image; both sides wrote equal bytes: {same}")
        rows_out.append(f"   ms per call, mean of {CALLS} calls; {ROUNDS} alternating rounds")
        first = {"device": 0, "pageable": 0}
        for Kn in KS:
            rows_out.append(f" K = {Kn}")
            res = alternate([("tdlo_render_result_batch, device sources and destinations", batch(Kn, True)),
                             ("K x tdlo_render_result, resident frame, device destinations", singles(Kn, True)),
                             ("tdlo_render_result_batch, pageable both ways", batch(Kn, False)),
                             ("K x tdlo_render_result, pageable both ways", singles(Kn, False))])
            for label, vals in res.items():
                rows_out.append(line(label, vals))
            v = list(res.values())
            wins = {"device": max(v[0]) < min(v[1]), "pageable": max(v[2]) < min(v[3])}
            rows_out.append("   every batch value below every single-calls value: device %s (%.4f / %.4f)  pageable %s (%.4f / %.4f)" %
                            (wins["device"], np.median(v[0]), np.median(v[1]), wins["pageable"], np.median(v[2]), np.median(v[3])))
            for kind in first:
                if wins[kind] and not first[kind]:
                    first[kind] = Kn
                elif not wins[kind]:
                    first[kind] = 0
        rows_out.append(f"   {cols}x{rows}: the batch wins throughout from K = {first['device'] or 'none'} (device-resident) / {first['pageable'] or 'none'} (pageable)")
        # (b) R ropes over one image: the two-level search against the single-rope kernel
        rows_out.append(" R ropes of 45 nodes over ONE image (device sources and destination); the single call draws one rope")
        sides = [("tdlo_render_result, 1 rope", singles(1, True))]
        for Rn in (1, 3, 32):
            ropes = [dict(r, image=0) for r in rope45[:Rn]]
            im = [dict(colour=colour_d[0], occluder=occ_d, out=out_d[0])]
            sides.append((f"tdlo_render_result_batch, {Rn} rope(s)", (lambda ropes=ropes, im=im: ctx.render_result_batch(im, ropes, shape=(rows, cols)))))
        for label, vals in alternate(sides).items():
            rows_out.append(line(label, vals))
    ctx.close()
    text = "\n".join(rows_out) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
