"""Numpy statement of the result images for many ropes (tdlo_render_result_batch, csrc/tdlo_render_batch.hip), a few lines over render_ref's functions:

  per image k:  img = blend(colour_k, occluder_k)
                for rope in ropes whose image == k, in the order of the caller's list:  if rope has more than one node: paint(img, primitives(rope))
                corners_k = corners(occluder_k)

The blend ONCE, then each rope exactly as the single call draws its one rope; ropes in list order, so a later rope paints over an earlier one.  The reference
(trackdlo_node.cpp:377-452) has one rope and gives no order across ropes: list order is what R successive drawing passes over one blended image give.
An image without a rope is the blend alone; an image with one rope is render_ref.render's.  Parity against OpenCV's own rasterisers stays unpinned.

table(): the host half's records (tdlo_render_batch_table) formed independently from render_ref.primitives."""
import numpy as np

import render_ref as RR


def render_batch(images, ropes, rows, cols, guard=True):
    """images: dicts {colour [rows x cols x 3], occluder [rows x cols] or None}; ropes: dicts {image, Y, proj, vis, params (render_ref's dict or None)}.
    Returns ([image], [corners])."""
    K = len(images)
    for r in ropes:
        if not 0 <= int(r["image"]) < K:
            raise ValueError("a rope's image is outside 0 .. K - 1")
    prims = [RR.primitives(r["Y"], r["proj"], r["vis"], r.get("params"), guard) for r in ropes]      # (all of them validated before anything is drawn)
    outs, cors = [], []
    for k, im in enumerate(images):
        assert np.asarray(im["colour"]).shape == (rows, cols, 3)
        img = RR.blend(im["colour"], im.get("occluder"))
        for r, p in zip(ropes, prims):
            if int(r["image"]) == k and len(r["Y"]) > 1:
                RR.paint(img, p)
        outs.append(img); cors.append(RR.corners(im.get("occluder")))
    return outs, cors


def box(rec):
    """(c_lo, r_lo, c_hi, r_hi) of one primitive record, inflated as the kernels inflate it: a disc by its radius, a line by (width + 1) >> 1."""
    kind, c0, r0, c1, r1, size = (int(v) for v in rec[:6])
    ext = size if kind == 1 else (size + 1) >> 1
    return min(c0, c1) - ext, min(r0, r1) - ext, max(c0, c1) + ext, max(r0, r1) + ext


def table(ropes, K, guard=True):
    """(heads [R x 8], prims [n x 8], rope_first [K + 1]): the ropes ordered stably by image, per rope {the union of its primitives' boxes, first primitive,
    number of primitives, 0, 0} (a one-node rope: no primitive, the empty box {0, 0, -1, -1}), the ropes' records one after the other."""
    order = sorted(range(len(ropes)), key=lambda i: (int(ropes[i]["image"]), i))
    first = [sum(1 for r in ropes if int(r["image"]) < k) for k in range(K + 1)]
    heads, prims = [], []
    for i in order:
        r = ropes[i]
        p = RR.primitives(r["Y"], r["proj"], r["vis"], r.get("params"), guard)
        b = [box(rec) for rec in p]
        u = [min(x[0] for x in b), min(x[1] for x in b), max(x[2] for x in b), max(x[3] for x in b)] if b else [0, 0, -1, -1]
        heads.append(u + [len(prims), len(p), 0, 0])
        prims.extend(p.tolist())
    return (np.asarray(heads, dtype=np.int32).reshape(-1, 8), np.asarray(prims, dtype=np.int32).reshape(-1, 8), np.asarray(first, dtype=np.int32))
