"""The inputs of tests/test_render_batch_gpu.py and tests/test_render_batch_ref.py: ropes as dicts {image, Y, proj, vis, params} over images as dicts
{colour, occluder}, in the form tests/render_batch_ref.py takes them (params: render_ref's dict or None).  Nodes come from integer pixels through
render_ref.nodes_from_pixels, so every projection lands half a pixel inside its pixel and the reference's guards pass."""
import numpy as np

import render_cases as K
import render_ref as R

PROJ = K.PROJ


def rope(px, image=0, vis=None, z=None, params=None):
    px = np.asarray(px).reshape(-1, 2)
    vis = np.arange(len(px)) if vis is None else vis
    return dict(image=int(image), Y=np.asfortranarray(R.nodes_from_pixels(px, K.FX, z)), proj=PROJ, vis=np.asarray(vis, dtype=np.int32), params=params)


def random_rope(rng, rows, cols, M, image, params=None, margin=10):
    """M nodes at random pixels, some of them outside the image; depths a random permutation of distinct steps (the edge order is not the index order)."""
    px = np.stack([rng.integers(-margin, cols + margin, size=M), rng.integers(-margin, rows + margin, size=M)], axis=1)
    z = 1.0 + 0.0113 * rng.permutation(M) + 1e-5 * np.arange(M)
    vis = np.flatnonzero(rng.random(M) < 0.6)
    return rope(px, image, vis, z, params)


def images(K_, rows, cols, seed, occluders=None):
    """K_ random images; occluders: per image True / False (default: alternating, starting with one)."""
    out = []
    for k in range(K_):
        occ = (k % 2 == 0) if occluders is None else bool(occluders[k])
        colour, o = K.image(rows, cols, seed + 17 * k, occ)
        out.append(dict(colour=colour, occluder=o))
    return out


def two_node_fan(n, rows=64, cols=64):
    """n two-node ropes on one image that all pass through its centre, each with colours of its own: the rope drawn last decides the centre."""
    out = []
    for i in range(n):
        a = (3 + (i * 7) % (cols - 6), 2 + (i % 3))
        b = (cols - 1 - a[0], rows - 1 - a[1])
        prm = dict(line_width=3, node_radius=2, edge_visible=(i % 251 + 1, (i // 251) + 1, 7), edge_hidden=(i % 251 + 1, (i // 251) + 1, 9),
                   node_visible=(3, i % 251 + 1, 200), node_hidden=(4, i % 251 + 1, 100))
        out.append(rope([a, b], 0, [0] if i % 2 else [], [1.0 + 0.001 * i, 1.2 + 0.001 * i], prm))
    return out
