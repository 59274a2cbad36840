"""The inputs of tests/test_render_gpu.py, built here so that tests/test_render_ref.py (no GPU) can confirm that every one of them passes the
reference's guards (render_ref.primitives: no pixel coordinate within 1e-9 of an integer, no two edge keys within 1e-12 relative).
A case is a dict(colour, occluder or None, Y, proj, vis, params or None)."""
import numpy as np

import render_ref as R

FX = 100.0
PROJ = R.pinhole(FX)


def image(rows, cols, seed, occluder=True):
    """A random colour image and an occluder image that mixes 0, 255 and other bytes (the blend ANDs with the byte itself)."""
    rng = np.random.default_rng(4200 + seed)
    colour = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
    occ = None
    if occluder:
        occ = rng.choice(np.array([0, 255, 255, 255, 0x5a, 1], dtype=np.uint8), size=(rows, cols))
    return colour, occ


def case(rows, cols, seed, px, vis, z=None, params=None, occluder=True):
    colour, occ = image(rows, cols, seed, occluder)
    return dict(colour=colour, occluder=occ, Y=np.asfortranarray(R.nodes_from_pixels(px, FX, z)), proj=PROJ, vis=np.asarray(vis, dtype=np.int32), params=params)


def shapes():
    """Test 1: odd width, rows * cols % 4 == 0 and == 3; horizontal, vertical, diagonal and zero-length edges; one node; two nodes."""
    out = {}
    for rows, cols in ((48, 53), (47, 53)):
        out[f"{rows}x{cols}-mixed"] = case(rows, cols, 1, [(5, 10), (30, 10), (30, 35), (12, 20), (12, 20)], [0, 2, 3])
        out[f"{rows}x{cols}-one"] = case(rows, cols, 2, [(20, 20)], [0])
        out[f"{rows}x{cols}-two"] = case(rows, cols, 3, [(8, 8), (40, 30)], [], occluder=False)
        out[f"{rows}x{cols}-tail"] = case(rows, cols, 4, [(cols - 3, rows - 1), (cols - 1, rows - 1), (cols - 20, rows - 4)], [1])      # primitives over the image's last pixels
    return out


def borders():
    """Test 2: discs and line ends on columns 255 / 256 / 0 / cols - 1, on the first and last row, in the four corners; nodes outside the image."""
    out = {}
    for rows, cols in ((33, 257), (64, 256)):
        px = [(-100, -100), (0, 0), (255, 0), (256, 5), (cols - 1, 0), (cols - 1, rows - 1), (255, rows - 1), (0, rows - 1), (128, rows // 2),
              (cols + 50, rows + 50), (256, rows - 1), (0, rows // 2), (255, rows // 2)]
        z = 1.0 + 0.013 * ((np.arange(len(px)) * 5) % len(px))
        out[f"{rows}x{cols}"] = case(rows, cols, 10, px, [1, 2, 5, 8, 9, 12], z)
    return out


def crossing():
    """Test 3: a rope that crosses itself in the image, edge order by camera distance not the index order; vis mixed, all, none."""
    px = [(8, 8), (56, 50), (56, 12), (30, 30), (8, 52), (40, 6), (40, 60)]
    z = [1.00, 1.40, 0.80, 1.25, 0.90, 1.60, 0.70]
    out = {}
    for name, vis in (("mixed", [0, 3, 4]), ("all", list(range(7))), ("none", [])):
        out[name] = case(64, 72, 20, px, vis, z)
    assert R.edge_order(out["all"]["Y"]) != list(range(5, -1, -1)) and R.edge_order(out["all"]["Y"]) != list(range(6))
    return out


def zigzag(M, seed=30):
    """Test 4: M nodes zig-zagging between the top and the bottom of a 96 x 128 image: every wave's row span meets every edge's bounding box."""
    k = np.arange(M)
    px = np.stack([2 + (k * 123) // (M - 1), np.where(k % 2 == 0, 2, 93)], axis=1)
    z = 1.0 + 0.0007 * ((k * 37) % M) + 1e-6 * k
    return case(96, 128, seed, px, k[(k % 3) != 1], z)


def all_byte_pairs():
    """Test 5: colour[r, c] = (r, r, r), occluder[r, c] = c on 256 x 256: every byte pair once."""
    r = np.arange(256, dtype=np.uint8)
    colour = np.repeat(np.repeat(r[:, None, None], 256, axis=1), 3, axis=2)
    occ = np.repeat(r[None, :], 256, axis=0)
    return dict(colour=np.ascontiguousarray(colour), occluder=np.ascontiguousarray(occ), Y=np.asfortranarray(R.nodes_from_pixels([(100, 100)], FX)), proj=PROJ,
                vis=np.zeros(0, dtype=np.int32), params=None)


def corner_cases():
    """Test 5: occluders with no zero, a single zero at pixel 0, a single zero at the last pixel, a rectangle; and no occluder."""
    rows, cols = 41, 54
    out = {}
    for name in ("none", "first", "last", "rect", "no-occluder"):
        c = case(rows, cols, 50, [(10, 10), (44, 30)], [0], occluder=False)
        if name != "no-occluder":
            occ = np.full((rows, cols), 255, dtype=np.uint8)
            if name == "first":
                occ[0, 0] = 0
            elif name == "last":
                occ[-1, -1] = 0
            elif name == "rect":
                occ[7:19, 21:40] = 0
            c["occluder"] = occ
        out[name] = c
    return out


def bench_frame(rows, cols):
    """Test 8: bench.py's frame_from_depth scene (synth.depth_scene(30, config=9, frame=3)) with its colour image; the scene's nodes moved onto the rope as
    the images show it (depth_scene's inter-frame shift), which also takes the end nodes off the exact pixel row cy that the guard refuses."""
    import colour_ref
    from trackdlo_amd import synth
    _, colour, occ, _, cam, Y0 = synth.colour_scene(30, *colour_ref.LAUNCH_RANGE, config=9, frame=3, rows=rows, cols=cols, occluder=(rows // 3, rows // 2, cols // 4, cols // 3))
    return dict(colour=colour, occluder=occ, Y=np.asfortranarray(Y0 + np.array([0.0, 0.005, 0.0])), proj=R.pinhole(cam["fx"], cam["fy"], cam["cx"], cam["cy"]),
                vis=np.arange(0, 30, 2, dtype=np.int32), params=None)


def cpu_checkable():
    """Every case above that does not need a GPU to form its inputs, by name."""
    out = {}
    for group, cases in (("shapes", shapes()), ("borders", borders()), ("crossing", crossing()), ("corners", corner_cases())):
        out.update({f"{group}/{k}": v for k, v in cases.items()})
    out["zigzag/300"] = zigzag(300)
    out["zigzag/1024"] = zigzag(1024, 31)
    out["blend"] = all_byte_pairs()
    out["bench/480x640"] = bench_frame(480, 640)
    out["bench/720x1280"] = bench_frame(720, 1280)
    return out
