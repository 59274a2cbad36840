"""Frames for tests/test_rig_batch_cpu.py (which checks, on the reference alone, that every frame the GPU file calls served or passed really is one) and
tests/test_rig_batch_gpu.py (tdlo_rig_to_cloud_batch, bit for bit against the single call and tests/rig_ref.py).  A frame is a tuple of rig_ref.Cam -- a rig
of its own; the frames of one call share the image size and the leaf.  The hard scenes are those of tests/rig_scenes.py; `companions` are ordinary rigs of
the same image size that share a call with them."""
import functools

import numpy as np

import colour_ref
import rig_ref
import rig_scenes as S
import voxel_ref

LEAF = S.LEAF
BLUE_RANGE = (*colour_ref.LAUNCH_RANGE, 0)
RED_RANGE = (*S.RED_RANGE, 0)


def route(cams, leaf, fused=True):
    """What tdlo_rig_to_cloud_batch does with the frame: 'served' by the batch launch (counter 49) or 'passed' on to the single call (50) -- from the reference
    structure alone.  The two refusals of V (8, 9) are passed on: the single call refuses them."""
    if not fused:
        return "passed"
    try:
        return "served" if S.route(cams, leaf) == "taken" else "passed"
    except (voxel_ref.TooFar, voxel_ref.TooManyCells):
        return "passed"


def counts(frames, leaf, fused=True):
    """[served, passed] over the frames (each a tuple of cameras)."""
    r = [route(cams, leaf, fused) for cams in frames]
    return [r.count("served"), r.count("passed")]


@functools.lru_cache(maxsize=None)
def companions(rows, cols):
    """Three ordinary rigs of rows x cols pixels: one mask camera without a matrix, three mask cameras with matrices of their own, two colour cameras."""
    def cam(seed, T=None, colour=False):
        depth, mask = S.surface(rows, cols, seed)
        c = (600.0, 600.0, (cols - 1) / 2, (rows - 1) / 2)
        if colour:
            return rig_ref.Cam(depth, colour=S.paint(mask, seed + 1), ranges=BLUE_RANGE, cam=c, T=T)
        return rig_ref.Cam(depth, mask, cam=c, T=T)
    turn = lambda k: S.about(S.rotation(0.04 * k, (0.3, 1.0, 0.1)), (0.0, 0.0, 0.62), (0.0003 * k, -0.0002, 0.0))
    one = (cam(7000 + rows),)
    three = (cam(7100 + rows), cam(7200 + cols, turn(1)), cam(7300 + rows + cols, turn(2)))
    colour = (cam(7400 + rows, colour=True), cam(7500 + cols, turn(1), colour=True))
    return one, three, colour


@functools.lru_cache(maxsize=None)
def ropes_under_one_colour_rig(F, K=2, rows=48, cols=56):
    """F colour frames that name the SAME K colour and depth planes under different ranges: every camera's image shows a blue band and a red band (the masks
    of two ropes), frame f segments blue when f is even and red when it is odd, every later pair under a narrower saturation range -- the planes are shared
    objects, so the binding hands the library the same addresses."""
    planes = []
    for k in range(K):
        depth, m_blue = S.surface(rows, cols, 8000 + k, keep=0.5)
        _, m_red = S.surface(rows, cols, 8100 + k, keep=0.5)
        m_red = m_red * (m_blue == 0)
        img = S.paint(m_blue, 8200 + k, S.BLUE)
        red = S.paint(m_red, 8300 + k, S.RED)
        img[m_red != 0] = red[m_red != 0]
        T = None if k == 0 else S.about(S.rotation(0.05 * k, (0.0, 1.0, 0.2)), (0.0, 0.0, 0.62), (0.0004 * k, 0.0, 0.0))
        planes.append((depth, img, T))
    frames = []
    for f in range(F):
        rng = BLUE_RANGE if f % 2 == 0 else RED_RANGE
        if f >= 2:                                                 # (a range of its own: its lower V cuts into the painted band's noise)
            lower = [[rng[0][0][0], rng[0][0][1], (198 if f % 2 == 0 else 208) + 2 * (f // 2 - 1)]]
            rng = (lower, rng[1], 0)
        frames.append(tuple(rig_ref.Cam(d, colour=img, ranges=rng, cam=S.CAM, T=T) for d, img, T in planes))
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def ropes_under_one_mask_rig(F, K=2, rows=48, cols=56):
    """F mask frames that name the same K depth planes under masks of their own."""
    depths = [S.surface(rows, cols, 8400 + k)[0] for k in range(K)]
    Ts = [None if k == 0 else S.about(S.rotation(0.05 * k, (0.0, 1.0, 0.2)), (0.0, 0.0, 0.62), (0.0004 * k, 0.0, 0.0)) for k in range(K)]
    frames = []
    for f in range(F):
        frames.append(tuple(rig_ref.Cam(depths[k], S.surface(rows, cols, 8500 + 10 * f + k, keep=0.3 + 0.1 * (f % 4))[1], cam=S.CAM, T=Ts[k]) for k in range(K)))
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def too_far(rows, cols):
    """A frame V refuses (8): a camera whose matrix moves its points 1e9 leaf sizes from the origin."""
    depth, mask = S.surface(rows, cols, 8600)
    T = S.TRANSFORMS["translation"] + np.array([[0, 0, 0, 1.0e9], [0, 0, 0, 0], [0, 0, 0, 0]])
    return (rig_ref.Cam(depth, mask, cam=S.CAM, T=T),)


@functools.lru_cache(maxsize=None)
def crowded(rows, cols):
    """A frame of more than 32 704 kept points at a small image size: as many cameras as it takes, every pixel kept, all on ONE depth plane and ONE mask plane,
    each camera shifted by a matrix of its own."""
    K = 32705 // (rows * cols) + 1
    assert K <= 64
    depth, _ = S.surface(rows, cols, 8700, keep=1.0)
    mask = np.full((rows, cols), 255, np.uint8)
    shift = lambda k: S.TRANSFORMS["identity"] + np.array([[0, 0, 0, 0.0001 * k], [0, 0, 0, 0.0], [0, 0, 0, 0.00005 * k]])
    return tuple(rig_ref.Cam(depth, mask, cam=S.CAM, T=shift(k)) for k in range(K))


@functools.lru_cache(maxsize=None)
def many_cells(rows=65, cols=64):
    """A rig whose cloud has more than 1024 cells under FINE: a result that a slot of 1024 points does not hold."""
    return S.sized(rows, cols, 3)[0]


FINE = 0.002
