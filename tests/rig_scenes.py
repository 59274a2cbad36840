"""Constructed rigs for tests/test_rig_ref.py (CPU: each scene's stated property is asserted there on the reference's own structure) and
tests/test_rig_gpu.py (the same scenes through tdlo_rig_to_cloud, bit for bit against tests/rig_ref.py).  A scene is (cams: [rig_ref.Cam], leaf).
Images are small: a surface about 0.6 m in front of a camera whose pixels are about 1 mm apart there, so that an 8 mm cell holds tens of pixels."""
import functools

import numpy as np

import cloud_scenes
import colour_ref
import rig_ref
import voxel_ref

LEAF = 0.008
CAM = (600.0, 600.0, 31.5, 30.5)                                    # fx, fy, cx, cy
kTile, kFTmax, kFNmax = cloud_scenes.kFPix, cloud_scenes.kFTmax, cloud_scenes.kFNmax


def tiles(cams):
    """K x Tc: the tiles of the one-launch form."""
    return len(cams) * cloud_scenes.tiles(cams[0].depth.size)


def route(cams, leaf):
    """What tdlo_rig_to_cloud does with the rig: "taken" by the one-launch kernel (counter 45) or "passed" on to the multi-launch form (46) -- the header's
    rule on the structure of the reference; a rig of more than 4095 tiles, which the host never hands to the kernel, counts as passed."""
    st = voxel_ref.structure(rig_ref.points(cams), None, leaf)
    r = cloud_scenes.route_rule(st, tiles(cams))
    return "passed" if r == "untouched" else r


def surface(rows, cols, seed, keep=0.8, z0=600, cam=CAM):
    """A tilted, slightly rough surface z0 mm away and a random mask that keeps the fraction `keep` of its pixels."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:rows, 0:cols]
    depth = (z0 + 0.7 * j + 0.4 * i + rng.integers(0, 3, (rows, cols))).astype(np.uint16)
    mask = ((rng.random((rows, cols)) < keep) * rng.integers(1, 256, (rows, cols))).astype(np.uint8)
    return depth, mask


def rotation(angle, axis):
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def about(Rm, centre, shift=(0.0, 0.0, 0.0)):
    """[Rm | b]: the rotation Rm about `centre`, then `shift` -- the transformed surface stays where the untransformed one is."""
    c = np.asarray(centre, dtype=np.float64)
    return np.concatenate([Rm, (c - Rm @ c + np.asarray(shift))[:, None]], axis=1)


IRRATIONAL = about(rotation(0.3, (1.0, 2.0, 3.0)), (0.0, 0.0, 0.62), (0.0011, -0.0007, 0.0013))      # 0.3 rad about an oblique axis, and a translation
TRANSFORMS = {
    "identity": np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1),
    "translation": np.concatenate([np.eye(3), np.array([[0.0123], [-0.0456], [0.0789]])], axis=1),
    "rotation": IRRATIONAL,
    "scale": np.concatenate([np.diag([1.7, 0.6, 1.1]), np.array([[0.01], [0.02], [-0.03]])], axis=1),
}


@functools.lru_cache(maxsize=None)
def sized(rows, cols, K):
    """K cameras of rows x cols pixels (64 x 64: one tile exactly; 65 x 64: a second tile with a tail; 1 x 1; 3 x 5), every camera but the first with a
    transform of its own."""
    cams = []
    for k in range(K):
        depth, mask = surface(rows, cols, 100 * rows + 10 * cols + k)
        mask[-1, -1] = 9                                            # (the last pixel of the last tile is kept)
        T = None if k == 0 else about(rotation(0.05 * k, (0.0, 1.0, 0.2)), (0.0, 0.0, 0.62), (0.0004 * k, 0.0, 0.0))
        cams.append(rig_ref.Cam(depth, mask, cam=(600.0, 600.0, (cols - 1) / 2, (rows - 1) / 2), T=T))
    return tuple(cams), LEAF


@functools.lru_cache(maxsize=None)
def shared_cells():
    """Two cameras on one surface, the second shifted by a fraction of a pixel: their points interleave in the same 8 mm cells, tens of points of each per
    cell -- a cell's float sum depends on which camera comes first."""
    d0, m0 = surface(48, 48, 21, keep=0.9)
    d1, m1 = surface(48, 48, 22, keep=0.9)
    a = rig_ref.Cam(d0, m0, cam=CAM)
    b = rig_ref.Cam(d1, m1, cam=CAM, T=TRANSFORMS["identity"] + np.array([[0, 0, 0, 0.00041], [0, 0, 0, 0.00033], [0, 0, 0, 0.0]]))
    return (a, b), LEAF


@functools.lru_cache(maxsize=None)
def irrational():
    """Two cameras, the second turned by 0.3 rad about an oblique axis through the surface and shifted: the transformed points have no short binary
    expansion, so rounding early or multiplying in float shows, and the two clouds overlap, so the camera order shows."""
    d0, m0 = surface(56, 60, 31)
    d1, m1 = surface(56, 60, 32)
    return (rig_ref.Cam(d0, m0, cam=CAM), rig_ref.Cam(d1, m1, cam=(610.0, 605.0, 29.0, 27.5), T=IRRATIONAL)), LEAF


@functools.lru_cache(maxsize=None)
def fused_boundary():
    """Two cameras in front of flat walls (constant depth z), each with a matrix whose x and y rows carry a large entry a on zd and the offset -(a z): the
    sum a zd + b cancels to the last bits of a double, so what is left of x and y is a camera-frame coordinate PLUS the rounding of the product a zd, at the
    scale of a float's last bit.  A fused multiply-add rounds that product away differently: for tens of pixels the fused sum and the separately rounded sum
    lie on different sides of a float rounding boundary (tests/test_rig_ref.py counts them on the statement), which no ordinary transform shows; the leaf is the pixel pitch, so that those pixels show in the cloud and not only in R.  Not a rigid
    motion: the contract does not ask for one."""
    rng = np.random.default_rng(0)
    a = 1.0e5 + 1.0 / 3.0
    cams = []
    for z0 in (600, 640):
        depth = np.full((40, 52), z0, np.uint16)
        mask = ((rng.random((40, 52)) < 0.8) * 255).astype(np.uint8)
        zd = z0 / 1000.0
        T = np.array([[1.0, 0.25, a, -(a * zd)], [0.0, 1.0, 1.37 * a, -(1.37 * a * zd)], [0.0, 0.0, 1.0, 0.0]])
        cams.append(rig_ref.Cam(depth, mask, cam=(600.0, 600.0, 25.5, 19.5), T=T))
    return tuple(cams), 0.001                                       # (a 1 mm leaf: a cell holds a pixel or two, so a point's last bit shows in its centroid)


@functools.lru_cache(maxsize=None)
def transform(kind):
    d0, m0 = surface(40, 52, 41)
    d1, m1 = surface(40, 52, 42)
    return (rig_ref.Cam(d0, m0, cam=CAM), rig_ref.Cam(d1, m1, cam=CAM, T=TRANSFORMS[kind])), LEAF


@functools.lru_cache(maxsize=None)
def empties(where):
    """Three cameras; the one at `where` (0, 1, 2) keeps no pixel; where = "all": none does."""
    cams = []
    for k in range(3):
        depth, mask = surface(65, 64, 50 + k)
        if where == "all" or where == k:
            mask[:] = 0
        cams.append(rig_ref.Cam(depth, mask, cam=CAM, T=None if k == 0 else TRANSFORMS["translation"] * np.array([[1, 1, 1, 0.01 * k]])))
    return tuple(cams), LEAF


@functools.lru_cache(maxsize=None)
def overflow():
    """The second camera's transform scales x by 1e42: every pixel off the column j = cx (an integer: xd = 0 exactly there) overflows float and is
    dropped, that column stays."""
    d0, m0 = surface(40, 41, 61, keep=1.0)
    d1, m1 = surface(40, 41, 62, keep=1.0)
    T = np.concatenate([np.diag([1e42, 1.0, 1.0]), np.zeros((3, 1))], axis=1)
    cam = (600.0, 600.0, 20.0, 19.5)
    return (rig_ref.Cam(d0, m0, cam=cam), rig_ref.Cam(d1, m1, cam=cam, T=T)), LEAF


@functools.lru_cache(maxsize=None)
def minus_zero(colour=False):
    """One camera, no transform: a masked pixel with depth 0 left of cx back-projects to (-0.0f, -0.0f, 0.0f); the leaf is small enough for PCL's
    pass-through, which hands the point on as it is."""
    depth, mask = surface(30, 44, 71, keep=0.6)
    depth[3, 2] = 0; mask[3, 2] = 255
    if not colour:
        return (rig_ref.Cam(depth, mask, cam=(600.0, 600.0, 21.5, 14.5)),), 1e-5
    img = paint(mask, 72)
    return (rig_ref.Cam(depth, colour=img, ranges=(*colour_ref.LAUNCH_RANGE, 0), cam=(600.0, 600.0, 21.5, 14.5)),), 1e-5


@functools.lru_cache(maxsize=None)
def border(n):
    """n kept pixels (32 704: the most the one launch serves; 32 705: passed on) spread over two 128 x 128 cameras."""
    cams = []
    left = 2 * 128 * 128 - n                                        # pixels to leave out
    for k in range(2):
        depth, _ = surface(128, 128, 80 + k)
        mask = np.full((128, 128), 255, np.uint8)
        out = left // 2 if k == 0 else left - left // 2
        mask.reshape(-1)[np.random.default_rng(90 + k).choice(128 * 128, out, replace=False)] = 0
        cams.append(rig_ref.Cam(depth, mask, cam=(600.0, 600.0, 63.5, 63.5), T=None if k == 0 else TRANSFORMS["translation"]))
    return tuple(cams), LEAF


@functools.lru_cache(maxsize=None)
def many_tiles(K, cols):
    """K cameras of 1 x cols pixels that share ONE depth plane (every distinct plane is copied once), masks almost empty: each camera keeps its first
    pixel, its last and one of its own."""
    depth = (500 + (np.arange(cols) % 200)).astype(np.uint16).reshape(1, cols)
    cams = []
    for k in range(K):
        mask = np.zeros((1, cols), np.uint8)
        mask[0, [0, cols - 1, (7919 * (k + 1)) % cols]] = 255
        T = np.concatenate([np.eye(3), np.array([[0.0], [0.001 * k], [0.0]])], axis=1)
        cams.append(rig_ref.Cam(depth, mask, cam=(600.0, 600.0, cols / 2, 0.0), T=T))
    return tuple(cams), LEAF


# ---- colour rigs ------------------------------------------------------------------------------------------------------------------------------------------
BLUE, RED, OTHER = (200, 40, 30), (20, 30, 210), (90, 90, 90)     # B, G, R: inside the launch file's blue range / inside "red below 10" / inside neither
RED_RANGE = ([[0, 60, 50]], [[10, 255, 255]])


def paint(mask, seed, on=BLUE):
    """A colour image whose pixels are `on` (with a little noise that stays inside the range) where mask != 0 and grey elsewhere."""
    rng = np.random.default_rng(seed)
    img = np.empty(mask.shape + (3,), np.uint8)
    img[:] = OTHER
    img[mask != 0] = on
    return (img.astype(np.int64) + rng.integers(-8, 9, img.shape)).clip(0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def colour_rig():
    """Two colour cameras: the first segments blue with the launch file's range; the second red, with an occluder image that hides a band of its rope."""
    d0, m0 = surface(40, 50, 91, keep=0.5)
    d1, m1 = surface(40, 50, 92, keep=0.5)
    occ = np.full((40, 50), 255, np.uint8); occ[:, 20:30] = 0
    a = rig_ref.Cam(d0, colour=paint(m0, 93, BLUE), ranges=(*colour_ref.LAUNCH_RANGE, 0), cam=CAM)
    b = rig_ref.Cam(d1, colour=paint(m1, 94, RED), ranges=(*RED_RANGE, 0), occluder=occ, cam=CAM, T=TRANSFORMS["rotation"])
    return (a, b), LEAF


# ---- the binding's cameras ----------------------------------------------------------------------------------------------------------------------------------
def binding_cams(B, cams, place=None):
    """[B.RigCamera] of a scene's cameras; place(array) -> what is handed over for a plane (default: the numpy array itself)."""
    place = place or (lambda a: a)
    out = []
    for c in cams:
        params = None if c.ranges is None else B.make_colour_params(c.ranges[0], c.ranges[1], rgb_order=c.ranges[2])
        out.append(B.RigCamera(place(c.depth), mask=None if c.mask is None else place(c.mask), colour=None if c.colour is None else place(c.colour), params=params,
                               occluder=None if c.occluder is None else place(c.occluder), cam=c.cam, cam_to_rig=c.T))
    return out
