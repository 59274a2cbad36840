#!/usr/bin/env python3
"""Generates tests/golden/proto_sort_pts.npz by IMPORTING the reference's numpy prototype (utils/tracking_test.py) the way make_golden.py does --
its ROS / OpenCV / Open3D imports replaced by empty stub modules -- and calling its `sort_pts` (:174-229).  Nothing of the prototype is stored:
only the inputs and what it returned.

Per case k: in_k [M x 3] the nodes as given, out_k [M x 3] what the prototype's sort_pts returned, coord_k [M] the cumulative segment lengths of
out_k formed as the prototype's first-frame block forms them (:531-537: numpy's own row sums of the squared differences, a square root, then a
serial running sum).  The cases are tests/init_ref.py's scenes of up to 64 nodes, shuffled ropes of 2 .. 64 nodes, random clouds and lattice
points in random order (equal distances) -- all with pairwise distinct nodes and distances well below the prototype's `minimum = 999999`, where
it and utils.cpp:95-170 (`INFINITY`) are the same rule.

Run:  python tests/golden/make_init_golden.py        (needs the reference tree; writes next to this file)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import load_prototype  # noqa: E402
import init_ref as R  # noqa: E402


def cases():
    out = [(n, R.scenes()[n]) for n in R.small_scene_names() if len(R.scenes()[n]) <= 64 and n != "underflow"]
    rng = np.random.default_rng(17)
    for i, M in enumerate([2, 3, 4, 5, 7, 9, 12, 16, 20, 25, 33, 40, 48, 64]):
        Y, _ = R._shuffled(R._curve(M, 300 + i, jitter=0.3), int(rng.integers(0, M)), 400 + i)
        out.append((f"rope_{M}", Y))
    for i, M in enumerate([2, 3, 5, 8, 13, 21, 34, 55]):
        out.append((f"random_{M}", rng.uniform(-0.5, 0.5, (M, 3))))
    g = np.arange(4) * 0.03125
    L = np.array([[x, y, z] for x in g for y in g for z in g])
    for i, M in enumerate([6, 11, 27, 40, 64]):
        out.append((f"lattice_{M}", L[rng.permutation(64)[:M]].copy()))
    return out


def main():
    proto = load_prototype()
    data = {}
    names = []
    for name, Y in cases():
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        S = np.asarray(proto.sort_pts(Y.copy()), dtype=np.float64)
        seg = np.sqrt(np.sum(np.square(np.diff(S, axis=0)), axis=1))
        coord = [0.0]
        for i in range(1, len(S)):
            coord.append(coord[-1] + seg[i - 1])
        assert S.shape == Y.shape
        names.append(name)
        data[f"in_{name}"] = Y; data[f"out_{name}"] = S; data[f"coord_{name}"] = np.array(coord)
    path = os.path.join(HERE, "proto_sort_pts.npz")
    np.savez_compressed(path, names=np.array(names), **data)
    print("wrote", path, len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
