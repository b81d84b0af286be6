#!/usr/bin/env python3
"""The ground-truth cloud of a tools/make_dataset.py folder: every pixel of depth_gt.npy with a positive finite depth, back-projected
through its view's cams/%08d_cam.txt, as <folder>/gt.ply (binary little-endian, float x y z) - what `apd --evaluate
<folder>/APD/APD.ply --against <folder>/gt.ply` scores a fused cloud against.  numpy only.
usage: gt_cloud.py FOLDER [OUT.ply]"""
import os
import sys

import numpy as np


def read_cam(path):
    """(R (3, 3), t (3,), K (3, 3)) of a cam file: `extrinsic` 4 x 4, `intrinsic` 3 x 3"""
    words = open(path).read().split()
    e = words.index("extrinsic")
    i = words.index("intrinsic")
    E = np.array(words[e + 1:e + 17], np.float64).reshape(4, 4)
    K = np.array(words[i + 1:i + 10], np.float64).reshape(3, 3)
    return E[:3, :3], E[:3, 3], K


def back_project(depth, R, t, K):
    """(N, 3) float64 world points of the pixels with a positive finite depth: X = R^T (Z K^-1 (x, y, 1) - t), pixel centres at integers"""
    H, W = depth.shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    Z = depth.astype(np.float64)
    keep = np.isfinite(Z) & (Z > 0)
    cam = np.stack([Z * (xx - K[0, 2]) / K[0, 0], Z * (yy - K[1, 2]) / K[1, 1], Z], -1)[keep]
    return (cam - t) @ R      # rows of R^T (cam - t)


def write_ply(path, xyz):
    xyz = np.ascontiguousarray(xyz, "<f4")
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(xyz)).encode())
        f.write(xyz.tobytes())


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    folder = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) == 3 else os.path.join(folder, "gt.ply")
    depth = np.load(os.path.join(folder, "depth_gt.npy"))
    clouds = [back_project(depth[v], *read_cam(os.path.join(folder, "cams", "%08d_cam.txt" % v))) for v in range(len(depth))]
    xyz = np.concatenate(clouds) if clouds else np.zeros((0, 3))
    write_ply(out, xyz)
    print("%s: %d points from %d views" % (out, len(xyz), len(depth)))


if __name__ == "__main__":
    main()
