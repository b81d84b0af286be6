"""TEST INFRASTRUCTURE of the consistency-mask tests: the fusion ABI test's scene with outliers, holes, tilted normals and a block mask
put in; the float64 pair test of tests/np_fusion.py as (certainly passing, possibly passing) source counts; the driver of
tests/consistency_host (host/fusion.cpp's ConsistencyMaskHost, the serial twin of dvp_fuse_consistency)."""
import os
import subprocess

import numpy as np

import np_fusion as F
from conftest import ROOT, synth

W, H = 48, 32
PROGRAM = os.path.join(ROOT, "tests", "consistency_host", "consistency_host")
PAIRS = [(0, [1, 2]), (1, [0, 2]), (2, [1, 0]), (0, [1]), (1, []), (0, [1, 2, 1, 2, 0])]


def build_program():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROGRAM)])


def scene():
    sc = synth.make_scene(W, H, 2)
    cams = np.ascontiguousarray(sc["cameras"])
    dep = [np.ascontiguousarray(sc["depth_gt"][v], np.float32).copy() for v in range(3)]
    dep[1][::5, ::7] *= np.float32(1.05)      # outliers: the relative depth test fails
    dep[2][3::6, :] = 0                        # rows without a depth
    dep[0][10:14, 20:30] = 0                   # reference pixels without a depth
    dep[0][0, 0] = -1.0
    nrm = [np.ascontiguousarray(np.tile(sc["normal_gt"].astype(np.float32), (H, W, 1))) for _ in range(3)]
    nrm[2][:, 40:] = np.array([0.0, np.sin(0.3), -np.cos(0.3)], np.float32)   # normals 0.3 rad and more off
    bgr = np.full((H, W, 3), 77, np.uint8)
    block = np.full((H, W), 255, np.uint8)
    block[:, :5] = 127
    block[:, 5:8] = 128
    return dict(cams=cams, dep=dep, nrm=nrm, bgr=bgr, block=block)


def model(sc, ref, src):
    """(certainly passing, possibly passing) source counts per pixel of view `ref`, and the reference pixels, from np_fusion.Pair"""
    views = [F.View(sc["cams"][v]["K"], sc["cams"][v]["R"], sc["cams"][v]["t"], sc["dep"][v], sc["nrm"][v], image_bgr=sc["bgr"],
                    block=sc["block"] if v == 0 else None) for v in range(3)]
    R = views[ref]
    ys, xs, pix = F._ref_pixels(R)
    lo, hi = np.zeros(H * W, np.int64), np.zeros(H * W, np.int64)
    for s in src:
        P = F.Pair(R, views[s], ys, xs)
        with np.errstate(invalid="ignore"):
            sure = [(P.err < 2.0 - F.EPS_PX, P.err >= 2.0 + F.EPS_PX), (P.rel < 0.01 - F.EPS_REL, P.rel >= 0.01 + F.EPS_REL),
                    (P.ang < 0.174533 - P.ang_eps, P.ang >= 0.174533 + P.ang_eps)]
        passes = ~P.round_unc & P.zs_pos & sure[0][0] & sure[1][0] & sure[2][0]
        fails = ~P.round_unc & (~P.zs_pos | sure[0][1] | sure[1][1] | sure[2][1])
        lo[pix] += passes
        hi[pix] += ~fails
    ref_pixel = np.zeros(H * W, bool)
    ref_pixel[pix] = True
    return lo, hi, ref_pixel


def write_scene(sc, path):
    with open(path, "wb") as f:
        f.write(np.int32(3).tobytes())
        for v in range(3):
            f.write(sc["cams"][v].tobytes())
            f.write(np.array([W, H], np.int32).tobytes())
            f.write(sc["dep"][v].tobytes())
            f.write(sc["nrm"][v].tobytes())
            f.write(np.int32(1 if v == 0 else 0).tobytes())
            if v == 0:
                f.write(sc["block"].tobytes())


def twin(sc, ref, src, min_views, tmp):
    """the mask of host/fusion.cpp's ConsistencyMaskHost"""
    path, out = os.path.join(str(tmp), "scene.bin"), os.path.join(str(tmp), "mask.out")
    write_scene(sc, path)
    r = subprocess.run([PROGRAM, path, str(ref), ",".join(map(str, src)) or "-", str(min_views), out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, np.uint8)
