#!/usr/bin/env python3
"""Fixtures for `apd --convert-from` (tests/golden/convert/): a small synthetic COLMAP model of this tool's own making, as .txt
and .bin, and the pair.txt and cams/ that the reference's converter itself wrote from it.  Runs on a machine that has the
reference's tree and no GPU; never part of a test run.

usage: make_convert_golden.py REFERENCE_DIR            write tests/golden/convert/
       make_convert_golden.py --big OUT_DIR [N [OBS]]  a model of N images x OBS observations (default 1000 x 10000) as .bin under
                                                       OUT_DIR/dslr_calibration_undistorted, with 8 x 8 PPM images; not a fixture
       make_convert_golden.py --time-reference REFERENCE_DIR BIG_DIR [M]
                                                       seconds the reference's calc_score takes on the first M (60) images of BIG_DIR

The model: 6 images with COLMAP ids that are neither 1 .. 6 nor in file order, 2 cameras (PINHOLE, SIMPLE_RADIAL), about 300 points,
-1 entries, one point observed twice in one image, tracks of length 1, 2 and 6, and two cameras 0.01 apart, whose pair the
triangulation-angle rule zeroes.

The reference's processing_single_scene is imported and called unmodified, with two shims: np.asscalar (gone from numpy) supplied as
.item(), and a stand-in cv2 module whose three image functions do the minimum on PPM files.  The stand-in touches image files only,
and no image file becomes a fixture.

The fixtures are refused unless the reference's output cannot depend on numpy's unstable sort, on BLAS summation order or on the
last places of arccos:
  1. every off-diagonal score is positive and distinct within its row, except the zeroed pair;
  2. no two views are tied at the cut of a listed row - except, in the two rows of the zeroed pair, the view itself and its zeroed
     partner (both 0; with n <= 21 views every row lists all but one view, so these two always meet at the cut): there the tool
     checks that the reference listed the higher index, which is what a stable ascending sort read backwards gives;
  3. every angle is at least 1e-6 degrees from 1 (an arccos that differs in the last places moves an angle by about 1e-14 rad);
  4. every %f value is at least 1e-3 of the last digit from a rounding boundary."""
import importlib
import os
import shutil
import struct
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import np_convert as N  # noqa: E402

MODEL_IDS = {"PINHOLE": 1, "SIMPLE_RADIAL": 2}


def look_at(centre, target):
    """world-to-camera rotation as a unit quaternion (w, x, y, z) and the translation t = -R c"""
    z = target - centre
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return q, -R @ centre


def synthetic_model(seed):
    rng = np.random.default_rng(seed)
    cameras = {1: ("PINHOLE", 64, 48, [70.25, 69.5, 31.5, 24.25]), 2: ("SIMPLE_RADIAL", 60, 44, [66.125, 30.0, 22.0, 0.0125])}
    ids = [21, 3, 12, 7, 20, 8]                      # file order; by id: 3 7 8 12 20 21
    xs = {3: -2.0, 7: -1.1, 8: -1.09, 12: 0.2, 20: 1.0, 21: 2.1}      # 7 and 8 are 0.01 apart
    centres = {iid: np.array([xs[iid], 0.1 * rng.normal(), 0.05 * rng.normal()]) for iid in sorted(xs)}
    centres[8] = centres[7] + np.array([0.01, 0.0, 0.0])
    images = []
    for iid in ids:
        q, t = look_at(centres[iid].copy(), np.array([0.0, 0.0, 6.0]) + 0.1 * rng.normal(size=3))
        images.append(dict(id=iid, q=q, t=t, cam=1 if iid % 2 else 2, name="%s%d.ppm" % ("view_" if iid % 3 else "v", iid), obs=[]))
    P = 300
    point_ids = rng.permutation(P) * 3 + 5
    xyz = np.stack([rng.uniform(-2.5, 2.5, P), rng.uniform(-1.5, 1.5, P), rng.uniform(4.5, 8.0, P)], 1)
    rgb = rng.integers(0, 256, (P, 3))
    by_id = {im["id"]: im for im in images}
    seen_p = {3: 0.55, 7: 0.8, 8: 0.7, 12: 0.9, 20: 0.6, 21: 0.45}
    tracks = {}
    for k in range(P):
        if k < 6:
            seen = sorted(by_id)                                    # length 6
        elif k < 14:
            seen = list(rng.choice(sorted(by_id), 2, replace=False))   # length 2
        elif k < 22:
            seen = [int(rng.choice(sorted(by_id)))]                 # length 1
        else:
            seen = [i for i in sorted(by_id) if rng.random() < seen_p[i]]
        tracks[k] = seen
        for i in seen:
            by_id[i]["obs"].append(k)
    by_id[12]["obs"].append(by_id[12]["obs"][3])                    # one point observed twice in one image
    for im in images:
        cam = cameras[im["cam"]]
        fx, fy, cx, cy = (cam[3][0], cam[3][0], cam[3][1], cam[3][2]) if cam[0] == "SIMPLE_RADIAL" else cam[3]
        R = np.array(N.rotation(list(im["q"])))
        rows = []
        for k in im["obs"]:
            pc = R @ xyz[k] + im["t"]
            rows.append((fx * pc[0] / pc[2] + cx + rng.normal(0, 0.3), fy * pc[1] / pc[2] + cy + rng.normal(0, 0.3), int(point_ids[k])))
        for _ in range(int(rng.integers(3, 9))):                    # observations without a point
            rows.append((rng.uniform(0, cam[1]), rng.uniform(0, cam[2]), -1))
        order = rng.permutation(len(rows))
        im["rows"] = [rows[o] for o in order]
    points = [(int(point_ids[k]), xyz[k], rgb[k], tracks[k]) for k in range(P)]
    return cameras, images, points


def write_model(folder, cameras, images, points, text=True):
    os.makedirs(folder, exist_ok=True)
    write_model_binary(folder, cameras, images, points)
    if text:
        write_model_text(folder, cameras, images, points)


def write_model_text(folder, cameras, images, points):
    with open(os.path.join(folder, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, (model, w, h, params) in cameras.items():
            f.write("%d %s %d %d %s\n" % (cid, model, w, h, " ".join(repr(float(p)) for p in params)))
    with open(os.path.join(folder, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for im in images:
            f.write("%d %s %s %d %s\n" % (im["id"], " ".join(repr(float(v)) for v in im["q"]), " ".join(repr(float(v)) for v in im["t"]), im["cam"], im["name"]))
            f.write(" ".join("%s %s %d" % (repr(float(x)), repr(float(y)), p) for x, y, p in im["rows"]) + "\n")
    with open(os.path.join(folder, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, xyz, rgb, track in points:
            f.write("%d %s %d %d %d 0.5 %s\n" % (pid, " ".join(repr(float(v)) for v in xyz), rgb[0], rgb[1], rgb[2], " ".join("%d 0" % i for i in track)))


def write_model_binary(folder, cameras, images, points):
    with open(os.path.join(folder, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for cid, (model, w, h, params) in cameras.items():
            f.write(struct.pack("<iiQQ", cid, MODEL_IDS[model], w, h) + struct.pack("<%dd" % len(params), *params))
    with open(os.path.join(folder, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for im in images:
            f.write(struct.pack("<idddddddi", im["id"], *[float(v) for v in im["q"]], *[float(v) for v in im["t"]], im["cam"]) + im["name"].encode() + b"\0")
            f.write(struct.pack("<Q", len(im["rows"])))
            for x, y, p in im["rows"]:
                f.write(struct.pack("<ddq", float(x), float(y), p))
    with open(os.path.join(folder, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(points)))
        for pid, xyz, rgb, track in points:
            f.write(struct.pack("<QdddBBBd", pid, *[float(v) for v in xyz], int(rgb[0]), int(rgb[1]), int(rgb[2]), 0.5) + struct.pack("<Q", len(track)))
            for i in track:
                f.write(struct.pack("<ii", i, 0))


def write_ppm(file, w, h, seed):
    with open(file, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h) + np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8).tobytes())


def stand_in_cv2():
    """the three functions the reference calls, on PPM files, doing the minimum"""
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST = 0

    def imread(file):
        b = open(file, "rb").read()
        head = b.split(b"\n", 3)
        w, h = [int(v) for v in head[1].split()]
        return np.frombuffer(head[3], np.uint8, w * h * 3).reshape(h, w, 3)[:, :, ::-1]

    def resize(img, size, interpolation=0):
        return img[:size[1], :size[0]]

    def imwrite(file, img):
        open(file, "wb").write(b"")
        return True

    cv2.imread, cv2.resize, cv2.imwrite = imread, resize, imwrite
    return cv2


def load_reference(reference_dir):
    if not hasattr(np, "asscalar"):
        np.asscalar = lambda a: a.item()
    sys.modules["cv2"] = stand_in_cv2()
    sys.path.insert(0, reference_dir)
    sys.dont_write_bytecode = True
    return importlib.import_module("colmap2mvsnet")


def run_reference(ref, dense, save, ext):
    args = types.SimpleNamespace(dense_folder=dense, save_folder=save, max_d=192, interval_scale=1, scale_factor=1, theta0=5, sigma1=1, sigma2=10, model_ext=ext)
    os.makedirs(save, exist_ok=True)
    ref.processing_single_scene(args)
    out = {"pair.txt": open(os.path.join(save, "pair.txt")).read()}
    for name in sorted(os.listdir(os.path.join(save, "cams"))):
        out["cams/" + name] = open(os.path.join(save, "cams", name)).read()
    return out


def check(files, folder):
    cameras, images, points = N.read_model(folder, ".txt")
    m = N.score_inputs(images, points)
    n = len(images)
    score = N.scores(m)
    zeroed = [(i, j) for i in range(n) for j in range(i + 1, n) if score[i, j] == 0]
    assert len(zeroed) == 1, "exactly one pair must be zeroed: %s" % zeroed
    zi, zj = zeroed[0]
    for i in range(n):
        row = [int(score[i, j]) for j in range(n) if j != i and (i, j) not in ((zi, zj), (zj, zi))]
        assert all(v > 0 for v in row) and len(set(row)) == len(row), "condition 1: row %d is %s" % (i, row)
    # condition 2: with condition 1 the only tie is self against the zeroed partner; the reference must have listed the higher index
    rows = files["pair.txt"].split("\n")
    for i, other in ((zi, zj), (zj, zi)):
        listed = [int(v) for v in rows[2 + 2 * i].split()[1::2]]
        assert (max(i, other) in listed) and (min(i, other) not in listed), "condition 2: row %d lists %s" % (i, listed)
    worst = min(float(np.abs(N.pair_angles(m, i, j) - 1).min()) for i in range(n) for j in range(i + 1, n) if N.pair_angles(m, i, j).size)
    assert worst >= 1e-6, "condition 3: an angle is %g degrees from 1" % worst
    # condition 4: the %f values, recomputed here in binary64
    pid = {k: v[0] for k, v in points.items()}
    for i, im in enumerate(images):
        R, t = N.rotation(im[1]), im[2]
        zs = sorted(R[2][0] * pid[p][0] + R[2][1] * pid[p][1] + R[2][2] * pid[p][2] + t[2] for p in im[6] if p != -1)
        dmin, dmax = zs[int(len(zs) * .01)] * 0.75, zs[int(len(zs) * .99)] * 1.25
        for v in (dmin, (dmax - dmin) / 191 / 1, dmax):
            frac = (v * 1e6) % 1.0
            assert abs(frac - 0.5) >= 1e-3, "condition 4: image %d writes %r" % (i, v)
        want = "%f %f %f %f" % (dmin, (dmax - dmin) / 191 / 1, 192, dmax)
        assert files["cams/%08d_cam.txt" % i].split("\n")[11] == want, (files["cams/%08d_cam.txt" % i].split("\n")[11], want)
    assert files["pair.txt"] == N.pair_text(score), "the independent reading disagrees with the reference's pair.txt"
    lengths = sorted(set(len(set(tr)) for tr in [[im[0] for im in images if k in im[6]] for k in points]))
    assert {1, 2, 6} <= set(lengths), lengths
    return score, (zi, zj)


def make_fixtures(reference_dir):
    ref = load_reference(reference_dir)
    for seed in range(1, 200):
        cameras, images, points = synthetic_model(seed)
        with tempfile.TemporaryDirectory() as tmp:
            dense = os.path.join(tmp, "dense")
            folder = os.path.join(dense, "dslr_calibration_undistorted")
            write_model(folder, cameras, images, points)
            os.makedirs(os.path.join(dense, "images"))
            for im in images:
                cam = cameras[im["cam"]]
                write_ppm(os.path.join(dense, "images", im["name"]), cam[1], cam[2], im["id"])
            a = run_reference(ref, dense, os.path.join(tmp, "out_txt"), ".txt")
            b = run_reference(ref, dense, os.path.join(tmp, "out_bin"), ".bin")
            assert a == b, "the reference wrote different files from the .txt and the .bin model"
            try:
                score, zeroed = check(a, folder)
            except AssertionError as e:
                print("seed %d refused: %s" % (seed, e))
                continue
            dst = os.path.join(ROOT, "tests", "golden", "convert")
            os.makedirs(os.path.join(dst, "cams"), exist_ok=True)
            os.makedirs(os.path.join(dst, "model"), exist_ok=True)
            for name in os.listdir(folder):
                shutil.copyfile(os.path.join(folder, name), os.path.join(dst, "model", name))
            for name, text in a.items():
                open(os.path.join(dst, name), "w").write(text)
            print("seed %d: fixtures written to %s; zeroed pair %s; scores\n%s" % (seed, dst, zeroed, score))
            return 0
    print("no seed gave a model that meets the conditions")
    return 1


def big_arrays(n_images, n_obs):
    """N images on an arc, each seeing the n_obs points nearest to it along the arc (with jitter): neighbours share most of their
    lists, far pairs little.  Returns (centres (N, 3), xyz (P, 3), [the point indices image i sees], tracks)"""
    rng = np.random.default_rng(7)
    P = n_obs * n_images // 8
    ang = np.linspace(0, 2.0, n_images)
    centres = np.stack([6 * np.sin(ang), 0.05 * rng.normal(size=n_images), 6 - 6 * np.cos(ang)], 1)
    xyz = np.stack([rng.uniform(-3, 3, P), rng.uniform(-2, 2, P), rng.uniform(4, 8, P)], 1)
    home = rng.uniform(0, n_images, P)                       # the image around which a point is seen
    width = 6.0 * n_obs * n_images / P / 2                   # a window that holds about 1.5 n_obs candidates
    seen, tracks = [], [[] for _ in range(P)]
    for i in range(n_images):
        cand = np.nonzero(np.abs(home - i) < width)[0]
        near = cand[np.argsort(np.abs(home[cand] - i) + rng.uniform(0, width / 2, cand.size))[:n_obs]]
        seen.append(near)
        for k in near:
            tracks[k].append(i + 1)
    return centres, xyz, seen, tracks


def big(out, n_images, n_obs):
    centres, xyz, seen, tracks = big_arrays(n_images, n_obs)
    rng = np.random.default_rng(8)
    cameras = {1: ("PINHOLE", 8, 8, [8.0, 8.0, 4.0, 4.0])}
    images = []
    for i in range(n_images):
        q, t = look_at(centres[i].copy(), np.array([0.0, 0.0, 6.0]))
        rows = [(float(x), float(y), int(k) + 1) for (x, y), k in zip(rng.uniform(0, 8, (len(seen[i]), 2)), seen[i])]
        images.append(dict(id=i + 1, q=q, t=t, cam=1, name="%d.ppm" % (i + 1), rows=rows))
    points = [(k + 1, xyz[k], (128, 128, 128), tracks[k]) for k in range(len(xyz))]
    write_model(os.path.join(out, "dslr_calibration_undistorted"), cameras, images, points, text=False)
    os.makedirs(os.path.join(out, "images"), exist_ok=True)
    for im in images:
        write_ppm(os.path.join(out, "images", im["name"]), 8, 8, im["id"])
    print("%d images x %d observations, %d points, sum of squared track lengths %d" % (n_images, n_obs, len(xyz), sum(len(t) ** 2 for t in tracks)))
    return 0


def time_reference(reference_dir, big_dir, m):
    ref = load_reference(reference_dir)
    cameras, images, points3d = ref.read_model(os.path.join(big_dir, "dslr_calibration_undistorted"), ".bin")
    images = {i + 1: images[k] for i, k in enumerate(sorted(images)[:m])}
    extrinsic = {}
    for k, im in images.items():
        e = np.zeros((4, 4))
        e[:3, :3] = ref.qvec2rotmat(im.qvec)
        e[:3, 3] = im.tvec
        e[3, 3] = 1
        extrinsic[k] = e
    t0 = time.time()
    for i in range(m):
        for j in range(i + 1, m):
            ref.calc_score((i, j), images, points3d, extrinsic, None)
    dt = time.time() - t0
    print("reference calc_score, %d images (%d pairs), one process: %.1f s = %.1f ms per pair" % (m, m * (m - 1) // 2, dt, 1e3 * dt / (m * (m - 1) // 2)))
    return 0


if __name__ == "__main__":
    a = sys.argv[1:]
    if len(a) >= 2 and a[0] == "--big":
        sys.exit(big(a[1], int(a[2]) if len(a) > 2 else 1000, int(a[3]) if len(a) > 3 else 10000))
    if len(a) >= 3 and a[0] == "--time-reference":
        sys.exit(time_reference(a[1], a[2], int(a[3]) if len(a) > 3 else 60))
    if len(a) == 1:
        sys.exit(make_fixtures(a[0]))
    print(__doc__)
    sys.exit(2)
