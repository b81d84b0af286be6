"""`apd --convert-from ... --undistort on` without a GPU: the text of csrc/dvp_undistort.hpp run serially by
tests/undistort_host/undistort_host, and host/colmap.cpp with the option, against
  * math.atan for the header's own atan;
  * np_undistort: an independent numpy reading of the stage's definition (np.arctan, whole-picture array arithmetic);
  * a byte ramp, which checks where the stage looks without relying on the fixed-point rule;
  * tests/golden/undistort/off: what the converter wrote for the fixture model before the option existed.
The pictures the converter writes go through the device's JPEG encoder and are checked in tests/test_gpu_undistort_driver.py."""
import math
import os
import re
import shutil

import numpy as np
import pytest

import np_convert as N
import np_undistort as U

pytestmark = pytest.mark.hostbox

MODEL = os.path.join(N.GOLDEN, "model")
OFF = os.path.join(U.ROOT, "tests", "golden", "undistort", "off")
NV = 6
# the fixture's two cameras with their fx, fy, cx, cy kept (camera 2 was SIMPLE_RADIAL: f stands for both) and a distortion that moves
# corner pixels by more than a pixel
CAMERAS = {1: (64, 48, [70.25, 69.5, 31.5, 24.25, -0.2, 0.05, 0.004, -0.003]), 2: (60, 44, [66.125, 66.125, 30.0, 22.0, 0.15, -0.03, 0.002, 0.001])}


def test_own_atan_meets_math_atan(tmp_path):
    x = np.concatenate([np.random.default_rng(11).uniform(0, 16, 10000), [0.0, 1e-300, 16.0]])
    got = U.serial_atan(x, tmp_path)
    want = np.array([math.atan(v) for v in x])
    assert got[-3] == 0.0 and got[-2] == 1e-300
    rel = np.abs(got - want) / np.where(want == 0, 1.0, want)
    print("largest relative error of atan_nonneg on [0, 16]: %.3g" % rel.max())
    assert rel.max() <= 1e-13


BYTE_CASES = [(m, w, h, False) for m in U.MODELS for w, h in U.HOST_SIZES] + [(m, 67, 5, True) for m in ("OPENCV", "THIN_PRISM_FISHEYE")]


@pytest.mark.parametrize("model,w,h,pad", BYTE_CASES)
def test_serial_bytes_equal_the_numpy_reading(tmp_path_factory, model, w, h, pad):
    got = U.serial_case(model, w, h, tmp_path_factory, pad)
    want, skip = U.undistort(U.picture(w, h), model, U.params(model, w, h))
    assert skip.sum() <= 0.001 * w * h, skip.sum()                      # decided by the numpy reading alone
    bad = (got != want).any(2) & ~skip
    assert not bad.any(), np.argwhere(bad)[:5]


@pytest.mark.parametrize("model", U.NOT_FISHEYE)
def test_zero_distortion_is_the_identity(tmp_path, model):
    for w, h in ((67, 5), (129, 66)):
        src = U.picture(w, h)
        zeros = [0.0] * len(U.EXTRA[model])
        rc, err, got = U.serial_image(src, model, U.params(model, w, h, zeros), tmp_path)
        assert rc == 0, err
        assert np.array_equal(got, src)


@pytest.mark.parametrize("model", U.MODELS)
def test_geometry_on_a_ramp(tmp_path, model):
    """|out - (alpha sx + beta sy + c)| <= 1 + (alpha + beta) / 64 wherever the source lies inside the picture: 0.5 from the ramp's
    rounding, 0.5 from the output's, half a 1/32-pixel step per axis.  The numpy reading reaches 0.90 of the 1.035."""
    w, h, alpha, beta, c = 67, 5, 1.5, 0.75, 20.0
    src = U.ramp(w, h, alpha, beta, c)
    p = U.params(model, w, h)
    rc, err, got = U.serial_image(src, model, p, tmp_path)
    assert rc == 0, err
    sx, sy = U.source_coordinates(model, p, w, h)
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    assert inside.sum() >= 0.5 * w * h
    err = np.abs(got[:, :, 0].astype(np.float64) - (alpha * sx + beta * sy + c))[inside]
    print("%s: largest departure from the ramp %.3f of %.3f" % (model, err.max(), 1 + (alpha + beta) / 64))
    assert err.max() <= 1 + (alpha + beta) / 64
    assert np.array_equal(got[:, :, 0], got[:, :, 1]) and np.array_equal(got[:, :, 0], got[:, :, 2])


def test_sources_outside_the_picture_read_zero(tmp_path_factory):
    """RADIAL 0.15, -0.03 at 129 x 66 looks past all four edges; a pixel all of whose taps are outside is zero"""
    seen = set()
    for model, w, h in (("RADIAL", 129, 66), ("RADIAL", 300, 7), ("OPENCV", 129, 66)):
        p = U.params(model, w, h)
        sx, sy = U.source_coordinates(model, p, w, h)
        got = U.serial_case(model, w, h, tmp_path_factory)
        edges = {"left": sx < -1.1, "right": sx > w + 0.1, "top": sy < -1.1, "bottom": sy > h + 0.1}
        for name, mask in edges.items():
            if mask.any():
                seen.add(name)
                assert not got[mask].any(), (model, name)
        if (model, w, h) == ("RADIAL", 129, 66):
            outside = (sx < 0) | (sx > w - 1) | (sy < 0) | (sy > h - 1)
            assert outside.mean() >= 0.05 and got[~outside].any()
    assert seen == {"left", "right", "top", "bottom"}


def test_argument_checks(tmp_path):
    src = U.picture(9, 5)
    good = U.params("OPENCV", 9, 5)
    cases = [
        (dict(model="FOV", p=[5.0, 5.0, 4.5, 2.5, 0.9]), "the FOV camera model is not supported"),
        (dict(model=11, p=good), "unknown camera model 11"),
        (dict(model=-1, p=good), "unknown camera model -1"),
        (dict(model="OPENCV", p=good, num_params=7), "OPENCV takes 8 parameters, not 7"),
        (dict(model="SIMPLE_RADIAL", p=good, num_params=8), "SIMPLE_RADIAL takes 4 parameters, not 8"),
        (dict(model="OPENCV", p=good, size=(0, 5)), "bad image geometry (sizes of 1 ... 65535)"),
        (dict(model="OPENCV", p=good, size=(9, 65536)), "bad image geometry (sizes of 1 ... 65535)"),
        (dict(model="OPENCV", p=good, pitch=26), "the pitch is below 3 * width bytes"),
        (dict(model="OPENCV", p=good, null=("in",)), "the picture, the parameters and the output are required"),
        (dict(model="OPENCV", p=good, null=("params",)), "the picture, the parameters and the output are required"),
        (dict(model="OPENCV", p=good, null=("out",)), "the picture, the parameters and the output are required"),
    ]
    for kw, message in cases:
        kw = dict(kw)
        rc, err, _ = U.serial_image(src, kw.pop("model"), kw.pop("p"), tmp_path, **kw)
        assert rc == 1 and message in err, (kw, err)


# ---- through host/colmap.cpp --------------------------------------------------------------------------------------------------
def distorted_source(folder, pictures=True, sizes=None):
    """a COLMAP folder around the fixture model with its cameras rewritten to OPENCV with distortion, and PPM pictures of the
    cameras' sizes; returns {new index: B, G, R pixels}"""
    shutil.copytree(MODEL, os.path.join(folder, "model"))
    with open(os.path.join(folder, "model", "cameras.txt"), "w") as f:
        for cid, (w, h, p) in CAMERAS.items():
            f.write("%d OPENCV %d %d %s\n" % (cid, w, h, " ".join(repr(v) for v in p)))
    _, images, _ = N.read_model(os.path.join(folder, "model"), ".txt")
    pixels = {}
    if pictures:
        os.makedirs(os.path.join(folder, "images"))
        for i, im in enumerate(images):
            w, h = (sizes or {}).get(i, CAMERAS[im[3]][:2])
            bgr = U.picture(w, h, seed=im[0])
            open(os.path.join(folder, "images", im[4]), "wb").write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())
            pixels[i] = bgr
    return pixels


def tree(d):
    out = {}
    for base, _, names in os.walk(d):
        for n in names:
            out[os.path.relpath(os.path.join(base, n), d)] = open(os.path.join(base, n), "rb").read()
    return out


def check_sfm(files, F):
    """the sfm rows of a converted distorted_source against the numpy projection"""
    folder_model = MODEL
    _, images, points = N.read_model(folder_model, ".txt")
    for i, im in enumerate(images):
        fx, fy, cx, cy = CAMERAS[im[3]][2][:4]
        rows = files[os.path.join("sfm", "%08d.txt" % i)].decode().split("\n")
        assert rows[-1] == ""
        rows = rows[:-1]
        want = []
        for pid in im[6]:
            if pid == -1:
                continue
            px, py, zc = U.project(im[1], im[2], points[pid][0], fx, fy, cx, cy, F)
            if zc > 0:
                want.append((px, py, pid))
        assert len(rows) == len(want) > 50, (i, len(rows), len(want))
        for row, (px, py, pid) in zip(rows, want):
            e = row.split(" ")
            # three-term sums, each term rounded once: the bound tests/test_convert_host.py holds the rotation entries to
            assert abs(float(e[0]) - px) <= 1e-15 and abs(float(e[1]) - py) <= 1e-15, (i, row, px, py)
            assert e[0] == repr(float(e[0])) and e[1] == repr(float(e[1]))
            assert " ".join(e[2:]) == "%s %s %s %d %d %d" % (tuple(repr(v) for v in points[pid][0]) + tuple(points[pid][1]))


@pytest.mark.parametrize("F", [1.0, 2.0])
def test_converter_keeps_the_cams_and_projects_the_points(tmp_path, F):
    src = str(tmp_path / "colmap")
    os.makedirs(src)
    distorted_source(src, pictures=False)
    trees = {}
    for how in ("on", "off"):
        out = U.run_program("model", src, str(tmp_path / how), ".txt", how, "no-images", repr(F))
        assert out.returncode == 0, out.stderr
        trees[how] = tree(str(tmp_path / how))
    on, off = trees["on"], trees["off"]
    assert sorted(on) == sorted(off) and len(on) == 1 + 2 * NV
    for name in on:
        if not name.startswith("sfm"):
            assert on[name] == off[name], name                            # the cams already describe the pinhole camera
    assert any(on[name] != off[name] for name in on if name.startswith("sfm"))
    check_sfm(on, F)


def test_off_leaves_the_files_it_left_before(tmp_path):
    src = str(tmp_path / "colmap")
    os.makedirs(src)
    shutil.copytree(MODEL, os.path.join(src, "model"))
    out = U.run_program("model", src, str(tmp_path / "save"), ".txt", "off", "no-images")
    assert out.returncode == 0, out.stderr
    got, want = tree(str(tmp_path / "save")), tree(OFF)
    assert sorted(got) == sorted(want) and len(want) == 1 + 2 * NV
    assert not [k for k in got if got[k] != want[k]]


def test_converter_refuses_what_it_cannot_undistort(tmp_path):
    # a picture whose size is not its camera's: named, and nothing is written
    src = str(tmp_path / "wrong_size")
    os.makedirs(src)
    distorted_source(src, sizes={2: (64, 47)})
    _, images, _ = N.read_model(os.path.join(src, "model"), ".txt")
    out = U.run_program("model", src, str(tmp_path / "a"), ".txt", "on", "images")
    assert out.returncode == 1 and images[2][4] in out.stderr and re.search(r"the picture is 64 x 47, its camera \d+ \d+ x \d+", out.stderr), out.stderr
    assert not os.path.exists(str(tmp_path / "a" / "pair.txt")) and not os.path.exists(str(tmp_path / "a" / "cams"))
    # a FOV camera
    src = str(tmp_path / "fov")
    os.makedirs(src)
    distorted_source(src)
    with open(os.path.join(src, "model", "cameras.txt"), "w") as f:
        f.write("1 FOV 64 48 70.25 69.5 31.5 24.25 0.9\n2 PINHOLE 60 44 66.125 66.125 30.0 22.0\n")
    out = U.run_program("model", src, str(tmp_path / "b"), ".txt", "on", "images")
    assert out.returncode == 1 and "FOV" in out.stderr and "camera 1" in out.stderr, out.stderr
    assert not os.path.exists(str(tmp_path / "b" / "pair.txt"))
    # ... which the converter takes as before without the option
    out = U.run_program("model", src, str(tmp_path / "c"), ".txt", "off", "no-images")
    assert out.returncode == 0, out.stderr
