"""`apd --convert-from`: the fixture COLMAP model (tests/golden/convert) with PPM and with JPEG inputs of two sizes, converted
under --convert-on host and gpu: both leave the same bytes; pair.txt and the cams meet the files the reference's converter wrote;
every written JPEG is dvp_jpeg_encode of the padded, resampled input and decodes to the set's size; `apd` then runs on the folder
to APD.ply, with the plane prior from the written sfm/ once a dep/ is there; an unknown --convert-on value is a usage error; and
the driver's first form still leaves its files."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import np_convert as N
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

APD = os.path.join(ROOT, "dvp-mvs_amd", "apd")
MODEL = os.path.join(N.GOLDEN, "model")
NV = 6
_MADE = {}


def smooth_picture(w, h, seed):
    """something a JPEG keeps: low-frequency colour with a little texture"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [128 + 90 * np.sin(xx / (5.0 + c) + seed) * np.cos(yy / (7.0 - c)) + rng.normal(0, 6, (h, w)) for c in range(3)]
    return np.clip(np.stack(planes, 2), 0, 255).astype(np.uint8)


def rename(d, old, new):
    """an image name of the same length in both formats of the model (in images.bin the name ends with a zero byte)"""
    for name, tail in (("images.txt", b"\n"), ("images.bin", b"\0")):
        f = os.path.join(d, "model", name)
        data = open(f, "rb").read()
        assert old + tail in data and len(old) == len(new)
        open(f, "wb").write(data.replace(old + tail, new + tail))


def source(tmp_path_factory, kind):
    """a COLMAP folder around the fixture model: images/ as binary PPM (names as the model has them) or as baseline JPEG (the
    model's names rewritten to .jpg), 64 x 48 for camera 1 and 60 x 44 for camera 2; returns (folder, {new index: B, G, R pixels})"""
    if kind not in _MADE:
        capi = pkg().get_capi()
        d = str(tmp_path_factory.mktemp("colmap_" + kind))
        shutil.copytree(MODEL, os.path.join(d, "model"))
        if kind == "jpg":
            rename(d, b".ppm", b".jpg")
        cameras, images, _ = N.read_model(os.path.join(d, "model"), ".txt")
        os.makedirs(os.path.join(d, "images"))
        pixels = {}
        for i, im in enumerate(images):
            w, h = (64, 48) if im[3] == 1 else (60, 44)
            bgr = smooth_picture(w, h, im[0])
            file = os.path.join(d, "images", im[4])
            if kind == "jpg":
                data = capi.jpeg_encode(bgr, 90)
                open(file, "wb").write(bytes(data))
                pixels[i] = capi.jpeg_decode(bytes(data), 3)
            elif i == 0:      # one grey input: replicated to three channels, as cv::imread does
                grey = np.ascontiguousarray(bgr[:, :, 1])
                file = file[:-4] + ".pgm"
                rename(d, im[4].encode(), im[4][:-4].encode() + b".pgm")
                open(file, "wb").write(b"P5\n%d %d\n255\n" % (w, h) + grey.tobytes())
                pixels[i] = np.repeat(grey[:, :, None], 3, 2)
            else:
                open(file, "wb").write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())
                pixels[i] = bgr
        _MADE[kind] = (d, pixels)
    return _MADE[kind]


def convert(src, save, *extra):
    return subprocess.run([APD, "--convert-from", src, save, "--model-dir", "model"] + list(extra), capture_output=True, text=True, timeout=300)


def tree(d):
    out = {}
    for base, _, names in os.walk(d):
        for n in names:
            out[os.path.relpath(os.path.join(base, n), d)] = open(os.path.join(base, n), "rb").read()
    return out


@pytest.mark.parametrize("kind,F", [("ppm", 1.0), ("jpg", 1.0), ("jpg", 2.0), ("ppm", 1.5)])
def test_host_and_gpu_leave_the_same_folder(tmp_path, tmp_path_factory, kind, F):
    capi = pkg().get_capi()
    src, pixels = source(tmp_path_factory, kind)
    trees = {}
    for where in ("host", "gpu"):
        save = str(tmp_path / where)
        out = convert(src, save, "--convert-on", where, "--scale-factor", repr(F))
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        assert ("on the device" if where == "gpu" else "on the host") in out.stdout
        trees[where] = tree(save)
    a, b = trees["host"], trees["gpu"]
    want_names = ["pair.txt"] + [os.path.join(sub, "%08d%s" % (i, tail)) for i in range(NV) for sub, tail in (("cams", "_cam.txt"), ("images", ".jpg"), ("sfm", ".txt"))]
    assert sorted(a) == sorted(b) == sorted(want_names)
    assert not [k for k in a if a[k] != b[k]]
    assert a["pair.txt"].decode() == open(os.path.join(N.GOLDEN, "pair.txt")).read()
    for i in range(NV):
        got = N.parse_cam(a[os.path.join("cams", "%08d_cam.txt" % i)].decode())
        want = N.parse_cam(open(os.path.join(N.GOLDEN, "cams", "%08d_cam.txt" % i)).read())
        if F == 1.0:
            assert got[1] == want[1] and got[2] == want[2]
        for r in range(3):
            assert got[0][r][3:] == want[0][r][3:]
            assert all(abs(float(got[0][r][c]) - float(want[0][r][c])) <= 1e-15 for c in range(3))
    out_w, out_h = N.out_size(64, 48, F)
    for i in range(NV):
        file = a[os.path.join("images", "%08d.jpg" % i)]
        expected = N.convert_image(pixels[i], 64, 48, out_w, out_h)
        assert file == bytes(capi.jpeg_encode(expected, 95)), i
        assert capi.jpeg_size(file, 3) == (out_w, out_h) and capi.jpeg_decode(file, 3).shape == (out_h, out_w, 3)


def test_sfm_off_and_nothing_else_is_deleted(tmp_path, tmp_path_factory):
    src, _ = source(tmp_path_factory, "ppm")
    save = str(tmp_path / "save")
    os.makedirs(os.path.join(save, "images"))
    os.makedirs(os.path.join(save, "cams"))
    for keep in (os.path.join("images", "00000099.jpg"), os.path.join("cams", "notes.txt"), "pair.txt"):
        open(os.path.join(save, keep), "w").write("kept")
    out = convert(src, save, "--sfm", "off", "--model-ext", ".bin")
    assert out.returncode == 0, out.stderr
    t = tree(save)
    assert t[os.path.join("images", "00000099.jpg")] == b"kept" and t[os.path.join("cams", "notes.txt")] == b"kept"      # the script's rmtree is not copied
    assert t["pair.txt"].decode() == open(os.path.join(N.GOLDEN, "pair.txt")).read() and not any(k.startswith("sfm") for k in t)


def test_apd_runs_on_the_converted_folder(tmp_path, tmp_path_factory):
    src, _ = source(tmp_path_factory, "jpg")
    save = str(tmp_path / "save")
    assert convert(src, save).returncode == 0

    def run():
        out = subprocess.run([APD, save, "0", "--iters", "1", "--passes", "1", "--min-scale", "1"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        assert os.path.exists(os.path.join(save, "APD", "APD.ply"))
        return out.stdout

    log = run()
    assert "There are 6 problems" in log and "Plane prior from dep/ and sfm/" not in log
    # a dep/ by tools/make_dataset.py's recipe (255 - s * depth as a BinMat), for a fronto-parallel wall 6 units away
    os.makedirs(os.path.join(save, "dep"))
    yy, xx = np.mgrid[0:48, 0:64].astype(np.float32)
    raw = (255.0 - 25.0 * (1.0 + 0.08 * xx / 64 - 0.05 * yy / 48) * 6.0).astype(np.float32)
    for i in range(NV):
        with open(os.path.join(save, "dep", "%08d.dmb" % i), "wb") as f:
            f.write(np.array([1, 48, 64, 5], np.int32).tobytes() + raw.tobytes())
    shutil.rmtree(os.path.join(save, "APD"))
    assert run().count("Plane prior from dep/ and sfm/") >= 1


def test_unusable_inputs_are_errors_that_name_the_file(tmp_path, tmp_path_factory):
    src, _ = source(tmp_path_factory, "ppm")
    d = str(tmp_path / "colmap")
    shutil.copytree(src, d)
    victim = sorted(n for n in os.listdir(os.path.join(d, "images")) if n.endswith(".ppm"))[0]
    os.remove(os.path.join(d, "images", victim))
    out = convert(d, str(tmp_path / "a"))
    assert out.returncode == 1 and victim in out.stderr and not os.path.exists(str(tmp_path / "a" / "pair.txt"))
    open(os.path.join(d, "images", victim), "wb").write(b"\x89PNG\r\n\x1a\n" + b"\0" * 64)
    out = convert(d, str(tmp_path / "b"))
    assert out.returncode == 1 and victim in out.stderr
    # a progressive JPEG: the decoder rejects it, on the host and on the device
    src_j, _ = source(tmp_path_factory, "jpg")
    dj = str(tmp_path / "colmap_jpg")
    shutil.copytree(src_j, dj)
    victim = sorted(os.listdir(os.path.join(dj, "images")))[0]
    data = open(os.path.join(dj, "images", victim), "rb").read()
    at = data.index(b"\xff\xc0")
    open(os.path.join(dj, "images", victim), "wb").write(data[:at] + b"\xff\xc2" + data[at + 2:])
    for where in ("host", "gpu"):
        out = convert(dj, str(tmp_path / ("c_" + where)), "--convert-on", where)
        assert out.returncode == 1 and victim in out.stderr, out.stderr


def test_an_unknown_value_is_a_usage_error(tmp_path, tmp_path_factory):
    src, _ = source(tmp_path_factory, "ppm")
    save = str(tmp_path / "save")
    out = convert(src, save, "--convert-on", "device")
    assert out.returncode == 1 and "--convert-on takes gpu or host" in out.stderr and not os.path.exists(os.path.join(save, "pair.txt"))
    out = subprocess.run([APD, "--convert-from", src], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "USAGE: apd --convert-from" in out.stderr


def test_the_first_form_still_leaves_its_files(tmp_path):
    """tests/test_gpu_jpeg_decode_driver.py's invocation, unchanged"""
    d = str(tmp_path / "data")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, "128", "96", "3", "2", "--jpg"], stdout=subprocess.DEVNULL, timeout=300)
    out = subprocess.run([APD, d, "0", "--iters", "2", "--passes", "1", "--min-scale", "1", "--seed", "7"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    t = tree(os.path.join(d, "APD"))
    for kind in ("depths.dmb", "APD_normals.dmb", "weak.bin", "selected_views.bin"):
        assert sum(k.endswith(kind) for k in t) == 3, (kind, sorted(t))
    assert "APD.ply" in t and "There are 3 problems" in out.stdout
