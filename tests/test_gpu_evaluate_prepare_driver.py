"""`apd --evaluate` with the preparation options end to end, on the synthetic scene of tests/test_gpu_evaluate_driver.py, built the
same way: --transform, --crop and --voxel-size leave the same report bytes on gpu and on host; --save-prepared writes two clouds whose
plain --evaluate prints the same table; a reconstruction moved by a rigid matrix and given the inverse as --transform scores the same
on both flavours and, at the coarse tolerances, as the unmoved one; without the options the report has the form it always had."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import np_cloudprep as P
import np_evaluate as N
from conftest import ROOT

pytestmark = pytest.mark.gpu

APD = os.path.join(ROOT, "dvp-mvs_amd", "apd")
TEST_HOST = os.path.join(ROOT, "tests", "host", "test_host")


def vertex_count(ply):
    return int(open(ply, "rb").read(400).decode("latin1").split("element vertex ")[1].split("\n")[0])


def apd_evaluate(*args):
    return subprocess.run([APD, "--evaluate"] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    W, H, NV = 96, 64, 5
    d = str(tmp_path_factory.mktemp("evaluate_prepare") / "scene")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, str(W), str(H), str(NV), "4"], stdout=subprocess.DEVNULL)
    gt = np.load(os.path.join(d, "depth_gt.npy"))

    def write_binmat(path, a, typ):
        with open(path, "wb") as f:
            f.write(np.array([1, a.shape[0], a.shape[1], typ], np.int32).tobytes())
            f.write(np.ascontiguousarray(a).tobytes())
    n = np.array([0.25, 0.1, -1.0])
    n /= np.linalg.norm(n)
    for v in range(NV):
        r = os.path.join(d, "APD", "%08d" % v)
        os.makedirs(r, exist_ok=True)
        write_binmat(os.path.join(r, "depths.dmb"), gt[v].astype(np.float32), 5)
        write_binmat(os.path.join(r, "APD_normals.dmb"), np.tile(n.astype(np.float32), (H, W, 1)), 21)
        write_binmat(os.path.join(r, "weak.bin"), np.ones((H, W), np.uint8), 0)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host")])
    out = subprocess.run(["timeout", "-k", "10", "300", TEST_HOST, "--fuse", d], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-500:]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gt_cloud.py"), d], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    recon, truth = os.path.join(d, "APD", "APD.ply"), os.path.join(d, "gt.ply")
    # a crop around the middle of the ground truth: the 12-gon of the case table over the central 80 % in x and y, the central 90 % in z
    N.build_program()
    rc, err, xyz = N.read_ply(truth, tmp_path_factory.mktemp("read"))
    assert rc == 0, err
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    poly = (lo[:2] + 0.1 * (hi[:2] - lo[:2])) + np.array(P.CONCAVE_12) * 0.8 * (hi[:2] - lo[:2])
    crop = os.path.join(d, "crop.json")
    with open(crop, "w") as f:
        json.dump({"class_name": "SelectionPolygonVolume", "orthogonal_axis": "Z", "axis_min": float(lo[2] + 0.05 * (hi[2] - lo[2])), "axis_max": float(hi[2] - 0.05 * (hi[2] - lo[2])),
                   "bounding_polygon": [[float(u), float(v), 0.0] for u, v in poly], "version_major": 1, "version_minor": 0}, f, indent=1)
    return recon, truth, d, crop


def moved_scene(scene, tmp_path):
    """the reconstruction moved by a rigid matrix, and the file of the inverse"""
    recon, truth, d, crop = scene
    rc, err, xyz = N.read_ply(recon, tmp_path)
    assert rc == 0, err
    m = P.rotation(25.0, -15.0, [3.0, -2.0, 1.5]).reshape(4, 4)
    moved = (m @ np.concatenate([xyz.astype(np.float64), np.ones((len(xyz), 1))], 1).T).T[:, :3]
    ply, trans = str(tmp_path / "moved.ply"), str(tmp_path / "inverse.txt")
    N.write_ply_like_apd(ply, moved)
    np.savetxt(trans, np.linalg.inv(m))
    return ply, trans


def test_options_leave_the_same_report_on_device_and_host(scene, tmp_path):
    recon, truth, d, crop = scene
    ply, trans = moved_scene(scene, tmp_path)
    options = ["--transform", trans, "--crop", crop, "--voxel-size", "0.02"]
    dev = apd_evaluate(ply, "--against", truth, "--evaluate-on", "gpu", "--out", tmp_path / "gpu.txt", *options)
    assert dev.returncode == 0, dev.stderr
    host = apd_evaluate(ply, "--against", truth, "--evaluate-on", "host", "--out", tmp_path / "host.txt", *options)
    assert host.returncode == 0, host.stderr
    assert dev.stdout == host.stdout and open(tmp_path / "gpu.txt", "rb").read() == open(tmp_path / "host.txt", "rb").read() == dev.stdout.encode()
    lines = dev.stdout.splitlines()
    assert len(lines) == 11 and lines[4] == "tolerance accuracy completeness f1"
    words = [ln.replace(",", "").split() for ln in lines[:4]]
    # prepared <name>: <finite> finite, <inside> in the crop volume, <out> points; the first two lines count the prepared points
    assert words[2][:2] == ["prepared", "reconstruction:"] and words[3][:2] == ["prepared", "ground_truth:"]
    assert words[2][3:4] + words[2][5:9] + words[2][10:] == ["finite", "in", "the", "crop", "volume", "points"]
    fin_r, in_r, out_r, fin_t, in_t, out_t = (int(words[k][j]) for k in (2, 3) for j in (2, 4, 9))
    assert fin_r == vertex_count(recon) and fin_t == vertex_count(truth) and 100 < out_r <= in_r < fin_r and 100 < out_t <= in_t < fin_t and out_r + out_t < in_r + in_t
    assert lines[0] == "reconstruction %s %d points (0 skipped)" % (ply, out_r) and lines[1] == "ground_truth %s %d points (0 skipped)" % (truth, out_t)
    # each option alone, too
    for one in (options[0:2], options[2:4], options[4:6]):
        a, b = apd_evaluate(ply, "--against", truth, "--evaluate-on", "gpu", *one), apd_evaluate(ply, "--against", truth, "--evaluate-on", "host", *one)
        assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) == 11, (one, a.stderr, b.stderr)
    print("\n" + dev.stdout)


def test_saved_prepared_clouds_score_the_same(scene, tmp_path):
    recon, truth, d, crop = scene
    prefix = str(tmp_path / "prep_")
    tables = []
    for where in ("gpu", "host"):
        out = apd_evaluate(recon, "--against", truth, "--evaluate-on", where, "--crop", crop, "--voxel-size", "0.02", "--save-prepared", prefix + where + "_")
        assert out.returncode == 0, out.stderr
        saved = [prefix + where + "_recon.ply", prefix + where + "_truth.ply"]
        lines = out.stdout.splitlines()
        assert lines[2].endswith(", %d points" % vertex_count(saved[0])) and lines[3].endswith(", %d points" % vertex_count(saved[1]))
        assert open(saved[0], "rb").read(200).startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % vertex_count(saved[0]))
        plain = apd_evaluate(saved[0], "--against", saved[1], "--evaluate-on", where)
        assert plain.returncode == 0, plain.stderr
        assert plain.stdout.splitlines()[2:] == lines[4:] and len(lines) == 11
        tables.append(lines[2:])
    assert tables[0] == tables[1]
    assert open(prefix + "gpu_recon.ply", "rb").read() == open(prefix + "host_recon.ply", "rb").read()
    assert open(prefix + "gpu_truth.ply", "rb").read() == open(prefix + "host_truth.ply", "rb").read()


def test_a_moved_reconstruction_and_the_inverse_matrix(scene, tmp_path):
    recon, truth, d, crop = scene
    ply, trans = moved_scene(scene, tmp_path)
    dev = apd_evaluate(ply, "--against", truth, "--evaluate-on", "gpu", "--transform", trans)
    host = apd_evaluate(ply, "--against", truth, "--evaluate-on", "host", "--transform", trans)
    assert dev.returncode == 0 and host.returncode == 0, dev.stderr + host.stderr
    assert dev.stdout == host.stdout
    unmoved = apd_evaluate(recon, "--against", truth, "--evaluate-on", "host")
    wrong = apd_evaluate(ply, "--against", truth, "--evaluate-on", "gpu")
    assert unmoved.returncode == 0 and wrong.returncode == 0
    figures = lambda text, first: np.array([[float(v) for v in ln.split()[1:]] for ln in text.splitlines()[first:]])
    # Moving and moving back changes a coordinate of this scene (magnitude below 16) by a few binary32 roundings, under 1e-5.  From
    # 0.05 up that is 2e-4 of the tolerance: a figure changes by a tenth of a point only if more than one point in a thousand has
    # its nearest neighbour that close to the tolerance.
    a, b = figures(dev.stdout, 5), figures(unmoved.stdout, 3)
    assert a.shape == b.shape == (6, 3) and np.abs(a[2:] - b[2:]).max() < 0.1, (a, b)
    assert (figures(wrong.stdout, 3)[:3, 2] < a[:3, 2]).all()      # without the matrix the frames do not meet


def test_without_the_options_the_report_is_the_old_one(scene):
    recon, truth, d, crop = scene
    dev, host = apd_evaluate(recon, "--against", truth, "--evaluate-on", "gpu"), apd_evaluate(recon, "--against", truth, "--evaluate-on", "host")
    assert dev.returncode == 0 and dev.stdout == host.stdout and "prepared" not in dev.stdout
    lines = dev.stdout.splitlines()
    assert lines[0] == "reconstruction %s %d points (0 skipped)" % (recon, vertex_count(recon))
    assert lines[1] == "ground_truth %s %d points (0 skipped)" % (truth, vertex_count(truth))
    assert lines[2] == "tolerance accuracy completeness f1" and len(lines) == 9
    # and it is what dvp_cloud_evaluate counts: the figures again from the library's counts
    rc, err, r = N.read_ply(recon, os.path.dirname(crop))
    rc2, err2, t = N.read_ply(truth, os.path.dirname(crop))
    assert rc == 0 and rc2 == 0
    from conftest import pkg
    got = pkg("capi").cloud_evaluate(r, t, N.DEFAULT_TOLERANCES)
    for k, ln in enumerate(lines[3:]):
        a, c = got["within_recon"][k] / got["used"][0], got["within_truth"][k] / got["used"][1]
        f = 0.0 if a + c == 0 else 2 * a * c / (a + c)
        assert ln == "%.9g %.6f %.6f %.6f" % (float(np.float32(N.DEFAULT_TOLERANCES[k])), 100 * a, 100 * c, 100 * f)
