"""`apd --evaluate` end to end on a synthetic scene: a 96 x 64, five-view tools/make_dataset.py folder with the true maps as results
(as test_boundary.test_fusion_cpu has them) is fused by the RunFusion of libdvp_host.so - the one `apd` calls after its last pass -
through tests/host/test_host --fuse, as that test does (`apd` itself has no fusion-only mode), tools/gt_cloud.py makes its
ground-truth cloud, and
the sub-command scores one against the other.  --evaluate-on gpu and host leave the same report bytes; the used counts are the files'
vertex counts; a cloud against itself scores 100 everywhere and against its shifted copy 0 at the first tolerance and 100 from the
second on, on the device; an unknown --evaluate-on value is a usage error.  The figures of the scene are printed (pytest -s) and not
gated on: DESIGN.md, "Cloud evaluation", quotes them."""
import os
import subprocess
import sys

import numpy as np
import pytest

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
    d = str(tmp_path_factory.mktemp("evaluate") / "scene")
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
    return os.path.join(d, "APD", "APD.ply"), os.path.join(d, "gt.ply"), d


def test_device_and_host_leave_the_same_report(scene):
    recon, truth, d = scene
    dev = apd_evaluate(recon, "--against", truth, "--evaluate-on", "gpu", "--out", os.path.join(d, "gpu.txt"))
    assert dev.returncode == 0, dev.stderr
    host = apd_evaluate(recon, "--against", truth, "--evaluate-on", "host", "--out", os.path.join(d, "host.txt"))
    assert host.returncode == 0, host.stderr
    assert dev.stdout == host.stdout and open(os.path.join(d, "gpu.txt"), "rb").read() == open(os.path.join(d, "host.txt"), "rb").read() == dev.stdout.encode()
    assert apd_evaluate(recon, "--against", truth).stdout == dev.stdout      # the device is the default
    lines = dev.stdout.splitlines()
    assert lines[0] == "reconstruction %s %d points (0 skipped)" % (recon, vertex_count(recon))
    assert lines[1] == "ground_truth %s %d points (0 skipped)" % (truth, vertex_count(truth))
    assert vertex_count(truth) == 5 * 96 * 64 and lines[2] == "tolerance accuracy completeness f1" and len(lines) == 9
    figures = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[3:]])
    assert (np.diff(figures, axis=0) >= 0).all()
    print("\n" + dev.stdout)


def test_self_and_shifted_on_the_device(scene, tmp_path):
    recon, _, _ = scene
    out = apd_evaluate(recon, "--against", recon, "--evaluate-on", "gpu")
    assert out.returncode == 0, out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()[3:]]
    assert len(rows) == 6 and all(r[1:] == ["100.000000"] * 3 for r in rows), rows
    # Points at least 0.01 apart (a point is dropped when an earlier one is nearer), shifted by 1.5 x 0.0025 along z: a point's own
    # copy is 0.00375 away, every other copy at least 0.00625, and binary32 coordinates of this size round by less than 1e-6
    rc, err, xyz = N.read_ply(recon, tmp_path)
    assert rc == 0, err
    x64 = xyz.astype(np.float64)
    drop = np.zeros(len(xyz), bool)
    for first in range(0, len(xyz), 256):
        near = np.linalg.norm(x64[first:first + 256, None, :] - x64[None, :, :], axis=2) < 0.01
        drop[first:first + 256] = (near & (np.arange(len(xyz))[None, :] < np.arange(first, min(first + 256, len(xyz)))[:, None])).any(1)
    thin = xyz[~drop]
    assert len(thin) > 1000 and np.abs(thin).max() < 16
    a, b = str(tmp_path / "thin.ply"), str(tmp_path / "shifted.ply")
    N.write_ply_like_apd(a, thin)
    N.write_ply_like_apd(b, thin + np.float32([0, 0, 0.00375]))
    for where in ("gpu", "host"):
        out = apd_evaluate(a, "--against", b, "--evaluate-on", where, "--tolerances", "0.0025,0.005,0.02")
        assert out.returncode == 0, out.stderr
        rows = [ln.split() for ln in out.stdout.splitlines()[3:]]
        assert rows[0][1:] == ["0.000000"] * 3 and all(r[1:] == ["100.000000"] * 3 for r in rows[1:]), (where, rows)


def test_unknown_flavour_is_a_usage_error(scene):
    recon, truth, _ = scene
    out = apd_evaluate(recon, "--against", truth, "--evaluate-on", "cuda")
    assert out.returncode == 1 and "--evaluate-on takes gpu or host" in out.stderr and out.stdout == ""
