"""The device plane prior's arithmetic and its decomposition of the sweep without a GPU: csrc/dvp_prior.hpp + dvp_prior_mid.hpp,
built for the host in tests/prior_host and run one item after the other (a counter sequence per triangle, the owner map, one pass
over the pixels), against the numpy model of np_prior.py — the source's overwriting loops — and the serial planes against the host
mirror's BuildPlanePrior (tests/host/test_host --prior) on a folder written from the same case.  Every comparison is bitwise on
all pixels, NaN == NaN."""
import os
import subprocess

import numpy as np
import pytest

import np_prior as N
from conftest import ROOT

pytestmark = pytest.mark.hostbox


@pytest.mark.parametrize("k", range(len(N.CASES)), ids=N.CASES)
def test_serial_build_equals_the_model_stage_by_stage(k):
    middle, tris, skipped, want = N.expected(k)
    got = N.serial_stages(N.case(k), tris, middle)
    assert got["rows"] == want["rows"]
    assert np.array_equal(got["owner"], want["owner"]), int((got["owner"] != want["owner"]).sum())
    for stage in ("rate", "depth", "planes"):
        assert N.same_bits(got[stage], want[stage]), (stage, N.differing(got[stage], want[stage]))


@pytest.mark.parametrize("k", range(len(N.CASES)), ids=N.CASES)
def test_serial_planes_equal_the_host_mirror(tmp_path, k):
    c = N.case(k)
    middle, tris, skipped, want = N.expected(k)
    d = str(tmp_path / "scene")
    N.write_folder(d, c)
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host")])
    out = subprocess.run([os.path.join(ROOT, "tests", "host", "test_host"), "--prior", d, "0", str(c["W"]), str(c["H"]), str(tmp_path / "planes.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    mirror = np.fromfile(str(tmp_path / "planes.bin"), np.float32).reshape(c["H"], c["W"], 4)
    got = N.serial_stages(c, tris, middle)["planes"]
    assert N.same_bits(got, mirror), N.differing(got, mirror)
    assert N.same_bits(mirror, want["planes"]), N.differing(mirror, want["planes"])


def test_unusable_inputs_give_status_1(tmp_path):
    for c in N.unusable_cases():
        status, middle, tris, skipped = N.serial_triangles(c)
        assert status == 1 and len(tris) == 0, c["name"]


def test_cases_say_what_they_claim():
    """Measured from the model (pixels two triangles gave different values / of those, held by a triangle that was not the first
    to reach them): hand_96x72 162 / 162, aspect_200x100_to_96x72 662 / 662, specials_191x143_to_96x72 2952 / 2952,
    long_400x300 1941 / 1941.  Unvisited pixels enclosed by visited ones: 4, all in specials_191x143_to_96x72 (the sweep's step is
    one over the LONGEST edge, so a swept triangle is sampled densely; the gaps are where triangles were skipped)."""
    counts = {}
    for k, name in enumerate(N.CASES):
        c = N.case(k)
        middle, tris, skipped, m = N.expected(k)
        assert len(tris) >= 4 and m["rows"] == sum(len(N.sequence(s)) for s in tris["step"])
        contested = m["differ"]
        later = contested & (m["owner"] != m["first"])
        counts[name] = (int(contested.sum()), int(later.sum()))
        # unvisited pixels inside the hull: enclosed on all four sides by pixels some triangle reached
        o = m["owner"] >= 0
        left, right = np.maximum.accumulate(o, 1), np.maximum.accumulate(o[:, ::-1], 1)[:, ::-1]
        up, down = np.maximum.accumulate(o, 0), np.maximum.accumulate(o[::-1], 0)[::-1]
        holes = ~o & left & right & up & down
        if k in (0, 2, 3):
            assert contested.sum() > 0 and later.sum() >= 20, (name, counts[name])
        if k == 2:
            assert holes.sum() > 0, name
        assert (m["reached"][~o] == 0).all() and (m["reached"][o] >= 1).all()
    print(counts)
    # 1: a row of more than 64 columns (more than one wave's lanes); 4: more than 256, and a width that is no multiple of 64
    assert max(len(N.sequence(s)) for s in N.expected(0)[1]["step"]) > 64
    assert max(len(N.sequence(s)) for s in N.expected(3)[1]["step"]) > 256 and N.case(3)["raw"].shape[1] % 64 != 0
    # 2: target pixels whose source index lies outside the map keep depth 0, the others do not
    c = N.case(1)
    o_r = (np.arange(c["H"]).astype(np.float32) / (np.float32(c["W"]) / np.float32(c["raw"].shape[1]))).astype(np.int32)
    outside = o_r >= c["raw"].shape[0]
    depth = N.expected(1)[3]["depth"]
    assert outside.any() and not outside.all() and (depth[outside] == 0).all() and (depth[~outside] != 0).all()
    # 3: every skip rule fires; the specials are what they say
    middle, tris, skipped, m = N.expected(2)
    assert (skipped > 0).all(), skipped
    c = N.case(2)
    rows, cols = c["raw"].shape
    xy = c["xy"]
    assert (xy[0] == xy[1]).all() and not (c["xyz"][0] == c["xyz"][1]).all()
    assert len({(int(x), int(y)) for x, y in xy[2:5]}) == 1 and len({(float(x), float(y)) for x, y in xy[2:5]}) == 3
    assert {int(y) for x, y in xy[5:8]} == {40} and len({int(x) for x, y in xy[5:8]}) == 3
    assert xy[8, 0] >= cols and (xy[:, 1].astype(int) == rows - 1).any() and (xy[:, 0].astype(int) == cols - 1).any()
    corners = np.stack([np.concatenate([tris["x1"], tris["x2"], tris["x3"]]), np.concatenate([tris["y1"], tris["y2"], tris["y3"]])], 1)
    assert (corners[:, 1] == rows - 1).any() and (corners[:, 0] == cols - 1).any()
    assert not ((corners[:, 0] == 70) & (corners[:, 1] == 90)).any()          # the point that projects onto column 0 is in no triangle
    assert c["W"] / cols != c["H"] / rows and (cols / c["W"]) % 1 != 0
    # the duplicate's second rate is the one the triangles carry
    at = [(tris["r" + s][(tris["x" + s] == 30) & (tris["y" + s] == 25)]) for s in "123"]
    carried = np.unique(np.concatenate(at))
    cam = N.camera()
    K, R, t = cam["K"].astype(np.float64).reshape(3, 3), cam["R"].astype(np.float64).reshape(3, 3), cam["t"].astype(np.float64)
    z = [(R @ c["xyz"][i].astype(np.float64) + t)[2] for i in (0, 1)]
    want = [(255.0 - float(c["raw"][25, 30])) / zi for zi in z]
    assert len(carried) == 1 and abs(carried[0] - want[1]) < 1e-4 * want[1] and abs(want[0] - want[1]) > 0.1 * want[1]
    # 4: the accumulated counter is not k * step
    middle, tris, skipped, m = N.expected(3)
    step = tris["step"][np.argmax([len(N.sequence(s)) for s in tris["step"]])]
    seq = N.sequence(step)
    assert (seq != (np.arange(len(seq)).astype(np.float32) * np.float32(step))).any()
