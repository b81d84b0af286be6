"""The preparation in front of `apd --evaluate` on the device: dvp_cloud_prepare equals the serial text of csrc/dvp_cloudprep.hpp
(tests/cloudprep_host) bit for bit on xyz and exactly on first_index and counts over the case table of tests/np_cloudprep.py, every
case twice with equal results; dvp_cloud_evaluate_prepared equals dvp_cloud_evaluate on the host-prepared clouds and the serial text
on d2 bit for bit and on the counts exactly, including crops that keep nothing on one side or on both; the refusals and their
messages; two threads at once."""
import threading

import numpy as np
import pytest

import np_cloudprep as P
import np_evaluate as N
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = P.cases()


@pytest.fixture(scope="module", autouse=True)
def built():
    P.build_program()
    N.build_program()


@pytest.fixture(scope="module")
def capi():
    return pkg("capi")


@pytest.mark.parametrize("case", list(CASES))
def test_prepare_equals_the_serial_text(tmp_path, capi, case):
    xyz, prep = CASES[case]
    rc, err, want = P.serial(xyz, tmp_path, **prep)
    assert rc == 0, err
    got = capi.cloud_prepare(xyz, **prep)
    assert P.same_result(got, want) == ""
    again = capi.cloud_prepare(xyz, **prep)
    assert P.same_result(again, got) == ""
    if case == "transform_identity":
        assert got["xyz"].tobytes() == xyz.tobytes()
    if case == "transform_overflows_one":
        assert got["counts"].tolist() == [70, 69, 69, 69] and 33 not in got["first_index"]


def test_no_option_returns_the_finite_points_bit_for_bit(capi):
    xyz, _ = CASES["non_finite"]
    got = capi.cloud_prepare(xyz)
    ok = np.isfinite(xyz).all(1)
    assert got["xyz"].tobytes() == xyz[ok].tobytes() and got["first_index"].tolist() == np.flatnonzero(ok).tolist() and got["counts"].tolist() == [194] * 4


def evaluate_scene(seed=31, n=6000):
    rng = np.random.default_rng(seed)
    truth = P.cloud(rng.random((n, 3)) * [1.4, 1.4, 1.0] - [0.2, 0.2, 0.0])
    moved = truth[: n - 500] + rng.normal(0, 0.01, (n - 500, 3)).astype(np.float32)
    m = P.rotation(30.0, 10.0, [0.1, -0.05, 0.02]).reshape(4, 4)
    recon = P.cloud((np.linalg.inv(m) @ np.concatenate([moved.astype(np.float64), np.ones((len(moved), 1))], 1).T).T[:, :3])
    recon[7, 1] = np.nan
    truth[11, 0] = np.inf
    crop = P.crop_of(2, 0.1, 0.8, P.polygon_3d(2, P.CONCAVE_12))
    return recon, truth, m.reshape(-1), crop


NOTHING = P.crop_of(2, 50.0, 60.0, P.polygon_3d(2, P.CONCAVE_12))      # a crop that keeps no point of the scene


@pytest.mark.parametrize("which", ["all_options", "crop_only", "voxel_only", "recon_empty", "truth_empty", "both_empty"])
def test_evaluate_prepared_three_ways(tmp_path, capi, which):
    recon, truth, m, crop = evaluate_scene()
    tol = [0.01, 0.02, 0.05]
    pr, pt = {
        "all_options": (P.prep(m, crop, 0.01), P.prep(None, crop, 0.01)), "crop_only": (P.prep(None, crop), P.prep(None, crop)),
        "voxel_only": (P.prep(voxel=0.03), P.prep(voxel=0.03)), "recon_empty": (P.prep(m, NOTHING, 0.01), P.prep(None, crop, 0.01)),
        "truth_empty": (P.prep(m, crop), P.prep(None, NOTHING)), "both_empty": (P.prep(None, NOTHING, 0.01), P.prep(None, NOTHING, 0.01))}[which]
    got = capi.cloud_evaluate_prepared(recon, truth, tol, pr, pt, distances=True)
    # the serial text: both clouds prepared, then evaluated
    (tmp_path / "r").mkdir()
    (tmp_path / "t").mkdir()
    rc, err, hr = P.serial(recon, tmp_path / "r", **pr)
    assert rc == 0, err
    rc, err, ht = P.serial(truth, tmp_path / "t", **pt)
    assert rc == 0, err
    assert np.array_equal(got["counts"], np.stack([hr["counts"], ht["counts"]]))
    assert (hr["counts"][3] == 0) == (which in ("recon_empty", "both_empty")) and (ht["counts"][3] == 0) == (which in ("truth_empty", "both_empty"))
    rc, err, want = N.serial(hr["xyz"], ht["xyz"], tol, tmp_path)
    assert rc == 0, err
    assert N.same_result(got, want) == ""
    # dvp_cloud_evaluate on the host-prepared clouds
    plain = capi.cloud_evaluate(hr["xyz"], ht["xyz"], tol, distances=True)
    assert N.same_result(got, plain) == ""
    if which == "all_options":
        assert 500 < got["used"][0] < len(recon) and got["within_recon"][2] > 0.9 * got["used"][0]      # the transform did bring the clouds together


def test_refusals(capi):
    xyz = P.cloud(np.random.default_rng(1).random((100, 3)))
    square = P.polygon_3d(2, P.BIG_SQUARE)
    bad_row, nan_m = np.eye(4), np.eye(4)
    bad_row[3, 3] = 1.0 + 2.0 ** -52
    nan_m[0, 3] = np.inf
    for prep, say in ((P.prep(transform=bad_row.reshape(-1)), "last row must be 0 0 0 1"), (P.prep(transform=nan_m.reshape(-1)), "non-finite entry"),
                      (P.prep(crop=P.crop_of(2, 0, 1, square[:2])), "at least 3 vertices, got 2"),
                      (P.prep(crop=P.crop_of(2, 0, 1, np.zeros((257, 3)))), "at most 256 vertices, got 257"),
                      (P.prep(crop=P.crop_of(2, 1, 0, square)), "axis_min (1) must not exceed axis_max (0)"), (P.prep(crop=P.crop_of(3, 0, 1, square)), "crop_axis must be"),
                      (P.prep(voxel=-0.5), "voxel must be finite and positive"), (P.prep(voxel=np.nan), "voxel must be finite and positive"),
                      (P.prep(voxel=1e-7), "voxels of edge 1e-07; at most 2097150 are supported")):
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_prepare(xyz, **prep)
        assert "dvp_cloud_prepare: " in str(e.value) and say in str(e.value), (prep, str(e.value))
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_evaluate_prepared(xyz, xyz, [0.1], P.prep(), prep)
        assert "dvp_cloud_evaluate_prepared: " in str(e.value) and say in str(e.value), (prep, str(e.value))
    with pytest.raises(capi.DvpError) as e:
        capi.cloud_evaluate_prepared(xyz, xyz, [0.2, 0.1], P.prep(), P.prep())
    assert "strictly ascending" in str(e.value)
    # null pointers, through the C ABI itself
    L = capi.lib()
    import ctypes
    p, _ = capi._cloud_prep()
    out, counts = np.empty((100, 3), np.float32), np.zeros(4, np.int64)
    for args, say in (((None, 100, ctypes.byref(p), capi._p(out), None, capi._p(counts)), "the point arrays are required"),
                      ((capi._p(xyz), 100, None, capi._p(out), None, capi._p(counts)), "the preparation is required"),
                      ((capi._p(xyz), 100, ctypes.byref(p), None, None, capi._p(counts)), "xyz_out and counts_out are required"),
                      ((capi._p(xyz), 100, ctypes.byref(p), capi._p(out), None, None), "xyz_out and counts_out are required"),
                      ((capi._p(xyz), -1, ctypes.byref(p), capi._p(out), None, capi._p(counts)), "0 ... 2^31 - 1 points, got -1")):
        assert L.dvp_cloud_prepare(0, *args) == 1 and say in L.dvp_cloud_prep_last_error().decode(), say
    p.crop_axis, p.num_polygon = 1, 4
    assert L.dvp_cloud_prepare(0, capi._p(xyz), 100, ctypes.byref(p), capi._p(out), None, capi._p(counts)) == 1 and "the crop polygon is required" in L.dvp_cloud_prep_last_error().decode()
    assert L.dvp_cloud_prepare(0, capi._p(xyz), 100, ctypes.byref(capi._cloud_prep()[0]), capi._p(out), None, capi._p(counts)) == 0 and L.dvp_cloud_prep_last_error() == b""
    assert L.dvp_cloud_evaluate_prepared(0, capi._p(xyz), 100, ctypes.byref(p), capi._p(xyz), 100, ctypes.byref(p), None, 1, None, None, None, None, None, None) == 1
    assert "are required" in L.dvp_cloud_prep_last_error().decode()


def test_out_of_device_memory_is_an_error(capi, monkeypatch):
    xyz, prep = CASES["voxel_shared"]
    monkeypatch.setenv("DVP_TEST_SIDE_ALLOC_FAIL", "1")      # (csrc/dvp_devmem.hpp: every request of a byte or more is refused)
    with pytest.raises(capi.DvpError) as e:
        capi.cloud_prepare(xyz, **prep)
    assert "dvp_cloud_prepare: out of device memory" in str(e.value)
    with pytest.raises(capi.DvpError) as e:
        capi.cloud_evaluate_prepared(xyz, xyz, [0.1], prep, prep)
    assert "dvp_cloud_evaluate_prepared: out of device memory" in str(e.value)
    monkeypatch.delenv("DVP_TEST_SIDE_ALLOC_FAIL")
    assert capi.cloud_prepare(xyz, **prep)["counts"][3] == 1250


def test_two_threads_at_once(tmp_path, capi):
    names = ["combined", "voxel_shared"]
    want = {}
    for n in names:
        (tmp_path / n).mkdir()
        rc, err, want[n] = P.serial(CASES[n][0], tmp_path / n, **CASES[n][1])
        assert rc == 0, err
    got = {n: [] for n in names}

    def work(n):
        for _ in range(4):
            got[n].append(capi.cloud_prepare(CASES[n][0], **CASES[n][1]))
    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for n in names:
        assert len(got[n]) == 4 and all(P.same_result(g, want[n]) == "" for g in got[n])
