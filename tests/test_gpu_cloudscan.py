"""The observed-space accuracy of `apd --evaluate --against-scans` on the device: dvp_cloud_scan_gaps and dvp_cloud_evaluate_scans equal
the serial text of csrc/dvp_cloudscan.hpp (tests/cloudscan_host) - maps, truth points, gaps, distances and prepared clouds bit for bit,
the counts exactly - over the case table of tests/np_cloudscan.py (one point, no point, 63 ... 129 points and queries in one texel, the
axes, face diagonals and corners at cube sizes 16, 64 and 1 024, the clamp, negative zero, the void pairs, 64 scans, a transform some
1e4 away), at the thresholds, on the room, on random scans twice and with a preparation, from two threads at once; the refusals carry
their messages, and out of device memory is an error."""
import threading

import numpy as np
import pytest

import np_cloudprep as P
import np_cloudscan as S
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = S.cases()
TOLERANCES = [0.05, 0.1, 0.5]


@pytest.fixture(scope="module", autouse=True)
def built():
    S.build_program()


@pytest.fixture(scope="module")
def capi():
    return pkg("capi")


@pytest.fixture(scope="module")
def random_serial(tmp_path_factory):
    """the random scans, and the serial text's gaps and evaluation of them, computed once"""
    scans, queries = S.random_case()
    tmp = tmp_path_factory.mktemp("random")
    out = dict(scans=scans, queries=queries)
    for R in (64, 1024):
        rc, err, out["gaps_%d" % R] = S.serial_gaps(scans, queries, R, tmp)
        assert rc == 0, err
    rc, err, out["evaluation"] = S.serial_evaluate(queries, scans, TOLERANCES, 64, tmp)
    assert rc == 0, err
    return out


def device_gaps(capi, scans, queries, R):
    got = capi.cloud_scan_gaps(scans, queries, R, maps=True, truth=True)
    got["maps"] = got["maps"].reshape(len(scans), -1)
    return got


@pytest.mark.parametrize("case", list(CASES))
def test_gaps_equal_the_serial_text(capi, tmp_path, case):
    c = CASES[case]
    rc, err, want = S.serial_gaps(c["scans"], c["queries"], c["R"], tmp_path)
    assert rc == 0, err
    assert S.same_gaps(device_gaps(capi, c["scans"], c["queries"], c["R"]), want) == ""


@pytest.mark.parametrize("R", [16, 64, 1024])
def test_one_texel_under_contention_at_every_cube_size(capi, tmp_path, R):
    """129 returns along one ray: one atomicMin target whatever the cube size; every output may be left out"""
    c = CASES["one_texel_129"]
    rc, err, want = S.serial_gaps(c["scans"], c["queries"], R, tmp_path)
    assert rc == 0, err
    got = device_gaps(capi, c["scans"], c["queries"], R)
    assert S.same_gaps(got, want) == "" and np.isfinite(got["maps"]).sum() == 1
    assert capi.cloud_scan_gaps(c["scans"], c["queries"], R)["gap"].tobytes() == want["gap"].tobytes()


def test_the_thresholds(capi, tmp_path):
    for T, free, accurate in ((S.THRESHOLD, [1, 0], [0, 0]), (S.ACCURATE_FIRST, [1, 1], [1, 1])):
        rc, err, want = S.serial_evaluate(T["recon"], T["scans"], T["tolerances"], T["R"], tmp_path)
        assert rc == 0, err
        got = capi.cloud_evaluate_scans(T["recon"], T["scans"], T["tolerances"], cube_size=T["R"], distances=True)
        assert S.same_evaluation(got, want) == ""
        assert got["free_space"].tolist() == free and got["within_recon"].tolist() == accurate
    assert capi.cloud_evaluate_scans(S.THRESHOLD["recon"], S.THRESHOLD["scans"], S.THRESHOLD["tolerances"], cube_size=16, distances=True)["gap"].tolist() == [0.4375]


def test_the_room(capi, tmp_path):
    room = S.room()
    rc, err, want = S.serial_evaluate(room["recon"], room["scans"], S.ROOM_TOLERANCES, S.ROOM_R, tmp_path)
    assert rc == 0, err
    got = capi.cloud_evaluate_scans(room["recon"], room["scans"], S.ROOM_TOLERANCES, cube_size=S.ROOM_R, distances=True)
    assert S.same_evaluation(got, want) == ""
    assert got["free_space"].tolist() == [2000] * 3 and got["within_recon"].tolist() == [3000] * 3 and got["unobserved"].tolist() == [2000] * 3
    assert got["accuracy"].tolist() == [3000 / 5000] * 3
    scans, behind = S.plate_scene()
    alone, both = (capi.cloud_evaluate_scans(behind, s, [0.1, 0.2], cube_size=S.ROOM_R) for s in (scans[:1], scans))
    assert alone["free_space"].tolist() == [0, 0] and alone["unobserved"].tolist() == [50, 50] and both["free_space"].tolist() == [50, 50]


@pytest.mark.parametrize("R", [64, 1024])
def test_random_scans_twice(capi, random_serial, R):
    want = random_serial["gaps_%d" % R]
    for _ in range(2):
        assert S.same_gaps(device_gaps(capi, random_serial["scans"], random_serial["queries"], R), want) == ""


def test_random_scans_evaluated(capi, random_serial, tmp_path):
    scans, queries = random_serial["scans"], random_serial["queries"]
    for _ in range(2):
        got = capi.cloud_evaluate_scans(queries, scans, TOLERANCES, cube_size=64, distances=True)
        assert S.same_evaluation(got, random_serial["evaluation"]) == ""
    prep_recon, prep_truth = P.prep(P.rotation(1.0, -0.5, [0.01, 0.02, -0.01]), None, 0.05), P.prep(None, P.crop_of(2, -3.0, 3.0, P.polygon_3d(2, P.BIG_SQUARE)), 0.05)
    rc, err, want = S.serial_evaluate(queries, scans, TOLERANCES, 64, tmp_path, prep_recon, prep_truth)
    assert rc == 0, err
    got = capi.cloud_evaluate_scans(queries, scans, TOLERANCES, prep_recon, prep_truth, cube_size=64, distances=True)
    assert S.same_evaluation(got, want) == "" and got["counts"][1, 3] < got["counts"][1, 0]
    # no reconstructed point at all; a scan without points among others
    empty = capi.cloud_evaluate_scans(np.zeros((0, 3)), scans, TOLERANCES, cube_size=64, distances=True)
    assert empty["used"][0] == 0 and empty["free_space"].tolist() == [0, 0, 0] and len(empty["gap"]) == 0 and empty["accuracy"].tolist() == [0, 0, 0]
    holed = [scans[0], S.scan(np.zeros((0, 3)), scans[1][1]), scans[2]]
    rc, err, want = S.serial_evaluate(queries, holed, TOLERANCES, 64, tmp_path)
    assert rc == 0 and S.same_evaluation(capi.cloud_evaluate_scans(queries, holed, TOLERANCES, cube_size=64, distances=True), want) == ""


def test_two_threads_at_once(capi, random_serial):
    got = {"gaps": [], "evaluation": []}

    def work(n):
        for _ in range(3):
            if n == "gaps":
                got[n].append(device_gaps(capi, random_serial["scans"], random_serial["queries"], 64))
            else:
                got[n].append(capi.cloud_evaluate_scans(random_serial["queries"], random_serial["scans"], TOLERANCES, cube_size=64, distances=True))
    threads = [threading.Thread(target=work, args=(n,)) for n in got]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(got["gaps"]) == 3 and all(S.same_gaps(g, random_serial["gaps_64"]) == "" for g in got["gaps"])
    assert len(got["evaluation"]) == 3 and all(S.same_evaluation(g, random_serial["evaluation"]) == "" for g in got["evaluation"])


def test_refusals(capi):
    x = [[1, 0, 0]]
    bad_row, nan_m = np.eye(4), np.eye(4)
    bad_row[3, 1] = 1e-300
    nan_m[0, 3] = np.nan
    for scans, R, say in (([S.scan(x)], 24, "cube_size must be a power of two, 16 ... 4096, got 24"), ([S.scan(x)], 8, "got 8"), ([S.scan(x)], 8192, "got 8192"),
                          ([S.scan(x)], 0, "got 0"), ([S.scan(x)], -16, "got -16"), ([], 16, "num_scans must be 1 ... 64, got 0"), ([S.scan(x)] * 65, 16, "num_scans must be 1 ... 64, got 65"),
                          ([S.scan(x), S.scan(x, bad_row)], 16, "scan 1: the transform's last row must be 0 0 0 1"),
                          ([S.scan(x, nan_m)], 16, "scan 0: the transform holds a non-finite entry"), ([S.scan(x) + (-1,)], 16, "scan 0: a scan holds 0 or more points, got -1")):
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_scan_gaps(scans, x, R)
        assert "dvp_cloud_scan_gaps: " in str(e.value) and say in str(e.value), (say, str(e.value))
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_evaluate_scans(x, scans, [0.1], cube_size=R)
        assert "dvp_cloud_evaluate_scans: " in str(e.value) and say in str(e.value), (say, str(e.value))
    for kw, say in ((dict(tolerances=[0.2, 0.1]), "strictly ascending"), (dict(tolerances=[]), "num_tol must be 1 ... 8, got 0"),
                    (dict(tolerances=[0.1], prep_recon=P.prep(voxel=-1.0)), "voxel must be finite and positive"),
                    (dict(tolerances=[0.1], prep_truth=P.prep(transform=bad_row.reshape(-1))), "last row must be 0 0 0 1")):
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_evaluate_scans(x, [S.scan(x)], cube_size=16, **kw)
        assert say in str(e.value), (say, str(e.value))
    assert capi.cloud_scan_gaps([S.scan(x)] * 64, x, 16)["gap"].tolist() == [0.0]      # 64 scans are taken: the point is its own return, range 1


def test_out_of_device_memory_is_an_error(capi, monkeypatch):
    c = CASES["one_texel_65"]
    monkeypatch.setenv("DVP_TEST_SIDE_ALLOC_FAIL", "1")      # (csrc/dvp_devmem.hpp: every request of a byte or more is refused)
    with pytest.raises(capi.DvpError) as e:
        capi.cloud_scan_gaps(c["scans"], c["queries"], 16)
    assert "dvp_cloud_scan_gaps: out of device memory" in str(e.value)
    with pytest.raises(capi.DvpError) as e:
        capi.cloud_evaluate_scans(c["queries"], c["scans"], [0.1], cube_size=16)
    assert "dvp_cloud_evaluate_scans: out of device memory" in str(e.value)
    monkeypatch.delenv("DVP_TEST_SIDE_ALLOC_FAIL")
    assert np.isfinite(capi.cloud_scan_gaps(c["scans"], c["queries"], 16)["gap"]).all()
