"""The alignment refinement of `apd --evaluate` on the device: dvp_cloud_icp_step equals the serial text of csrc/dvp_cloudicp.hpp
(tests/cloudicp_host) bit for bit on e and the sums and exactly on nearest and the count over the case table of tests/np_cloudicp.py,
in both search forms and both neighbourhoods, every case twice with equal results; dvp_cloud_refine_alignment equals `cloudicp_host
refine` bit for bit on the matrix and exactly on the log; the recovered motion against a float64 numpy ICP; the accuracy the refined
matrix buys; a stage that ends without correspondences; the refusals and their messages; two threads at once."""
import ctypes
import threading

import numpy as np
import pytest

import np_cloudicp as C
import np_cloudprep as P
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = C.cases()
FORMS = [("wave", "125"), ("lane", "125"), ("wave", "27"), ("lane", "27")]


@pytest.fixture(scope="module", autouse=True)
def built():
    C.build_program()


@pytest.fixture(scope="module")
def capi():
    return pkg("capi")


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    """the serial text's result of a case, computed once"""
    known = {}

    def of(name):
        if name not in known:
            c = CASES[name]
            rc, err, res = C.serial_step(c["src"], c["tgt"], tmp_path_factory.mktemp("step"), c["D"], c["d"])
            assert rc == 0, err
            known[name] = res
        return known[name]
    return of


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the refinement scene and, per crop, the serial text's matrix and log"""
    recon, truth, known, initial, crop = C.refine_scene()
    want = {}
    for name, cr in (("whole", None), ("cropped", crop)):
        rc, err, want[name] = C.serial_refine(recon, truth, tmp_path_factory.mktemp("refine"), initial, cr, C.STAGES)
        assert rc == 0, err
    return dict(recon=recon, truth=truth, known=known, initial=initial, crop={"whole": None, "cropped": crop}, want=want)


@pytest.mark.parametrize("form,cells", FORMS)
@pytest.mark.parametrize("case", list(CASES))
def test_step_equals_the_serial_text(capi, serial, monkeypatch, case, form, cells):
    monkeypatch.setenv("DVP_CLOUD_QUERY", form)
    monkeypatch.setenv("DVP_CLOUD_ICP_CELLS", cells)
    c, want = CASES[case], serial(case)
    got = capi.cloud_icp_step(c["src"], c["tgt"], c["d"], c["D"])
    assert C.same_step(got, want) == ""
    again = capi.cloud_icp_step(c["src"], c["tgt"], c["d"], c["D"])
    assert C.same_step(again, got) == ""
    if case == "exactly_two":
        assert got["count"] == 2 and np.flatnonzero(got["nearest"] >= 0).tolist() == [3, 8]
    if case == "equidistant_other_cells":
        assert got["nearest"].tolist() == [1, 3] and got["e"][0] == got["e"][1] == np.float32(0.09375) ** 2
    if case == "equidistant_other_chunks":
        assert (got["nearest"] < 64).all()
    if case.startswith("target_at_d"):
        assert got["count"] == 1 and got["e"][0] == np.float32(c["d"]) * np.float32(c["d"])
    if case.startswith("target_ulp_beyond_d"):
        assert got["count"] == 0 and got["nearest"][0] == -1 and np.isposinf(got["e"][0])
    if case == "non_finite_sources":
        assert (got["nearest"][[0, 63, 64, 127, 128, 199]] == -1).all() and got["count"] == 194
    if case == "image_overflows_binary32":
        assert got["nearest"][33] == -1 and got["count"] == 69
    if case == "negative_zero_2":
        assert np.signbit(got["sums"][6:15]).all() and not np.signbit(got["sums"][0:3]).any()


def test_the_cases_reach_every_cell_of_both_neighbourhoods():
    assert len(C.cell_offsets(CASES["every_cell_27"], 1)) == 27 and len(C.cell_offsets(CASES["every_cell_125"], 2)) == 125


def test_no_increment_is_the_identity(capi):
    c = CASES["tree_alternate_65"]
    assert C.same_step(capi.cloud_icp_step(c["src"], c["tgt"], c["d"], None), capi.cloud_icp_step(c["src"], c["tgt"], c["d"], np.eye(4))) == ""


@pytest.mark.parametrize("form,cells", [("wave", "125"), ("lane", "27")])
@pytest.mark.parametrize("which", ["whole", "cropped"])
def test_refine_equals_the_serial_text(capi, scene, monkeypatch, which, form, cells):
    monkeypatch.setenv("DVP_CLOUD_QUERY", form)
    monkeypatch.setenv("DVP_CLOUD_ICP_CELLS", cells)
    want = scene["want"][which]
    got = capi.cloud_refine_alignment(scene["recon"], scene["truth"], C.STAGES, scene["initial"], scene["crop"][which])
    assert got["matrix"].tobytes() == want["matrix"].tobytes(), (C.hexes(got["matrix"]), C.hexes(want["matrix"]))
    assert len(got["log"]) == len(want["log"]) and all(g[:4] == w[:4] and float(g[4]).hex() == float(w[4]).hex() for g, w in zip(got["log"], want["log"])), (got["log"], want["log"])
    assert {g[0] for g in got["log"]} == {0, 1, 2} and got["matrix"][12:].tolist() == [0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("which", ["whole", "cropped"])
def test_the_motion_is_recovered_as_well_as_in_float64(capi, scene, which):
    """at most twice the float64 numpy ICP's rotation and translation errors: the factor allows for the binary32 search"""
    crop = scene["crop"][which]
    got = capi.cloud_refine_alignment(scene["recon"], scene["truth"], C.STAGES, scene["initial"], crop)
    mine = C.motion_errors(got["matrix"], scene["known"])
    theirs = C.motion_errors(C.float64_icp(scene["recon"], scene["truth"], scene["initial"], crop, C.STAGES), scene["known"])
    start = C.motion_errors(scene["initial"], scene["known"])
    print("\n%s: start %.6f deg %.6f; device %.6f deg %.6f; float64 numpy %.6f deg %.6f" % ((which,) + start + mine + theirs))
    assert mine[0] <= 2.0 * theirs[0] and mine[1] <= 2.0 * theirs[1]
    assert mine[0] < start[0] and mine[1] < start[1]


def test_the_refined_matrix_raises_the_accuracy(capi, scene):
    tol = [0.01, 0.02, 0.05]
    got = capi.cloud_refine_alignment(scene["recon"], scene["truth"], C.STAGES, scene["initial"])
    rough = capi.cloud_evaluate_prepared(scene["recon"], scene["truth"], tol, P.prep(scene["initial"]), P.prep())
    fine = capi.cloud_evaluate_prepared(scene["recon"], scene["truth"], tol, P.prep(got["matrix"]), P.prep())
    assert fine["accuracy"][0] > rough["accuracy"][0] and fine["completeness"][0] > rough["completeness"][0]


def test_a_stage_without_correspondences_ends_and_keeps_the_matrix(capi, scene):
    away = np.eye(4)
    away[:3, 3] = [100.0, 0.0, 0.0]
    got = capi.cloud_refine_alignment(scene["recon"], scene["truth"], [(0.05, 0.1, 20), (0.0, 0.1, 5)], away.reshape(-1))
    assert got["matrix"].tobytes() == away.reshape(-1).tobytes()
    assert [g[:2] for g in got["log"]] == [(0, 1), (1, 1)] and all(g[3] == 0 and g[4] == 0.0 and g[2] > 0 for g in got["log"])
    # exactly two correspondences end it as well
    two = capi.cloud_refine_alignment(scene["truth"][[20, 30]] + np.float32(0.001), scene["truth"][:100], [(0.0, 0.01, 20)])
    assert two["matrix"].tobytes() == np.eye(4).tobytes() and [g[:4] for g in two["log"]] == [(0, 1, 2, 2)]


def test_refusals(capi, monkeypatch):
    rng = np.random.default_rng(2)
    xyz = P.cloud(rng.random((100, 3)))
    bad_row, nan_m = np.eye(4), np.eye(4)
    bad_row[3, 0] = 1e-300
    nan_m[1, 1] = np.nan
    holed = xyz.copy()
    holed[5, 2] = np.nan
    for args, say in (((xyz, xyz, 0.1, bad_row), "the increment's last row must be 0 0 0 1"), ((xyz, xyz, 0.1, nan_m), "the increment holds a non-finite entry"),
                      ((xyz, xyz, 0.0), "max_distance (0) must be finite and positive"), ((xyz, xyz, -1.0), "must be finite and positive"),
                      ((xyz, xyz, np.inf), "must be finite and positive"), ((xyz, xyz, np.nan), "must be finite and positive"), ((xyz, xyz, 1e-20), "normal binary32 square"),
                      ((xyz, xyz, 1e30), "normal binary32 square"), ((xyz, holed, 0.1), "the targets must have finite coordinates, 1 of 100 have not"),
                      ((xyz, [[0, 0, 0], [1e6, 0, 0]], 1e-3), "at most 2097150 are supported")):
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_icp_step(*args)
        assert "dvp_cloud_icp_step: " in str(e.value) and say in str(e.value), (say, str(e.value))
    square = P.polygon_3d(2, P.BIG_SQUARE)
    for kw, say in ((dict(stages=[]), "num_stages must be 1 ... 8, got 0"), (dict(stages=[(0, 0.1, 1)] * 9), "num_stages must be 1 ... 8, got 9"),
                    (dict(stages=[(-0.1, 0.1, 1)]), "stage 0: voxel must be finite and positive"), (dict(stages=[(0, 0.1, 1), (np.nan, 0.1, 1)]), "stage 1: voxel must be finite and positive"),
                    (dict(stages=[(0, 0.0, 1)]), "stage 0: max_distance (0) must be finite and positive"), (dict(stages=[(0, 1e-30, 1)]), "normal binary32 square"),
                    (dict(stages=[(0, 0.1, 0)]), "max_iterations must be 1 ... 1000, got 0"), (dict(stages=[(0, 0.1, 1001)]), "max_iterations must be 1 ... 1000, got 1001"),
                    (dict(stages=[(0, 0.1, 1)], transform=bad_row), "last row must be 0 0 0 1"), (dict(stages=[(0, 0.1, 1)], transform=nan_m), "non-finite entry"),
                    (dict(stages=[(0, 0.1, 1)], crop=P.crop_of(2, 0, 1, square[:2])), "at least 3 vertices, got 2"),
                    (dict(stages=[(0, 0.1, 1)], crop=P.crop_of(2, 1, 0, square)), "axis_min (1) must not exceed axis_max (0)"),
                    (dict(stages=[(1e-7, 0.1, 1)]), "voxels of edge 1e-07; at most 2097150 are supported")):
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_refine_alignment(xyz, xyz, **kw)
        assert "dvp_cloud_refine_alignment: " in str(e.value) and say in str(e.value), (say, str(e.value))
    # null pointers and counts, through the C ABI itself
    L = capi.lib()
    sums, count, out, n = np.zeros(16), np.zeros(1, np.int64), np.zeros(16), ctypes.c_int(0)
    for args, say in (((None, 100, capi._p(xyz), 100, None, 0.1, None, None, capi._p(sums), capi._p(count)), "the point arrays are required"),
                      ((capi._p(xyz), 100, None, 100, None, 0.1, None, None, capi._p(sums), capi._p(count)), "the point arrays are required"),
                      ((capi._p(xyz), 100, capi._p(xyz), 100, None, 0.1, None, None, None, capi._p(count)), "sums_out and count_out are required"),
                      ((capi._p(xyz), 100, capi._p(xyz), 100, None, 0.1, None, None, capi._p(sums), None), "sums_out and count_out are required"),
                      ((capi._p(xyz), -1, capi._p(xyz), 100, None, 0.1, None, None, capi._p(sums), capi._p(count)), "0 ... 2^31 - 1 points, got -1")):
        assert L.dvp_cloud_icp_step(0, *args) == 1 and say in L.dvp_cloud_icp_last_error().decode(), say
    stage = capi.DvpIcpStage(0.0, 0.1, 1)
    log = (capi.DvpIcpLog * 4)()
    # more than 2^30 sources: refused in the wave form before a point is read (its table keeps a source's slot in 32 bits)
    many = 2 ** 30 + 1
    assert L.dvp_cloud_icp_step(0, capi._p(xyz), many, capi._p(xyz), 100, None, 0.1, None, None, capi._p(sums), capi._p(count)) == 1
    assert "orders at most 1073741824 (2^30) sources, got 1073741825" in L.dvp_cloud_icp_last_error().decode()
    assert L.dvp_cloud_refine_alignment(0, capi._p(xyz), many, capi._p(xyz), 100, None, None, ctypes.byref(stage), 1, capi._p(out), log, 4, ctypes.byref(n)) == 1
    assert "orders at most 1073741824 (2^30) sources" in L.dvp_cloud_icp_last_error().decode()
    for args, say in (((None, 100, capi._p(xyz), 100, None, None, ctypes.byref(stage), 1, capi._p(out), log, 4, ctypes.byref(n)), "the point arrays are required"),
                      ((capi._p(xyz), 100, capi._p(xyz), 100, None, None, None, 1, capi._p(out), log, 4, ctypes.byref(n)), "are required"),
                      ((capi._p(xyz), 100, capi._p(xyz), 100, None, None, ctypes.byref(stage), 1, None, log, 4, ctypes.byref(n)), "are required"),
                      ((capi._p(xyz), 100, capi._p(xyz), 100, None, None, ctypes.byref(stage), 1, capi._p(out), None, 4, ctypes.byref(n)), "are required"),
                      ((capi._p(xyz), 100, capi._p(xyz), 100, None, None, ctypes.byref(stage), 1, capi._p(out), log, 4, None), "are required")):
        assert L.dvp_cloud_refine_alignment(0, *args) == 1 and say in L.dvp_cloud_icp_last_error().decode(), say
    # no description at all: identity, no crop; a success clears the error
    assert L.dvp_cloud_refine_alignment(0, capi._p(xyz), 100, capi._p(xyz), 100, None, None, ctypes.byref(stage), 1, capi._p(out), log, 4, ctypes.byref(n)) == 0
    assert L.dvp_cloud_icp_last_error() == b"" and n.value == 1 and (log[0].n_src, log[0].n, log[0].rmse) == (100, 100, 0.0) and out.tolist() == np.eye(4).reshape(-1).tolist()
    for name, value, say in (("DVP_CLOUD_QUERY", "both", "DVP_CLOUD_QUERY takes wave or lane"), ("DVP_CLOUD_ICP_CELLS", "64", "DVP_CLOUD_ICP_CELLS takes 27 or 125")):
        monkeypatch.setenv(name, value)
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_icp_step(xyz, xyz, 0.1)
        assert say in str(e.value)
        with pytest.raises(capi.DvpError) as e:
            capi.cloud_refine_alignment(xyz, xyz, [(0, 0.1, 1)])
        assert say in str(e.value)
        monkeypatch.delenv(name)


def test_out_of_device_memory_is_an_error(capi, monkeypatch):
    c = CASES["random_3000"]
    monkeypatch.setenv("DVP_TEST_SIDE_ALLOC_FAIL", "1")      # (csrc/dvp_devmem.hpp: every request of a byte or more is refused)
    with pytest.raises(capi.DvpError) as e:
        capi.cloud_icp_step(c["src"], c["tgt"], c["d"])
    assert "dvp_cloud_icp_step: out of device memory" in str(e.value)
    with pytest.raises(capi.DvpError) as e:
        capi.cloud_refine_alignment(c["src"], c["tgt"], [(0.0, 0.05, 2)])
    assert "dvp_cloud_refine_alignment: out of device memory" in str(e.value)
    monkeypatch.delenv("DVP_TEST_SIDE_ALLOC_FAIL")
    assert capi.cloud_icp_step(c["src"], c["tgt"], c["d"])["count"] == 2294


def test_two_threads_at_once(capi, serial, scene):
    names = ["random_3000", "near_1e4"]
    got = {n: [] for n in names + ["refine"]}

    def work(n):
        for _ in range(3):
            if n == "refine":
                got[n].append(capi.cloud_refine_alignment(scene["recon"], scene["truth"], C.STAGES, scene["initial"], scene["crop"]["cropped"]))
            else:
                got[n].append(capi.cloud_icp_step(CASES[n]["src"], CASES[n]["tgt"], CASES[n]["d"], CASES[n]["D"]))
    threads = [threading.Thread(target=work, args=(n,)) for n in got]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for n in names:
        assert len(got[n]) == 3 and all(C.same_step(g, serial(n)) == "" for g in got[n])
    want = scene["want"]["cropped"]
    assert len(got["refine"]) == 3 and all(g["matrix"].tobytes() == want["matrix"].tobytes() and len(g["log"]) == len(want["log"]) for g in got["refine"])
