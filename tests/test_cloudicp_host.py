"""The alignment refinement of `apd --evaluate` without a GPU: the serial text of csrc/dvp_cloudicp.hpp (tests/cloudicp_host) equals
the numpy restatement of tests/np_cloudicp.py over the case table and on random points - nearest and the count exactly, e and the 16
sums bit for bit, by the double loop and by the grid with either neighbourhood -; the tree sum against math.fsum; the solve against an
independent float64 Kabsch; the stage loop against a numpy loop around the restated step; every refusal and its message; and `apd
--evaluate --evaluate-on host --refine-alignment` end to end, with the saved matrix read back by --transform."""
import math
import os
import subprocess

import numpy as np
import pytest

import np_cloudicp as C
import np_cloudprep as P
import np_evaluate as N
from conftest import ROOT

CASES = C.cases()
APD = os.path.join(ROOT, "dvp-mvs_amd", "apd")


@pytest.fixture(scope="module", autouse=True)
def built():
    C.build_program()


@pytest.fixture(scope="module")
def restated():
    known = {}

    def of(name):
        if name not in known:
            c = CASES[name]
            known[name] = C.step(c["src"], c["tgt"], c["D"], c["d"])
        return known[name]
    return of


@pytest.mark.parametrize("case", list(CASES))
def test_serial_step_equals_numpy(tmp_path, restated, case):
    c, want = CASES[case], restated(case)
    for cells, search in ((None, None), (27, "grid"), (125, "grid"), (27, "brute")):
        rc, err, got = C.serial_step(c["src"], c["tgt"], tmp_path, c["D"], c["d"], cells, search)
        assert rc == 0, err
        assert C.same_step(got, want) == "", (cells, search)


def test_the_case_table_holds_what_it_says(restated):
    assert len(C.cell_offsets(CASES["every_cell_27"], 1)) == 27 and len(C.cell_offsets(CASES["every_cell_125"], 2)) == 125
    assert restated("exactly_two")["count"] == 2 and restated("tree_all_257")["count"] == 257 and restated("tree_none_257")["count"] == 0
    assert restated("equidistant_other_cells")["nearest"].tolist() == [1, 3]
    chunks = restated("equidistant_other_chunks")
    assert chunks["count"] == 100 and (chunks["nearest"] < 64).all()
    assert restated("target_at_d")["count"] == 1 and restated("target_ulp_beyond_d")["count"] == 0
    assert restated("target_at_d_tenth")["count"] == 1 and restated("target_ulp_beyond_d_tenth")["count"] == 0
    assert restated("image_overflows_binary32")["nearest"][33] == -1 and restated("non_finite_sources")["count"] == 194
    assert np.signbit(restated("negative_zero_2")["sums"][6:15]).all() and not np.signbit(restated("negative_zero_3")["sums"][6:15]).any()
    assert len(CASES["tree_second_level_seam"]["src"]) == 256 * 1024 + 300


@pytest.mark.parametrize("case", ["random_3000", "near_1e4", "tree_second_level_seam", "rotation"])
def test_tree_sums_are_within_the_bound_of_the_exact_sum(restated, case):
    """every addition rounds by at most 2^-53 of its result, and no partial sum of a column exceeds the sum of its |leaf|: over the
    N - 1 additions the tree is within N * 2^-53 * sum |leaf| of the exact sum, which math.fsum rounds once"""
    res = restated(case)
    leaves = res["leaves"]
    for k in range(16):
        exact = math.fsum(leaves[:, k])
        bound = len(leaves) * 2.0 ** -53 * math.fsum(np.abs(leaves[:, k]))
        assert abs(res["sums"][k] - exact) <= bound, (k, res["sums"][k], exact, bound)


def planar_case():
    rng = np.random.default_rng(3)
    tgt = rng.random((400, 3))
    tgt[:, 2] = 0.25
    turn = P.rotation(4.0, 0.0, [0.01, -0.02, 0.0]).reshape(4, 4)
    src = (np.linalg.inv(turn) @ np.concatenate([tgt, np.ones((400, 1))], 1).T).T[:, :3]
    return C.case(src, tgt, None, 0.2)


@pytest.mark.parametrize("case", ["rotation", "large_translation", "random_3000", "negative_coordinates", "near_1e4", "planar"])
def test_solve_against_kabsch(restated, case):
    if case == "planar":
        c = planar_case()
        res = C.step(c["src"], c["tgt"], c["D"], c["d"])
    else:
        c, res = CASES[case], restated(case)
    ref = C.reference_point(c["tgt"])
    E = C.serial_solve(res["sums"], res["count"], ref).reshape(4, 4)
    R = E[:3, :3]
    assert abs(np.linalg.det(R) - 1.0) <= 1e-14 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-14
    assert E[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    if case != "planar":      # (a plane's third singular value is 0: the SVD's own answer is no better conditioned than ours)
        K = C.kabsch(res["sums"], res["count"], ref).reshape(4, 4)
        assert np.abs(E[:3, :3] - K[:3, :3]).max() <= 1e-12, (E, K)
        # The translation is a difference of coordinates of the size of c.  Where that is of order one, every entry within 1e-12.  Near
        # 1e4 a double's spacing is 2^-39 = 1.8e-12 and 1e-12 cannot be met: there the bound is what the operands allow - the 16
        # roundings of the two computations, half a spacing each, plus the 1e-12 allowed on each of a row's three rotation entries
        # times a coordinate of at most |c| + 1.
        size = np.abs(ref).max()
        bound = 1e-12 if case != "near_1e4" else 16 * 2.0 ** -40 + 3 * 1e-12 * (size + 1.0)
        assert (size < 8.0) == (case != "near_1e4") and np.abs(E[:3, 3] - K[:3, 3]).max() <= bound, (E, K, bound)
    else:
        assert res["count"] == 400 and np.ptp(c["tgt"][:, 2]) == 0.0      # (all correspond, and the targets do lie in one plane)


@pytest.mark.parametrize("which", ["whole", "cropped"])
def test_stage_loop_equals_a_numpy_loop(tmp_path, which):
    recon, truth, known, initial, crop = C.refine_scene()
    crop = crop if which == "cropped" else None
    rc, err, got = C.serial_refine(recon, truth, tmp_path, initial, crop, C.STAGES)
    assert rc == 0, err
    M, log = np.asarray(initial, np.float64).reshape(4, 4), []

    def compose(E, D):      # the header's summation order
        out = np.eye(4)
        for r in range(3):
            for k in range(4):
                out[r, k] = ((E[r, 0] * D[0, k] + E[r, 1] * D[1, k]) + E[r, 2] * D[2, k]) + E[r, 3] * D[3, k]
        return out
    for s, (v, d, k) in enumerate(C.STAGES):
        src = P.prepare(recon, M.reshape(-1), crop, v)["xyz"]
        tgt = P.prepare(truth, None, crop, v)["xyz"]
        D, last = np.eye(4), None
        for it in range(1, k + 1):
            res = C.step(src, tgt, D.reshape(-1), d)
            n = res["count"]
            now = (n / len(src), math.sqrt(res["sums"][15] / n))
            log.append((s, it, len(src), n, now[1]))
            if n < 3 or (last is not None and abs(now[0] - last[0]) < 1e-6 and abs(now[1] - last[1]) < 1e-6):
                break
            last = now
            D = compose(C.serial_solve(res["sums"], n, C.reference_point(tgt)).reshape(4, 4), D)
        M = compose(D, M)
    assert got["matrix"].tobytes() == M.reshape(-1).tobytes()
    assert len(got["log"]) == len(log) and all(g[:4] == w[:4] and float(g[4]).hex() == float(w[4]).hex() for g, w in zip(got["log"], log)), (got["log"], log)
    before, after = C.motion_errors(initial, known), C.motion_errors(got["matrix"], known)
    assert after[0] < 0.1 * before[0] and after[1] < 0.1 * before[1]
    again = C.serial_refine(recon, truth, tmp_path, initial, crop, C.STAGES, cells=27)[2]
    assert again["matrix"].tobytes() == got["matrix"].tobytes() and again["log"] == got["log"]


def test_a_stage_with_fewer_than_three_correspondences_ends(tmp_path):
    recon, truth, known, initial, crop = C.refine_scene()
    away = np.eye(4)
    away[:3, 3] = [100.0, 0.0, 0.0]
    rc, err, got = C.serial_refine(recon, truth, tmp_path, away.reshape(-1), None, [(0.05, 0.1, 20), (0.0, 0.1, 5)])
    assert rc == 0, err
    assert got["matrix"].tobytes() == away.reshape(-1).tobytes() and [g[:2] for g in got["log"]] == [(0, 1), (1, 1)] and all(g[3] == 0 and g[4] == 0.0 for g in got["log"])
    rc, err, two = C.serial_refine(truth[[20, 30]] + np.float32(0.001), truth[:100], tmp_path, None, None, [(0.0, 0.01, 20)])
    assert rc == 0 and two["matrix"].tobytes() == np.eye(4).tobytes() and [g[:4] for g in two["log"]] == [(0, 1, 2, 2)]


def test_refusals(tmp_path):
    xyz = P.cloud(np.random.default_rng(2).random((100, 3)))
    bad_row, nan_m = np.eye(4), np.eye(4)
    bad_row[3, 0] = 1e-300
    nan_m[1, 1] = np.nan
    holed = xyz.copy()
    holed[5, 2] = np.nan
    for args, say in (((xyz, xyz, tmp_path, bad_row, 0.1), "the increment's last row must be 0 0 0 1"), ((xyz, xyz, tmp_path, nan_m, 0.1), "the increment holds a non-finite entry"),
                      ((xyz, xyz, tmp_path, None, 0.0), "max_distance (0) must be finite and positive"), ((xyz, xyz, tmp_path, None, -1.0), "must be finite and positive"),
                      ((xyz, xyz, tmp_path, None, np.inf), "must be finite and positive"), ((xyz, xyz, tmp_path, None, np.nan), "must be finite and positive"),
                      ((xyz, xyz, tmp_path, None, 1e-20), "normal binary32 square"), ((xyz, xyz, tmp_path, None, 1e30), "normal binary32 square"),
                      ((xyz, holed, tmp_path, None, 0.1), "the targets must have finite coordinates, 1 of 100 have not"),
                      ((xyz, [[0, 0, 0], [1e6, 0, 0]], tmp_path, None, 1e-3), "at most 2097150 are supported")):
        rc, err, _ = C.serial_step(*args)
        assert rc == 3 and say in err, (say, err)
    square = P.polygon_3d(2, P.BIG_SQUARE)
    for kw, say in ((dict(stages=[]), "num_stages must be 1 ... 8, got 0"), (dict(stages=[(0, 0.1, 1)] * 9), "num_stages must be 1 ... 8, got 9"),
                    (dict(stages=[(-0.1, 0.1, 1)]), "stage 0: voxel must be finite and positive"), (dict(stages=[(0, 0.1, 1), (np.nan, 0.1, 1)]), "stage 1: voxel must be finite and positive"),
                    (dict(stages=[(0, 0.0, 1)]), "stage 0: max_distance (0) must be finite and positive"), (dict(stages=[(0, 1e-30, 1)]), "normal binary32 square"),
                    (dict(stages=[(0, 0.1, 0)]), "max_iterations must be 1 ... 1000, got 0"), (dict(stages=[(0, 0.1, 1001)]), "max_iterations must be 1 ... 1000, got 1001"),
                    (dict(stages=[(0, 0.1, 1)], transform=bad_row), "last row must be 0 0 0 1"), (dict(stages=[(0, 0.1, 1)], transform=nan_m), "non-finite entry"),
                    (dict(stages=[(0, 0.1, 1)], crop=P.crop_of(2, 0, 1, square[:2])), "at least 3 vertices, got 2"),
                    (dict(stages=[(0, 0.1, 1)], crop=P.crop_of(2, 1, 0, square)), "axis_min (1) must not exceed axis_max (0)"),
                    (dict(stages=[(1e-7, 0.1, 1)]), "voxels of edge 1e-07; at most 2097150 are supported")):
        rc, err, _ = C.serial_refine(xyz, xyz, tmp_path, **kw)
        assert rc == 3 and say in err, (say, err)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the refinement scene as the files `apd --evaluate` takes"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    d = tmp_path_factory.mktemp("apd")
    recon, truth, known, initial, crop = C.refine_scene()
    names = dict(recon=str(d / "recon.ply"), truth=str(d / "truth.ply"), rough=str(d / "rough.txt"), fine=str(d / "fine.txt"))
    N.write_ply_like_apd(names["recon"], recon[np.isfinite(recon).all(1)])
    N.write_ply_like_apd(names["truth"], truth[np.isfinite(truth).all(1)])
    with open(names["rough"], "w") as f:
        f.write("\n".join(" ".join("%.17g" % v for v in row) for row in np.asarray(initial).reshape(4, 4)) + "\n")
    names["stages"] = ",".join("%.17g:%.17g:%d" % s for s in C.STAGES)
    return names


def apd_host(files, *args):
    return subprocess.run([APD, "--evaluate", files["recon"], "--against", files["truth"], "--evaluate-on", "host", "--tolerances", "0.01,0.02,0.05"] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=300)


def test_apd_refines_on_the_host_and_the_saved_matrix_reads_back(files, tmp_path):
    recon, truth, known, initial, crop = C.refine_scene()
    out = apd_host(files, "--transform", files["rough"], "--refine-alignment", files["stages"], "--save-transform", files["fine"])
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    rc, err, want = C.serial_refine(recon[np.isfinite(recon).all(1)], truth[np.isfinite(truth).all(1)], tmp_path, initial, None, C.STAGES)
    assert rc == 0, err
    for s in range(3):
        last = [g for g in want["log"] if g[0] == s][-1]
        assert lines[s] == "alignment stage %d: %d steps, %d of %d correspondences, rmse %.9g" % (s, last[1], last[3], last[2], last[4])
    rows = [" ".join("%.17g" % v for v in row) for row in want["matrix"].reshape(4, 4)]
    assert lines[3:7] == ["alignment " + r for r in rows] and open(files["fine"]).read().splitlines() == rows
    assert lines[7].startswith("reconstruction ") and lines[9].startswith("prepared reconstruction: ") and lines[11] == "tolerance accuracy completeness f1"
    # the saved matrix through --transform, no refinement: the same evaluation lines
    again = apd_host(files, "--transform", files["fine"])
    assert again.returncode == 0 and again.stdout.splitlines() == lines[7:]
    rough = apd_host(files, "--transform", files["rough"])
    accuracy = lambda text: float(text.splitlines()[-3].split()[1])
    assert rough.returncode == 0 and "alignment" not in rough.stdout and accuracy(out.stdout) > accuracy(rough.stdout)
    # without --transform the stages start from the identity
    plain = apd_host(files, "--refine-alignment", "0:0.05:2")
    assert plain.returncode == 0 and plain.stdout.splitlines()[0].startswith("alignment stage 0: ")


def test_apd_refuses_bad_stage_lists(files):
    for v, say in (("", "--refine-alignment takes VOXEL:DISTANCE:ITERATIONS"), ("0.1:0.2", "got `0.1:0.2`"), ("0.1:0.2:3:4", "got `0.1:0.2:3:4`"), ("a:0.2:3", "got `a:0.2:3`"),
                   ("0.1:0.2:3.5", "got `0.1:0.2:3.5`"), ("0:0.1:1e30", "got `0:0.1:1e30`"), ("0:0.1:nan", "got `0:0.1:nan`"), ("0:0.1:-inf", "got `0:0.1:-inf`"), ("0.1:0.2:3,", "separated by commas"), ("0.1:0.2:3,,0.1:0.2:3", "got ``"), (",".join(["0:0.1:1"] * 9), "at most 8 stages, got 9"),
                   ("0:0:5", "stage 0: max_distance (0) must be finite and positive"), ("-1:0.1:5", "stage 0: voxel must be finite and positive"),
                   ("0:0.1:0", "max_iterations must be 1 ... 1000, got 0")):
        out = apd_host(files, "--refine-alignment", v)
        assert out.returncode == 1 and say in out.stderr and out.stdout == "", (v, out.stderr)
    out = apd_host(files, "--save-transform", files["fine"] + ".none")
    assert out.returncode == 1 and "--save-transform needs --refine-alignment" in out.stderr and not os.path.exists(files["fine"] + ".none")
