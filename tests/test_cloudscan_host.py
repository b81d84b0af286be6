"""The observed-space accuracy of `apd --evaluate --against-scans` without a GPU: the serial text of csrc/dvp_cloudscan.hpp
(tests/cloudscan_host) equals the numpy restatement of tests/np_cloudscan.py - maps, truth points and gaps bit for bit, the counts
exactly - over the case table, the room and random scans; the room holds what its description says; the MeshLab project reader takes
the writer's bytes and a rearranged project and refuses every malformed one with its own message; `apd --evaluate --evaluate-on host
--against-scans` prints the restated report, refuses the option mistakes, and without the option prints what it printed before."""
import os
import subprocess

import numpy as np
import pytest

import np_cloudicp as C
import np_cloudprep as P
import np_cloudscan as S
import np_evaluate as N
from conftest import ROOT

pytestmark = pytest.mark.hostbox

CASES = S.cases()
APD = os.path.join(ROOT, "dvp-mvs_amd", "apd")


@pytest.fixture(scope="module", autouse=True)
def built():
    S.build_program()


@pytest.fixture(scope="module")
def room():
    return S.room()


@pytest.fixture(scope="module")
def room_serial(room, tmp_path_factory):
    rc, err, got = S.serial_evaluate(room["recon"], room["scans"], S.ROOM_TOLERANCES, S.ROOM_R, tmp_path_factory.mktemp("room"))
    assert rc == 0, err
    return got


@pytest.mark.parametrize("case", list(CASES))
def test_serial_text_equals_numpy(tmp_path, case):
    c = CASES[case]
    want = dict(truth=S.truth_cloud(c["scans"]), maps=S.maps(c["scans"], c["R"]))
    want["gap"] = S.gaps(c["queries"], c["scans"], c["R"], want["maps"])
    rc, err, got = S.serial_gaps(c["scans"], c["queries"], c["R"], tmp_path)
    assert rc == 0, err
    assert S.same_gaps(got, want) == ""


def test_the_case_table_holds_what_it_says():
    inf = np.inf
    gap = lambda name: S.gaps(CASES[name]["queries"], CASES[name]["scans"], CASES[name]["R"])
    assert gap("one_point").tolist() == [0.5, -1.0, -inf]
    g = gap("empty_scan")
    assert g[:2].tolist() == [-inf, -inf] and np.isnan(g[2])
    for n in (63, 64, 65, 129):      # every point of the scan and every query in one and the same texel
        c = CASES["one_texel_%d" % n]
        t, _, ok = S.texel_of(np.concatenate([c["scans"][0][0], c["queries"]]), [0, 0, 0], 16)
        assert ok.all() and len(set(t.tolist())) == 1 and len(c["queries"]) == n
        assert np.isfinite(S.maps(c["scans"], 16)).sum() == 1
    # the directions: 26 distinct texels, the nearer of the two ranges kept, every query observed; the diagonal's su == 1 is clamped
    for R in (16, 64, 1024):
        c = CASES["directions_R%d" % R]
        m = S.maps(c["scans"], R)
        assert np.isfinite(m).sum() == 26 and np.isfinite(gap("directions_R%d" % R)).all()
        t, _, _ = S.texel_of([[1, 1, 0], [1, 0, 1], [-1, 1, 1]], [0, 0, 0], R)
        assert t.tolist() == [(0 * R + R // 2) * R + R - 1, (0 * R + R - 1) * R + R // 2, (1 * R + R - 1) * R + R - 1]
    # ties go to the lower axis: |dx| == |dy| is face x, |dy| == |dz| with a smaller |dx| is face y
    t, _, _ = S.texel_of([[1, -1, 0], [0.5, -1, 1]], [0, 0, 0], 16)
    assert (t // 256).tolist() == [0, 3]
    assert gap("negative_zero").tolist() == [1, 1, 1, 1, -1, -1, -1, -1]
    g = gap("void_at_scanner")
    assert g[0] == -inf and g[1] == 0.5 and np.isnan(g[[2, 3, 5]]).all() and g[4] > 0 and g[6] == -1.5
    c = CASES["void_at_scanner"]
    assert np.isfinite(S.maps(c["scans"], 16)).sum() == 3      # the point at the scanner and the three non-finite ones fall nowhere
    # differences and squares that overflow binary32 are void beside two returns that are not
    g = gap("void_overflow")
    assert g[:4].tolist() == [-inf] * 4 and g[4] == np.float32(1e10) and -5.1e18 < g[5] < -4.9e18 and np.isfinite(S.maps(CASES["void_overflow"]["scans"], 16)).sum() == 2
    assert gap("two_scans").tolist() == [4.0, 1.0, -1.0, 3.0, -inf]
    assert len(CASES["scans_64"]["scans"]) == 64 and (gap("scans_64") > 0).sum() > 5
    assert (gap("far_transform") > 0).sum() > 50


def test_the_thresholds(tmp_path):
    """a gap exactly t_k is not free space, one ulp above it is; a point within the tolerance of the truth is accurate whatever lies
    behind it"""
    T = S.THRESHOLD
    rc, err, got = S.serial_evaluate(T["recon"], T["scans"], T["tolerances"], T["R"], tmp_path)
    assert rc == 0, err
    assert got["gap"].tolist() == [0.4375] and np.float32(T["tolerances"][0]) == np.nextafter(np.float32(0.4375), np.float32(0))
    assert got["free_space"].tolist() == [1, 0] and got["within_recon"].tolist() == [0, 0]
    assert S.same_evaluation(got, S.evaluate(T["recon"], T["scans"], T["tolerances"], T["R"])) == ""
    A = S.ACCURATE_FIRST
    rc, err, got = S.serial_evaluate(A["recon"], A["scans"], A["tolerances"], A["R"], tmp_path)
    assert rc == 0, err
    assert got["gap"].tolist() == [4.0, 3.0] and got["within_recon"].tolist() == [1, 1] and got["free_space"].tolist() == [1, 1]
    assert S.same_evaluation(got, S.evaluate(A["recon"], A["scans"], A["tolerances"], A["R"])) == ""


def test_the_room_equals_numpy(room, room_serial, tmp_path):
    """the distances of 7 000 points against 485 000 are left to dvp_cloudeval.hpp's own tests: numpy takes them as given"""
    want = S.evaluate(room["recon"], room["scans"], S.ROOM_TOLERANCES, S.ROOM_R, d2=room_serial["d2_recon"])
    assert S.same_evaluation(room_serial, want) == ""
    rc, err, got = S.serial_gaps(room["scans"], room["recon"], S.ROOM_R, tmp_path)
    assert rc == 0, err
    maps = S.maps(room["scans"], S.ROOM_R)
    assert S.same_gaps(got, dict(truth=S.truth_cloud(room["scans"]), maps=maps, gap=S.gaps(room["recon"], room["scans"], S.ROOM_R, maps))) == ""


def test_the_room_holds_what_it_says(room, room_serial):
    maps = S.maps(room["scans"], S.ROOM_R)
    assert maps.shape == (2, 6 * 64 * 64) and np.isfinite(maps).all()      # no texel is empty
    gap = room_serial["gap"]
    assert (gap[room["inner"]] > 0.6).all() and (gap[room["outer"]] < -0.59).all()
    inner, outer, walls = (s.stop - s.start for s in (room["inner"], room["outer"], room["walls"]))
    assert (inner, outer, walls) == (2000, 2000, 3000)
    for k, t in enumerate(S.ROOM_TOLERANCES):
        assert room_serial["free_space"][k] == inner and room_serial["within_recon"][k] == walls
        assert room_serial["used"][0] - room_serial["within_recon"][k] - room_serial["free_space"][k] == outer
    # class by class: the inner points are free space, the outer ones unobserved, the wall samples accurate
    t2 = np.float32(0.5) * np.float32(0.5)
    d2 = room_serial["d2_recon"]
    assert not (d2[room["inner"]] <= t2).any() and not (d2[room["outer"]] <= t2).any() and (d2[room["walls"]] == 0).all()


def test_a_plate_hides_from_one_scanner_what_the_other_sees(tmp_path):
    scans, behind = S.plate_scene()
    tol = [0.1, 0.2]
    alone = S.serial_evaluate(behind, scans[:1], tol, S.ROOM_R, tmp_path)[2]
    both = S.serial_evaluate(behind, scans, tol, S.ROOM_R, tmp_path)[2]
    assert (alone["gap"] < -0.49).all() and alone["free_space"].tolist() == [0, 0] and alone["within_recon"].tolist() == [0, 0]
    assert (both["gap"] > 0.5).all() and both["free_space"].tolist() == [50, 50]
    assert S.same_evaluation(both, S.evaluate(behind, scans, tol, S.ROOM_R, d2=both["d2_recon"])) == ""


def test_random_scans_equal_numpy(tmp_path):
    scans, queries = S.random_case()
    tol = [0.05, 0.1, 0.5]
    rc, err, got = S.serial_evaluate(queries, scans, tol, 64, tmp_path)
    assert rc == 0, err
    assert S.same_evaluation(got, S.evaluate(queries, scans, tol, 64)) == ""
    assert got["free_space"][0] > 100 and got["within_recon"][2] > 100 and (got["used"][0] - got["within_recon"] - got["free_space"] > 0).all()
    rc, err, raw = S.serial_gaps(scans, queries, 64, tmp_path)
    assert rc == 0, err
    maps = S.maps(scans, 64)
    assert S.same_gaps(raw, dict(truth=S.truth_cloud(scans), maps=maps, gap=S.gaps(queries, scans, 64, maps))) == ""
    # prepared clouds: the maps are made of every scan point, the truth cloud alone is thinned
    prep_recon, prep_truth = P.prep(P.rotation(1.0, -0.5, [0.01, 0.02, -0.01]), None, 0.05), P.prep(None, P.crop_of(2, -3.0, 3.0, P.polygon_3d(2, P.BIG_SQUARE)), 0.05)
    rc, err, got = S.serial_evaluate(queries, scans, tol, 64, tmp_path, prep_recon, prep_truth)
    assert rc == 0, err
    want = S.evaluate(queries, scans, tol, 64, prep_recon, prep_truth)
    assert S.same_evaluation(got, want) == "" and got["counts"][1, 3] < got["counts"][1, 0] and got["counts"][0, 3] < got["counts"][0, 0]


def test_refusals(tmp_path):
    x = [[1, 0, 0]]
    bad_row, nan_m = np.eye(4), np.eye(4)
    bad_row[3, 1] = 1e-300
    nan_m[0, 3] = np.nan
    for scans, R, say in (([S.scan(x)], 24, "cube_size must be a power of two, 16 ... 4096, got 24"), ([S.scan(x)], 8, "got 8"), ([S.scan(x)], 8192, "got 8192"),
                          ([S.scan(x)], 0, "got 0"), ([], 16, "num_scans must be 1 ... 64, got 0"), ([S.scan(x)] * 65, 16, "num_scans must be 1 ... 64, got 65"),
                          ([S.scan(x), S.scan(x, bad_row)], 16, "scan 1: the transform's last row must be 0 0 0 1"),
                          ([S.scan(x, nan_m)], 16, "scan 0: the transform holds a non-finite entry"), ([S.scan(x) + (-1,)], 16, "scan 0: a scan holds 0 or more points, got -1")):
        rc, err, _ = S.serial_gaps(scans, x, R, tmp_path)
        assert rc == 3 and say in err, (say, err)
    rc, err, _ = S.serial_evaluate(x, [S.scan(x)], [0.2, 0.1], 16, tmp_path)
    assert rc == 3 and "strictly ascending" in err
    rc, err, _ = S.serial_evaluate(x, [S.scan(x)], [0.1], 16, tmp_path, P.prep(voxel=-1.0))
    assert rc == 3 and "voxel must be finite and positive" in err


# ---- the MeshLab project reader ---------------------------------------------------------------------------------------------------
def read_mlp(tmp_path, text):
    path = str(tmp_path / "project.mlp")
    with open(path, "w") as f:
        f.write(text)
    out = S.run_program("mlp", path)
    rows = [ln.split() for ln in out.stdout.splitlines()]
    return out.returncode, out.stderr, [(r[0], r[1], [float.fromhex(w) for w in r[2:]]) for r in rows]


def test_mlp_reader(tmp_path):
    m = [P.rotation(10.0, 20.0, [1.5, -2.25, 1e-3]), S.moved_to([0.1, 0.2, 0.3])]
    rc, err, got = read_mlp(tmp_path, S.mlp_text(["scan1.ply", "sub/scan2.ply"], m))
    assert rc == 0, err
    assert [g[0] for g in got] == ["scan1.ply", "sub/scan2.ply"] and [g[1] for g in got] == [str(tmp_path / "scan1.ply"), str(tmp_path / "sub" / "scan2.ply")]
    assert got[0][2] == m[0].tolist() and got[1][2] == m[1].tolist()
    rc, err, got = read_mlp(tmp_path, S.mlp_text(["a.ply", "/abs/b.ply"], m))
    assert rc == 0 and got[1][1] == "/abs/b.ply" and got[1][2] == m[1].tolist()
    # attributes in another order, single quotes, the numbers on one line, other elements and attributes, a comment that holds an element
    one_line = " ".join(repr(float(v)) for v in m[0])
    text = ("<?xml version='1.0'?>\n<!DOCTYPE MeshLabDocument>\n<MeshLabProject><!-- <MLMesh filename=\"no.ply\"/> -->\n<MeshGroup>\n<MLMesh visible = '1' filename='scan1.ply'\n label=\"x > y\">"
            "<RenderingOption solidColor=\"192 192 192 255\">100001</RenderingOption>\n<MLMatrix44>%s</MLMatrix44></MLMesh>\n</MeshGroup><RasterGroup><MLRaster label='r'/></RasterGroup></MeshLabProject>" % one_line)
    rc, err, got = read_mlp(tmp_path, text)
    assert rc == 0, err
    assert len(got) == 1 and got[0][0] == "scan1.ply" and got[0][2] == m[0].tolist()
    good = S.mlp_text(["scan1.ply"], m[:1])
    numbers = good[good.index("<MLMatrix44>") + 12:good.index("</MLMatrix44>")]
    row = lambda *v: good.replace(numbers, "\n1 0 0 0\n0 1 0 0\n0 0 1 0\n%s %s %s %s\n" % v)
    for text, say in (("<MeshLabProject><MeshGroup/></MeshLabProject>", "holds no MLMesh element"), ("", "holds no MLMesh element"),
                      (good.replace(' filename="scan1.ply"', ""), "MLMesh element 1 has no filename"), (good.replace('filename="scan1.ply"', 'filename=""'), "has no filename"),
                      (good.replace("MLMatrix44", "Matrix"), "the MLMesh scan1.ply has no MLMatrix44"),
                      ('<MLMesh filename="a.ply"/><MLMesh filename="b.ply"><MLMatrix44>%s</MLMatrix44></MLMesh>' % one_line, "the MLMesh a.ply has no MLMatrix44"),
                      ('<MLMesh filename="a.ply"></MLMesh><MLMesh filename="b.ply"><MLMatrix44>%s</MLMatrix44></MLMesh>' % one_line, "the MLMesh a.ply has no MLMatrix44"),
                      (good.replace(numbers, numbers + " 1"), "holds 17 numbers; a transform is 16"), (good.replace(numbers, " 1 2 3 "), "holds 3 numbers"),
                      (good.replace(numbers, ""), "holds 0 numbers"), (good.replace(numbers, numbers.replace("1.5", "1.5q")), "`1.5q` is not a number"),
                      (good.replace(numbers, numbers.replace("1.5", "nan")), "non-finite entry"), (good.replace(numbers, numbers.replace("1.5", "1e999")), "non-finite entry"),
                      (row(0, 0, 0, 2), "last row must be 0 0 0 1, got 0 0 0 2"), (row(0, "1e-300", 0, 1), "last row must be 0 0 0 1"),
                      (S.mlp_text(["s%d.ply" % k for k in range(65)], [m[1]] * 65), "holds more than 64 scans")):
        rc, err, got = read_mlp(tmp_path, text)
        assert rc == 2 and say in err and got == [], (text[:200], err)
    assert read_mlp(tmp_path, S.mlp_text(["s%d.ply" % k for k in range(64)], [m[1]] * 64))[0] == 0
    out = S.run_program("mlp", str(tmp_path / "absent.mlp"))
    assert out.returncode == 2 and "cannot read" in out.stderr


# ---- the sub-command on the host --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(room, tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    d = tmp_path_factory.mktemp("apd")
    recon = str(d / "recon.ply")
    N.write_ply_like_apd(recon, room["recon"])
    project, names = S.write_scans(d, room["scans"])
    truth = str(d / "truth.ply")
    N.write_ply_like_apd(truth, S.truth_cloud(room["scans"]))
    return dict(recon=recon, project=project, names=names, truth=truth, folder=d)


def apd_host(files, *args):
    return subprocess.run([APD, "--evaluate", files["recon"], "--evaluate-on", "host", "--tolerances", N.tolerance_text(S.ROOM_TOLERANCES)] + [str(a) for a in args],
                          capture_output=True, text=True, timeout=300)


def test_apd_prints_the_restated_report(files, room, room_serial, tmp_path):
    out = apd_host(files, "--against-scans", files["project"], "--cube-size", S.ROOM_R, "--out", tmp_path / "report.txt")
    assert out.returncode == 0, out.stderr
    want = S.report_text(files["recon"], files["project"], files["names"], room["scans"], room_serial, S.ROOM_TOLERANCES, len(room["recon"]))
    assert out.stdout == want and open(str(tmp_path / "report.txt")).read() == want
    lines = want.splitlines()
    assert lines[2] == "scan scan1.ply: 242406 points, scanner at 0 0 0" and lines[3] == "scan scan2.ply: 242406 points, scanner at 0.5 -0.300000012 0.200000003"
    # the observed-space accuracy is exactly walls / (walls + inner)
    assert lines[4] == "tolerance accuracy completeness f1" and all(ln.split()[1] == "%.6f" % (100.0 * 3000 / 5000) for ln in lines[5:8])
    assert lines[8:] == ["tolerance accurate free_space unobserved"] + ["%.9g 3000 2000 2000" % float(np.float32(t)) for t in S.ROOM_TOLERANCES]
    # the default cube of 1 024 leaves most texels of this coarse room empty: fewer points are observed, none is misjudged
    wide = apd_host(files, "--against-scans", files["project"])
    assert wide.returncode == 0 and [int(ln.split()[2]) <= 2000 for ln in wide.stdout.splitlines()[9:]] == [True] * 3


def test_apd_with_a_preparation_and_saved_clouds(files, room, tmp_path):
    rough = str(tmp_path / "rough.txt")
    M = P.rotation(0.2, -0.1, [0.004, -0.003, 0.002])
    with open(rough, "w") as f:
        f.write("\n".join(" ".join("%.17g" % v for v in row) for row in M.reshape(4, 4)) + "\n")
    out = apd_host(files, "--against-scans", files["project"], "--cube-size", S.ROOM_R, "--transform", rough, "--voxel-size", "0.1", "--save-prepared", tmp_path / "p_")
    assert out.returncode == 0, out.stderr
    prep_recon, prep_truth = P.prep(M, None, 0.1), P.prep(None, None, 0.1)
    rc, err, got = S.serial_evaluate(room["recon"], room["scans"], S.ROOM_TOLERANCES, S.ROOM_R, tmp_path, prep_recon, prep_truth)
    assert rc == 0, err
    assert out.stdout == S.report_text(files["recon"], files["project"], files["names"], room["scans"], got, S.ROOM_TOLERANCES, len(room["recon"]), prepares=True)
    N.build_program()
    for which, prep, raw in (("recon", prep_recon, room["recon"]), ("truth", prep_truth, S.truth_cloud(room["scans"]))):
        rc, err, saved = N.read_ply(str(tmp_path / ("p_%s.ply" % which)), tmp_path)
        assert rc == 0 and N.same_bits(saved, P.prepare(raw, **prep)["xyz"]), which


def test_apd_refuses_option_mistakes(files, tmp_path):
    for args, say in ((("--against", files["truth"], "--cube-size", "64"), "--cube-size needs --against-scans"),
                      (("--against", files["truth"], "--against-scans", files["project"]), "--against and --against-scans exclude each other"),
                      ((), "--against is required"), (("--against-scans", files["project"], "--cube-size", "100"), "--cube-size takes a power of two, 16 ... 4096, got `100`"),
                      (("--against-scans", files["project"], "--cube-size", "8"), "got `8`"), (("--against-scans", files["project"], "--cube-size", "8192"), "got `8192`"),
                      (("--against-scans", files["project"], "--cube-size", "64x"), "got `64x`"), (("--against-scans", str(tmp_path / "absent.mlp")), "cannot read")):
        out = apd_host(files, *args)
        assert out.returncode == 1 and say in out.stderr and out.stdout == "", (args, out.stderr)
    lost = str(tmp_path / "lost.mlp")
    S.write_mlp(lost, ["nowhere.ply"], [S.IDENTITY])
    out = apd_host(files, "--against-scans", lost)
    assert out.returncode == 1 and "scan nowhere.ply: " in out.stderr and "nowhere.ply" in out.stderr.split("scan nowhere.ply: ")[1]
    bad = str(tmp_path / "bad.mlp")
    open(bad, "w").write("<MeshLabProject/>")
    out = apd_host(files, "--against-scans", bad)
    assert out.returncode == 1 and "holds no MLMesh element" in out.stderr


def test_without_the_option_the_report_is_the_existing_one(files, room, tmp_path):
    """--against on the truth cloud of the same scans: the bytes that tests/np_cloudicp.py restates from the format before this option,
    filled with the counts of the existing serial text"""
    truth = S.truth_cloud(room["scans"])
    rc, err, res = N.serial(room["recon"], truth, S.ROOM_TOLERANCES, tmp_path)
    assert rc == 0, err
    out = apd_host(files, "--against", files["truth"])
    assert out.returncode == 0, out.stderr
    assert out.stdout == C.report_text(files["recon"], files["truth"], [len(room["recon"]), len(truth)], res["used"], res["within_recon"], res["within_truth"], S.ROOM_TOLERANCES)
    assert "scan" not in out.stdout.replace(files["recon"], "").replace(files["truth"], "") and "free_space" not in out.stdout
    # every reconstructed point counts there: 3 000 of 7 000 are accurate, where the observed space has 3 000 of 5 000
    assert [ln.split()[1] for ln in out.stdout.splitlines()[3:]] == ["%.6f" % (100.0 * 3000 / 7000)] * 3
