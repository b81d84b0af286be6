"""The preparation in front of `apd --evaluate` without a GPU: the serial text of csrc/dvp_cloudprep.hpp (tests/cloudprep_host) equals
the numpy reading (tests/np_cloudprep.py) bit for bit on the case table and on 4 000 random points; the crop decision equals
matplotlib's Path.contains_points on a concave polygon; every centroid lies within s 2^-32 + 8 2^-53 max|coordinate| of the exact
rational mean; a shuffled input gives the same centroid set in the order of the new first points; the --transform and --crop readers
on what they take and on every refusal; the refusals of the description."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import np_cloudprep as P
from conftest import ROOT

pytestmark = pytest.mark.hostbox

CASES = P.cases()
GOLDEN = os.path.join(ROOT, "tests", "golden", "evaluate")


@pytest.fixture(scope="module", autouse=True)
def built():
    P.build_program()


@pytest.mark.parametrize("case", list(CASES))
def test_serial_text_equals_numpy(tmp_path, case):
    xyz, prep = CASES[case]
    rc, err, got = P.serial(xyz, tmp_path, **prep)
    assert rc == 0, err
    assert P.same_result(got, P.prepare(xyz, **prep)) == ""


def test_the_case_table_holds_what_it_says():
    for axis in range(3):
        xyz, prep = CASES["crop_edges_axis%d" % axis]
        u, v = P.uv_of(axis)
        kept = P.prepare(xyz, **prep)
        # both bounds are inclusive, one ulp outside is outside
        assert set(np.unique(kept["xyz"][:, axis]).tolist()) == {-0.75, 0.375, 1.5}
        mid = xyz[:, axis] == np.float32(0.375)
        inside = {(int(p[u]), int(p[v])) for p in kept["xyz"][kept["xyz"][:, axis] == np.float32(0.375)]}
        # worked by hand from the rule.  On the slanted edge through (3, 3): two crossings, out; on the one through (1, 3): its own
        # edge does not count (1 < 1 fails), one crossing, in; the vertex (2, 2), at the v of two edges' ends: in.  The left border
        # u = 0 is out and the right border u = 4 in (the side test is strict); the rows v = 0 and v = 4 at the vertices' v are out:
        # no edge has an end below 0, and at v = 4 the crossings come in pairs.
        assert (3, 3) not in inside and (1, 3) in inside and (1, 1) in inside and (2, 2) in inside and (2, 1) in inside
        assert (0, 1) not in inside and (4, 1) in inside and (5, 1) not in inside
        assert not any((a, b) in inside for a in range(-1, 6) for b in (-1, 0, 4, 5)) and mid.sum() == 49
    xyz, prep = CASES["voxel_face_and_minimum"]
    o, i, q = P.voxel_parts(xyz.astype(np.float64), prep["voxel"])
    assert q[0].tolist() == [2 ** 31] * 3 and i[0].tolist() == [0, 0, 0]      # the minimum: f = 0.5
    assert i[1, 0] == 1 and q[1, 0] == 0 and i[2, 0] == 0                      # exactly on the face: the next voxel, f = 0
    xyz, prep = CASES["voxel_near_1e4"]
    o, i, q = P.voxel_parts(xyz.astype(np.float64), prep["voxel"])
    i32 = np.floor((xyz - o.astype(np.float32)) / np.float32(prep["voxel"]))
    assert (i32 != i).any()                                                    # an index formed in binary32 is wrong here
    assert P.prepare(xyz, **prep)["counts"][3] < 1500
    xyz, prep = CASES["voxel_table"]
    out = P.prepare(xyz, **prep)
    assert out["counts"][3] >= 5990 and 2 * out["counts"][2] <= 16384 < 4 * out["counts"][2]
    assert len(CASES["combined"][0]) == 20000 and P.prepare(*[CASES["combined"][0]], **CASES["combined"][1])["counts"][3] > 500


def test_random_points_equal_numpy(tmp_path):
    rng = np.random.default_rng(8)
    xyz = P.cloud(rng.random((4000, 3)) * 1.4 - 0.2)
    _, prep = P.combined_scene()
    for name in (None, "transform", "crop", "voxel"):
        one = dict(prep) if name is None else P.prep(**{name: prep[name]})
        rc, err, got = P.serial(xyz, tmp_path, **one)
        assert rc == 0, err
        assert P.same_result(got, P.prepare(xyz, **one)) == "", name
    rc, err, got = P.serial(xyz, tmp_path)
    assert rc == 0 and got["xyz"].tobytes() == xyz.tobytes() and got["counts"].tolist() == [4000] * 4      # no option: the input's bits


def test_crop_equals_matplotlib():
    from matplotlib.path import Path
    rng = np.random.default_rng(3)
    pts = rng.random((20000, 2)) * 1.4 - 0.2
    poly = np.array(P.CONCAVE_12, np.float64)
    # no point within 1e-9 of an edge: the two rules may only differ there
    nearest = np.full(len(pts), np.inf)
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        t = np.clip(((pts - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
        nearest = np.minimum(nearest, np.linalg.norm(pts - (a + t[:, None] * (b - a)), axis=1))
    assert nearest.min() > 1e-9
    p3 = np.concatenate([pts, np.zeros((len(pts), 1))], 1)
    ours = P.inside_crop(p3, P.crop_of(2, -1.0, 1.0, P.polygon_3d(2, poly)))
    theirs = Path(poly).contains_points(pts)
    assert 4000 < ours.sum() < 16000 and (ours == theirs).all()


def exact_means(xyz, s):
    """{voxel index triple: (exact rational mean per axis)} with the definition's o and i"""
    p = xyz.astype(np.float64)
    o, i, _ = P.voxel_parts(p, s)
    groups = {}
    for k in range(len(p)):
        groups.setdefault(tuple(i[k]), []).append(k)
    return o, {key: [sum(Fraction(float(p[k, a])) for k in ks) / len(ks) for a in range(3)] for key, ks in groups.items()}, groups


@pytest.mark.parametrize("case", ["voxel_shared", "voxel_near_1e4", "voxel_negative"])
def test_centroids_are_within_the_bound_of_the_exact_mean(tmp_path, case):
    # q truncates f by less than one quantum 2^-32, i.e. s 2^-32 per point and so for the mean; then five roundings (the division,
    # the exact scaling, the add of i, the multiply by s, the add of o), each at most 2^-53 of a value of about the
    # largest coordinate's magnitude at most; the roundings inside t = (p - o) / s move f by a few 2^-53 t, that is the point by a
    # few 2^-53 |p - o|: 8 2^-53 max|coordinate| covers them all
    xyz, prep = CASES[case]
    s = prep["voxel"]
    rc, err, got = P.serial(xyz, tmp_path, **prep)
    assert rc == 0, err
    o, means, groups = exact_means(xyz, s)
    assert len(means) == got["counts"][3] <= 2000
    # the centroid in binary64, before the rounding to binary32 that follows: the numpy reading's, whose bits the serial text has
    p = xyz.astype(np.float64)
    _, i, q = P.voxel_parts(p, s)
    bound = Fraction(s) / 2 ** 32 + 8 * Fraction(1, 2 ** 53) * Fraction(float(np.abs(p).max()))
    worst = Fraction(0)
    for key, ks in groups.items():
        Q = [sum(int(q[k, a]) for k in ks) for a in range(3)]
        for a in range(3):
            c = o[a] + (key[a] + (float(Q[a]) / float(len(ks))) * 2.0 ** -32) * s
            worst = max(worst, abs(Fraction(c) - means[key][a]))
    print("\n%s: worst distance from the exact mean %.3e, bound %.3e" % (case, float(worst), float(bound)))
    assert worst <= bound
    # and the stored binary32 is that centroid rounded once
    order = sorted(groups, key=lambda key: groups[key][0])
    for n, key in enumerate(order[:200]):
        ks = groups[key]
        c = [o[a] + (key[a] + (float(sum(int(q[k, a]) for k in ks)) / float(len(ks))) * 2.0 ** -32) * s for a in range(3)]
        assert got["xyz"][n].tolist() == np.array(c, np.float64).astype(np.float32).tolist() and got["first_index"][n] == ks[0]


def test_a_shuffled_input_gives_the_same_centroid_set(tmp_path):
    xyz, prep = CASES["voxel_shared"]
    rng = np.random.default_rng(4)
    order = rng.permutation(len(xyz))
    rc, err, plain = P.serial(xyz, tmp_path, **prep)
    assert rc == 0, err
    rc, err, mixed = P.serial(xyz[order], tmp_path, **prep)
    assert rc == 0, err
    rows = lambda a: sorted(map(bytes, a.view(np.uint8).reshape(len(a), 12)))
    assert rows(plain["xyz"]) == rows(mixed["xyz"]) and len(plain["xyz"]) == 1250
    assert (np.diff(mixed["first_index"]) > 0).all() and not np.array_equal(plain["xyz"], mixed["xyz"])
    # the first point of every voxel in the new order
    _, i, _ = P.voxel_parts(xyz[order].astype(np.float64), prep["voxel"])
    _, first = np.unique(i, axis=0, return_index=True)
    assert sorted(first.tolist()) == mixed["first_index"].tolist()


# ---- the two readers ----------------------------------------------------------------------------------------------------------------
def read(which, tmp_path, text=None, path=None):
    if path is None:
        path = str(tmp_path / ("in." + which))
        with open(path, "w") as f:
            f.write(text)
    out = P.run_program(which, path)
    return out.returncode, out.stdout, out.stderr


def test_transform_reader(tmp_path):
    rc, out, err = read("transform", tmp_path, path=os.path.join(GOLDEN, "trans.txt"))
    assert rc == 0, err
    want = np.loadtxt(os.path.join(GOLDEN, "trans.txt"))
    assert [float.fromhex(w) for w in out.split()] == want.reshape(-1).tolist() and want[3].tolist() == [0, 0, 0, 1]
    m = np.arange(16, dtype=np.float64).reshape(4, 4) * 0.3
    m[3] = [0, 0, 0, 1]
    np.savetxt(str(tmp_path / "m.txt"), m)
    rc, out, err = read("transform", tmp_path, path=str(tmp_path / "m.txt"))
    assert rc == 0 and [float.fromhex(w) for w in out.split()] == m.reshape(-1).tolist()
    one_line = " ".join(repr(float(v)) for v in m.reshape(-1))
    assert read("transform", tmp_path, one_line)[0] == 0
    for text, say in ((" ".join(["1"] * 15), "holds 15 numbers; a transform is 16"), (" ".join(["1"] * 17), "holds 17 numbers"), ("", "holds 0 numbers"),
                      (one_line.replace("0.3", "0.3x", 1), "`0.3x` is not a number"), (" ".join(["1"] * 16), "last row must be 0 0 0 1, got 1 1 1 1"),
                      ("1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 2", "last row must be 0 0 0 1"), ("1 0 0 nan 0 1 0 0 0 0 1 0 0 0 0 1", "non-finite entry"),
                      ("1 0 0 0 0 inf 0 0 0 0 1 0 0 0 0 1", "non-finite entry")):
        rc, out, err = read("transform", tmp_path, text)
        assert rc == 2 and say in err and out == "", (text, err)
    rc, out, err = read("transform", tmp_path, path=str(tmp_path / "absent.txt"))
    assert rc == 2 and "cannot read" in err


CROP = '{"axis_max": 2.5, "axis_min": -1e-1, "bounding_polygon": [[0, 0, 9], [1.5, 0, 9], [0, 2E0, 9]], "class_name": "SelectionPolygonVolume", "orthogonal_axis": "Y", "version_major": 1}'


def test_crop_reader(tmp_path):
    rc, out, err = read("crop", tmp_path, path=os.path.join(GOLDEN, "crop.json"))
    assert rc == 0, err
    rows = [ln.split() for ln in out.splitlines()]
    assert rows[0][0] == "2" and [float.fromhex(w) for w in rows[0][1:3]] == [0.1, 0.8] and rows[0][3] == "12"
    assert [[float.fromhex(w) for w in r[:2]] for r in rows[1:]] == P.CONCAVE_12
    rc, out, err = read("crop", tmp_path, CROP)
    assert rc == 0, err
    rows = [ln.split() for ln in out.splitlines()]
    assert rows[0][0] == "1" and [float.fromhex(w) for w in rows[0][1:3]] == [-0.1, 2.5] and [[float.fromhex(w) for w in r] for r in rows[1:]] == [[0, 0, 9], [1.5, 0, 9], [0, 2, 9]]
    # other keys are ignored, whatever they hold
    assert read("crop", tmp_path, CROP.replace('"version_major": 1', r'"extra": {"a": [true, false, null, "q\"é\n"], "b": {}}, "c": []'))[0] == 0
    vertices = lambda n: ", ".join("[%d, %d, 0]" % (k, k * k) for k in range(n))
    assert read("crop", tmp_path, CROP.replace("[0, 0, 9], [1.5, 0, 9], [0, 2E0, 9]", vertices(256)))[0] == 0
    for text, say in ((CROP[:-1], "malformed JSON at byte"), (CROP.replace('"axis_min": -1e-1,', '"axis_min": -1e-1'), "malformed JSON at byte 36: expected `,` or `}`"),
                      (CROP + " x", "expected the end of the file"), (CROP.replace("2.5", "2.5.1"), "malformed JSON"), (CROP.replace("2.5", "+2.5"), "malformed JSON"),
                      (CROP.replace("2.5", "nan"), "malformed JSON"), ("[1, 2]", "expected an object"), ("", "malformed JSON at byte 0"),
                      (CROP.replace('"axis_min"', '"axis_mim"'), "the field `axis_min` is missing"), (CROP.replace('"axis_max"', '"axis_mux"'), "the field `axis_max` is missing"),
                      (CROP.replace('"orthogonal_axis"', '"axis"'), "the field `orthogonal_axis` is missing"),
                      (CROP.replace('"bounding_polygon"', '"polygon"'), "the field `bounding_polygon` is missing"),
                      (CROP.replace(", [0, 2E0, 9]", ""), "bounding_polygon needs at least 3 vertices, got 2"),
                      (CROP.replace("[0, 0, 9], [1.5, 0, 9], [0, 2E0, 9]", vertices(257)), "bounding_polygon takes at most 256 vertices, got 257"),
                      (CROP.replace('"Y"', '"W"'), 'orthogonal_axis must be "X", "Y" or "Z"'), (CROP.replace('"Y"', "1"), "orthogonal_axis must be"),
                      (CROP.replace("[1.5, 0, 9]", "[1.5, 0]"), "bounding_polygon vertex 1 must hold 3 numbers"),
                      (CROP.replace("[1.5, 0, 9]", '[1.5, "0", 9]'), "bounding_polygon vertex 1 must hold 3 numbers"),
                      (CROP.replace("2.5", '"2.5"'), "axis_min and axis_max must be numbers"), (CROP.replace("2.5", "-2.5"), "axis_min (-0.1) must not exceed axis_max (-2.5)"),
                      (CROP.replace("1.5", "1e999"), "non-finite coordinate")):
        rc, out, err = read("crop", tmp_path, text)
        assert rc == 2 and say in err and out == "", (text, err)


def test_refused_descriptions(tmp_path):
    xyz = P.cloud(np.random.default_rng(1).random((10, 3)))
    square = P.polygon_3d(2, P.BIG_SQUARE)
    bad_row, nan_m = np.eye(4), np.eye(4)
    bad_row[3, 0] = 1e-300
    nan_m[1, 2] = np.nan
    for prep, say in ((P.prep(transform=bad_row.reshape(-1)), "last row must be 0 0 0 1"), (P.prep(transform=nan_m.reshape(-1)), "non-finite entry"),
                      (P.prep(crop=P.crop_of(2, 0, 1, square[:2])), "at least 3 vertices, got 2"),
                      (P.prep(crop=P.crop_of(2, 0, 1, np.zeros((257, 3)))), "at most 256 vertices, got 257"),
                      (P.prep(crop=P.crop_of(2, 1, 0, square)), "axis_min (1) must not exceed axis_max (0)"), (P.prep(crop=P.crop_of(2, np.nan, 0, square)), "must not exceed"),
                      (P.prep(crop=P.crop_of(3, 0, 1, square)), "crop_axis must be"), (P.prep(voxel=-0.5), "voxel must be finite and positive"),
                      (P.prep(voxel=np.nan), "voxel must be finite and positive"), (P.prep(voxel=np.inf), "voxel must be finite and positive"),
                      (P.prep(voxel=1e-7), "voxels of edge 1e-07; at most 2097150 are supported")):
        rc, err, got = P.serial(xyz, tmp_path, **prep)
        assert rc == 3 and say in err, (prep, err)


def test_apd_refuses_bad_files_and_options(tmp_path):
    apd = os.path.join(ROOT, "dvp-mvs_amd", "apd")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    import np_evaluate as N
    ply = str(tmp_path / "a.ply")
    N.write_ply_like_apd(ply, np.random.default_rng(2).random((50, 3)))
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("1 2 3")
    run = lambda *a: subprocess.run([apd, "--evaluate", ply, "--against", ply, "--evaluate-on", "host"] + list(a), capture_output=True, text=True, timeout=120)
    out = run("--transform", bad)
    assert out.returncode == 1 and "holds 3 numbers; a transform is 16" in out.stderr and out.stdout == ""
    out = run("--crop", bad)
    assert out.returncode == 1 and "malformed JSON" in out.stderr and out.stdout == ""
    for v in ("0", "-1", "nan", "x"):
        out = run("--voxel-size", v)
        assert out.returncode == 1 and "--voxel-size takes a finite, positive number" in out.stderr
    out = run("--save-prepared", str(tmp_path / "p_"))
    assert out.returncode == 1 and "--save-prepared needs" in out.stderr
    # the host flavour end to end: the fixture files, the two new report lines, the saved clouds
    out = run("--transform", os.path.join(GOLDEN, "trans.txt"), "--crop", os.path.join(GOLDEN, "crop.json"), "--voxel-size", "0.05", "--save-prepared", str(tmp_path / "p_"))
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[2].startswith("prepared reconstruction: 50 finite, ") and lines[3].startswith("prepared ground_truth: 50 finite, ") and lines[4] == "tolerance accuracy completeness f1"
    N.build_program()
    rc, err, saved = N.read_ply(str(tmp_path / "p_truth.ply"), tmp_path)
    assert rc == 0 and lines[3].endswith(", %d points" % len(saved)) and lines[1] == "ground_truth %s %d points (0 skipped)" % (ply, len(saved))
    plain = subprocess.run([apd, "--evaluate", ply, "--against", ply, "--evaluate-on", "host"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and len(plain.stdout.splitlines()) == 9 and "prepared" not in plain.stdout
