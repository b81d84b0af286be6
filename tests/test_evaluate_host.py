"""`apd --evaluate` without a GPU: the serial text of csrc/dvp_cloudeval.hpp (tests/cloudeval_host), both as the double loop and as
the grid walk, equals the numpy restatement (tests/np_evaluate.py) bit for bit on d2 and exactly on the counts, on the case table and
on 4 000 x 4 000 random points; scipy's cKDTree in float64 gives the same counts on that random case, where no nearest distance lies
within a relative 1e-5 of a tolerance; the PLY reader reads the writer's bytes, ascii, doubles with normals and extra properties, a
face element after the vertices, and refuses the rest with a message that says which; the sub-command with --evaluate-on host."""
import os
import subprocess

import numpy as np
import pytest

import np_evaluate as N
from conftest import ROOT

pytestmark = pytest.mark.hostbox

CASES = N.cases()
APD = os.path.join(ROOT, "dvp-mvs_amd", "apd")
RANDOM_SEED = 5      # the nearest distances of this seed keep a relative 1.5e-4 clear of every tolerance (checked in the k-d tree test)


@pytest.fixture(scope="module", autouse=True)
def built():
    N.build_program()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])


@pytest.fixture(scope="module")
def random_case():
    recon, truth, tol = N.random_scene(RANDOM_SEED)
    return recon, truth, tol, N.evaluate(recon, truth, tol)


@pytest.mark.parametrize("mode", ["brute", "grid"])
@pytest.mark.parametrize("case", list(CASES))
def test_serial_text_equals_numpy(tmp_path, case, mode):
    recon, truth, tol = CASES[case]
    rc, err, got = N.serial(recon, truth, tol, tmp_path, mode)
    assert rc == 0, err
    assert N.same_result(got, N.evaluate(recon, truth, tol)) == ""


def test_the_case_table_holds_what_it_says(tmp_path):
    # corners: the nearest target of query n is the one across the cell border, in each of the 26 neighbour cells once
    recon, truth, tol = CASES["corners"]
    origin, h = N.grid_of(recon, truth, tol[-1])
    d = np.linalg.norm(recon[:, None, :].astype(np.float64) - truth[None, :, :].astype(np.float64), axis=2)
    nearest = d.argmin(1)
    assert list(nearest) == [2 + 2 * n for n in range(26)]
    step = N.cell_indices(truth[nearest], origin, h) - N.cell_indices(recon, origin, h)
    assert len({tuple(s) for s in step}) == 26 and (np.abs(step).max(1) == 1).all()
    assert (N.cell_indices(truth[nearest + 1], origin, h) == N.cell_indices(recon, origin, h)).all()      # the farther one: in the query's cell
    # thresholds: exactly T is kept, one ulp beyond is not
    assert N.evaluate(*CASES["at_T"])["d2_recon"].tolist() == [0.25, 0.25]
    assert np.isinf(N.evaluate(*CASES["beyond_T"])["d2_recon"]).all()
    # table: 8192 points make the smallest capacity, 16384; at least 5 000 cells; two cells with one home slot, as the tool has it
    recon, truth, tol = CASES["table"]
    origin, h = N.grid_of(recon, truth, tol[-1])
    pts = np.concatenate([recon, truth])
    assert len(pts) == 8192 and N.table_capacity(len(pts)) == 16384
    keys, first = np.unique(N.cell_keys(pts, origin, h), return_index=True)
    assert len(keys) >= 5000
    home = N.hash_keys(keys) & np.uint64(16383)
    order = np.argsort(home, kind="stable")
    twin = np.flatnonzero(home[order][1:] == home[order][:-1])[0]
    a, b = first[order[twin]], first[order[twin + 1]]
    slot_a, slot_b = N.home_slot(recon, truth, tol[-1], pts[a], tmp_path), N.home_slot(recon, truth, tol[-1], pts[b], tmp_path)
    assert slot_a[0] == 16384 and slot_a[:2] == slot_b[:2] and slot_a[2] != slot_b[2]
    assert slot_a[1] == int(home[order[twin]]) and slot_a[2] == int(keys[order[twin]])
    # contention: the 3 x 3 x 3 block
    recon, truth, tol = N.contention_scene()
    origin, h = N.grid_of(recon, truth, tol[-1])
    assert N.cell_indices(truth, origin, h).max() <= 3 and len(truth) == 20000


@pytest.mark.parametrize("mode", ["brute", "grid"])
def test_random_clouds_equal_numpy(tmp_path, random_case, mode):
    recon, truth, tol, want = random_case
    rc, err, got = N.serial(recon, truth, tol, tmp_path, mode)
    assert rc == 0, err
    assert N.same_result(got, want) == ""
    assert 0 < want["within_recon"][2] < want["within_recon"][4] <= 4000


def test_random_clouds_against_a_kd_tree(random_case):
    """an independent reading: scipy's cKDTree in float64.  No nearest distance lies within a relative 1e-5 of a tolerance (the seed
    is chosen so), so the binary32 roundings cannot move a point across one, and no point is excused."""
    from scipy.spatial import cKDTree
    recon, truth, tol, want = random_case
    for query, target, key in ((recon, truth, "within_recon"), (truth, recon, "within_truth")):
        d, _ = cKDTree(target.astype(np.float64)).query(query.astype(np.float64))
        for k, t in enumerate(tol):
            t64 = float(np.float32(t))
            assert (np.abs(d - t64) > 1e-5 * t64).all(), (key, t)
            assert int((d <= t64).sum()) == want[key][k], (key, t)


def test_refused_inputs(tmp_path):
    a = N.cloud([[0, 0, 0], [1, 1, 1]])
    for tol, message in (([0.1, 0.1], "strictly ascending"), ([0.0], "finite and positive"), ([-1.0], "finite and positive"), ([1e-30], "normal binary32 square"),
                         ([float("inf")], "finite and positive"), ([1e30], "finite and positive"), (list(np.linspace(0.1, 0.9, 9)), "num_tol must be 1 ... 8")):
        rc, err, _ = N.serial(a, a, tol, tmp_path)
        assert rc == 3 and message in err, (tol, err)
    # the extent limit: 2^21 - 2 cells of the largest tolerance along an axis
    far = N.cloud([[0, 0, 0], [0, 30000, 0]])
    rc, err, _ = N.serial(a, far, [0.01], tmp_path)
    assert rc == 3 and "30000" in err and "axis 1" in err and "0.00999999978" in err and "2097150" in err, err
    rc, err, _ = N.serial(a, far, [0.01, 0.02], tmp_path)
    assert rc == 0, err
    # at most 2^30 finite points in both clouds together: a slot of the table, 2^31 at the most, is kept in 32 bits per point
    out = N.run_program("binned", 2 ** 30)
    assert out.returncode == 0 and out.stdout.split() == [str(2 ** 31)], out.stderr
    out = N.run_program("binned", 2 ** 30 + 1)
    assert out.returncode == 3 and "1073741825 points with finite coordinates together; at most 1073741824 (2^30)" in out.stderr, out.stderr


def test_contention_scene_equals_numpy(tmp_path):
    """the reference of the device's contention test, against the double loop in numpy, which shares no grid or table code with it"""
    recon, truth, tol = N.contention_scene()
    rc, err, got = N.serial(recon, truth, tol, tmp_path, "grid")
    assert rc == 0, err
    assert N.same_result(got, N.evaluate(recon, truth, tol)) == ""


# ---- the PLY reader -----------------------------------------------------------------------------------------------------------
def _ply(tmp_path, name, header_lines, body):
    f = str(tmp_path / name)
    with open(f, "wb") as out:
        out.write(("\n".join(header_lines) + "\n").encode() + body)
    return f


def test_ply_reader_reads(tmp_path):
    rng = np.random.default_rng(2)
    xyz = N.cloud(rng.normal(0, 3, (77, 3)))
    # our own writer's bytes
    f = str(tmp_path / "apd.ply")
    N.write_ply_like_apd(f, xyz, rng.integers(0, 255, (77, 3)))
    rc, err, got = N.read_ply(f, tmp_path)
    assert rc == 0 and N.same_bits(got, xyz), err
    # ascii, with a comment, CR LF line ends, an extra property and nan / inf
    rows = xyz.copy()
    rows[5, 1], rows[6, 2] = np.nan, -np.inf
    text = "".join("%.9g %d %.9g %.9g\r\n" % (p[0], i, p[1], p[2]) for i, p in enumerate(rows))
    f = _ply(tmp_path, "ascii.ply", ["ply\r", "format ascii 1.0\r", "comment made by a test\r", "element vertex 77\r", "property float x\r", "property int id\r", "property float y\r",
                                     "property float z\r", "end_header\r"], text.encode())
    rc, err, got = N.read_ply(f, tmp_path)
    assert rc == 0 and N.same_bits(got, rows), err
    # doubles, normals and extra properties of every size, x y z not in order; a fixed-size element before and a face element after
    wide = rng.normal(0, 100, (77, 3))
    rec = np.zeros(77, np.dtype([("nx", "<f4"), ("z", "<f8"), ("flag", "u1"), ("x", "<f8"), ("ny", "<f4"), ("level", "<i2"), ("y", "<f8"), ("nz", "<f4"), ("stamp", "<f8")]))
    rec["x"], rec["y"], rec["z"] = wide[:, 0], wide[:, 1], wide[:, 2]
    rec["flag"], rec["level"] = 255, -2
    header = ["ply", "format binary_little_endian 1.0", "obj_info scanner", "element station 2", "property double height", "property uchar kind", "element vertex 77",
              "property float nx", "property double z", "property uchar flag", "property double x", "property float ny", "property short level", "property double y",
              "property float nz", "property double stamp", "element face 3", "property list uchar int vertex_indices", "end_header"]
    faces = b"".join(bytes([3]) + np.array(t, "<i4").tobytes() for t in ((0, 1, 2), (2, 3, 4), (4, 5, 6)))
    f = _ply(tmp_path, "scan.ply", header, bytes(18) + rec.tobytes() + faces)
    rc, err, got = N.read_ply(f, tmp_path)
    assert rc == 0 and N.same_bits(got, wide.astype(np.float32)), err      # a double is rounded to binary32
    # no vertices at all
    f = _ply(tmp_path, "none.ply", ["ply", "format ascii 1.0", "element vertex 0", "property float x", "property float y", "property float z", "end_header"], b"")
    rc, err, got = N.read_ply(f, tmp_path)
    assert rc == 0 and got.shape == (0, 3), err


def test_ply_reader_refuses(tmp_path):
    xyz = ["property float x", "property float y", "property float z"]
    body = np.zeros(9, "<f4").tobytes()
    for name, header, data, message in (
            ("big", ["ply", "format binary_big_endian 1.0", "element vertex 3"] + xyz + ["end_header"], body, "binary_big_endian is not supported"),
            ("list", ["ply", "format binary_little_endian 1.0", "element vertex 3"] + xyz + ["property list uchar int seen_by", "end_header"], body, "list property `seen_by` in element vertex"),
            ("before", ["ply", "format binary_little_endian 1.0", "element face 1", "property list uchar int vertex_indices", "element vertex 3"] + xyz + ["end_header"], body,
             "list property `vertex_indices` in element face, which comes before element vertex"),
            ("short", ["ply", "format binary_little_endian 1.0", "element vertex 4"] + xyz + ["end_header"], body + bytes(5), "the body is short: 3 of 4 vertices"),
            ("short_huge", ["ply", "format binary_little_endian 1.0", "element vertex 2147483647"] + xyz + ["end_header"], body, "the body is short: 3 of 2147483647 vertices"),
            ("short_huge_ascii", ["ply", "format ascii 1.0", "element vertex 2147483647"] + xyz + ["end_header"], b"1 2 3\n4 5 6\n7\n", "the body is short: 2 of 2147483647 vertices"),
            ("short_ascii", ["ply", "format ascii 1.0", "element vertex 2"] + xyz + ["end_header"], b"1 2 3\n4 5\n", "the body is short: 1 of 2 vertices"),
            ("no_x", ["ply", "format binary_little_endian 1.0", "element vertex 3", "property float y", "property float z", "end_header"], body, "no property x"),
            ("no_y", ["ply", "format binary_little_endian 1.0", "element vertex 3", "property float x", "property float z", "end_header"], body, "no property y"),
            ("no_z", ["ply", "format binary_little_endian 1.0", "element vertex 3", "property float x", "property float y", "end_header"], body, "no property z"),
            ("int_x", ["ply", "format binary_little_endian 1.0", "element vertex 3", "property int x", "property float y", "property float z", "end_header"], body, "property x of element vertex is int"),
            ("no_vertex", ["ply", "format ascii 1.0", "element point 3"] + xyz + ["end_header"], b"", "no element vertex"),
            ("not_ply", ["plz", "format ascii 1.0"], b"", "not a PLY file"),
            ("no_end", ["ply", "format ascii 1.0", "element vertex 0"] + xyz, b"", "no end_header")):
        f = _ply(tmp_path, name + ".ply", header, data)
        rc, err, got = N.read_ply(f, tmp_path)
        assert rc == 2 and message in err and f in err, (name, err)
    rc, err, _ = N.read_ply(str(tmp_path / "missing.ply"), tmp_path)
    assert rc == 2 and "cannot be opened" in err


# ---- the sub-command ----------------------------------------------------------------------------------------------------------
def apd_evaluate(*args):
    return subprocess.run([APD, "--evaluate"] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def report_rows(text):
    lines = text.splitlines()
    assert lines[0].split()[0] == "reconstruction" and lines[1].split()[0] == "ground_truth" and lines[2] == "tolerance accuracy completeness f1", text
    return [ln.split() for ln in lines[3:]]


def test_sub_command_on_the_host(tmp_path):
    rng = np.random.default_rng(4)
    i = np.arange(5000)      # a lattice 0.04 apart in x and y, two layers 0.1 apart: a point's shifted copy is the nearest by far
    xyz = N.cloud(np.stack([0.04 * (i % 50), 0.04 * ((i // 50) % 50), 0.1 * (i // 2500)], 1))
    xyz[17, 1] = np.nan
    a, b, c = str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), str(tmp_path / "c.ply")
    N.write_ply_like_apd(a, xyz)
    N.write_ply_like_apd(b, xyz + np.float32([0, 0, 0.015]))      # 1.5 x the smallest tolerance along z; the next tolerance is 2 x
    other = N.cloud(rng.random((4500, 3)) * [2, 2, 0.2])
    N.write_ply_like_apd(c, other)
    # a cloud against itself
    out = apd_evaluate(a, "--against", a, "--evaluate-on", "host", "--out", tmp_path / "self.txt")
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines()[0] == "reconstruction %s 4999 points (1 skipped)" % a and out.stdout.splitlines()[1] == "ground_truth %s 4999 points (1 skipped)" % a
    rows = report_rows(out.stdout)
    assert [r[0] for r in rows] == ["0.00999999978", "0.0199999996", "0.0500000007", "0.100000001", "0.200000003", "0.5"]
    assert all(r[1:] == ["100.000000"] * 3 for r in rows), rows
    assert open(tmp_path / "self.txt").read() == out.stdout
    # ... against its shifted copy
    out = apd_evaluate(a, "--against", b, "--evaluate-on", "host")
    rows = report_rows(out.stdout)
    assert rows[0][1:] == ["0.000000"] * 3 and all(r[1:] == ["100.000000"] * 3 for r in rows[1:]), rows
    # ... against another cloud: the figures never decrease with the tolerance, and are the counts' quotients
    tol = [0.01, 0.03, 0.1, 0.3]
    out = apd_evaluate(a, "--against", c, "--evaluate-on", "host", "--tolerances", "0.01,0.03,0.1,0.3")
    assert out.returncode == 0, out.stderr
    rows = report_rows(out.stdout)
    want = N.evaluate(xyz, other, tol)
    for k, r in enumerate(rows):
        acc, comp = want["within_recon"][k] / 4999, want["within_truth"][k] / 4500
        assert r == ["%.9g" % np.float32(tol[k]), "%.6f" % (100 * acc), "%.6f" % (100 * comp), "%.6f" % (100 * (2 * acc * comp / (acc + comp) if acc + comp else 0.0))], (k, r)
    figures = np.array([[float(v) for v in r[1:]] for r in rows])
    assert (np.diff(figures, axis=0) >= 0).all() and 0 < figures[1, 0] < figures[3, 0]


def test_sub_command_usage_errors(tmp_path):
    a = str(tmp_path / "a.ply")
    N.write_ply_like_apd(a, N.cloud([[0, 0, 0]]))
    for args, message in ((("--against", a, "--evaluate-on", "cpu"), "--evaluate-on takes gpu or host"), (("--against", a, "--voxel", "0.1"), "unknown option --voxel"),
                          (("--against",), "--against takes a value"), ((), "--against is required"), (("--against", a, "--tolerances", "0.1,x"), "--tolerances takes numbers"),
                          (("--against", a, "--tolerances", "1,2,3,4,5,6,7,8,9"), "1 to 8 numbers")):
        out = apd_evaluate(a, *args)
        assert out.returncode == 1 and message in out.stderr, (args, out.stderr)
    out = subprocess.run([APD, "--evaluate"], capture_output=True, text=True)
    assert out.returncode == 1 and "USAGE: apd --evaluate" in out.stderr
    out = apd_evaluate(a, "--against", a, "--evaluate-on", "host", "--tolerances", "0.2,0.1")
    assert out.returncode == 1 and "strictly ascending" in out.stderr
    out = apd_evaluate(a, "--against", str(tmp_path / "none.ply"), "--evaluate-on", "host")
    assert out.returncode == 1 and "cannot be opened" in out.stderr
    # a truncated file that claims 2^31 - 1 vertices is told so; the count is not trusted with memory
    cut = _ply(tmp_path, "cut.ply", ["ply", "format binary_little_endian 1.0", "element vertex 2147483647", "property float x", "property float y", "property float z", "end_header"], bytes(24))
    out = apd_evaluate(a, "--against", cut, "--evaluate-on", "host")
    assert out.returncode == 1 and "the body is short: 2 of 2147483647 vertices" in out.stderr, out.stderr
