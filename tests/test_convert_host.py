"""`apd --convert-from` without a GPU: host/colmap.cpp's readers, cameras, formatter and writers, and the text of
csrc/dvp_pairs.hpp run serially by tests/convert_host/convert_host, against
  * tests/golden/convert: a synthetic COLMAP model and the pair.txt and cams/ the reference's own converter wrote from it
    (tools/make_convert_golden.py says under which conditions those files do not depend on sort stability or summation order);
  * np_convert: an independent numpy reading that sorts the angles as calc_score does;
  * Python's own str(float)."""
import os
import shutil
import struct

import numpy as np
import pytest

import np_convert as N

pytestmark = pytest.mark.hostbox

MODEL = os.path.join(N.GOLDEN, "model")
NV = 6
SCORE_CASES = N.score_cases()


def golden(name):
    return open(os.path.join(N.GOLDEN, name)).read()


_CONVERTED = {}


def converted(tmp_path_factory, ext, *extra):
    """the folder convert_host model leaves for the fixture model, made once per argument set"""
    key = (ext,) + extra
    if key not in _CONVERTED:
        d = str(tmp_path_factory.mktemp("converted") / "save")
        out = N.run_program("model", MODEL, d, ext, *extra)
        assert out.returncode == 0, out.stderr
        _CONVERTED[key] = d
    return _CONVERTED[key]


@pytest.mark.parametrize("ext", [".txt", ".bin"])
def test_pair_txt_is_the_references(tmp_path_factory, ext):
    d = converted(tmp_path_factory, ext)
    assert open(os.path.join(d, "pair.txt")).read() == golden("pair.txt")


@pytest.mark.parametrize("ext", [".txt", ".bin"])
def test_cams_meet_the_references(tmp_path_factory, ext):
    d = converted(tmp_path_factory, ext)
    assert sorted(os.listdir(os.path.join(d, "cams"))) == ["%08d_cam.txt" % i for i in range(NV)]
    for i in range(NV):
        got = N.parse_cam(open(os.path.join(d, "cams", "%08d_cam.txt" % i)).read())
        want = N.parse_cam(golden("cams/%08d_cam.txt" % i))
        assert got[1] == want[1] and got[2] == want[2], i               # the intrinsic and the depth-range lines: byte for byte
        assert got[0][3] == want[0][3] == ["0.0", "0.0", "0.0", "1.0", ""]
        for r in range(3):
            assert got[0][r][3:] == want[0][r][3:], (i, r)                 # the translation: identical
            for c in range(3):
                # three terms of magnitude at most 2, each rounded once; numpy's scalar ** 2 need not be correctly rounded
                assert abs(float(got[0][r][c]) - float(want[0][r][c])) <= 1e-15, (i, r, c)
                assert got[0][r][c] == repr(float(got[0][r][c]))


def test_scale_factor_and_interval_scale(tmp_path_factory):
    d = converted(tmp_path_factory, ".txt", "2", "64", "0.5")
    cameras, images, _ = N.read_model(MODEL, ".txt")
    for i, im in enumerate(images):
        _, K, last = N.parse_cam(open(os.path.join(d, "cams", "%08d_cam.txt" % i)).read())
        name, p = cameras[im[3]]
        fx, fy, cx, cy = (p[0], p[0], p[1], p[2]) if name == "SIMPLE_RADIAL" else p[:4]
        assert K == [[repr(fx / 2.0), "0.0", repr(cx / 2.0), ""], ["0.0", repr(fy / 2.0), repr(cy / 2.0), ""], ["0.0", "0.0", "1.0", ""]]
        dmin, _, _, dmax = [float(v) for v in N.parse_cam(golden("cams/%08d_cam.txt" % i))[2].split()]
        got = [float(v) for v in last.split()]
        assert got[0] == dmin and got[3] == dmax and got[2] == 64.0
        assert abs(got[1] - (dmax - dmin) / 63 / 0.5) <= 2e-6           # (from the six decimals of the fixture's range)
    assert open(os.path.join(d, "pair.txt")).read() == golden("pair.txt")


def test_max_d_zero_takes_the_inverse_depth_rule(tmp_path_factory):
    d = converted(tmp_path_factory, ".txt", "1", "0")
    cameras, images, points = N.read_model(MODEL, ".txt")
    for i, im in enumerate(images):
        _, K, last = N.parse_cam(open(os.path.join(d, "cams", "%08d_cam.txt" % i)).read())
        dmin, interval, num, dmax = [float(v) for v in last.split()]
        # colmap2mvsnet.py:386-400 in numpy, from the written camera
        Kf = np.array([[float(v) for v in row[:3]] for row in K])
        R, t = np.array(N.rotation(im[1])), np.array(im[2])
        zs = sorted((R @ np.array(points[p][0]) + t)[2] for p in im[6] if p != -1)
        lo, hi = zs[int(len(zs) * .01)] * 0.75, zs[int(len(zs) * .99)] * 1.25
        P1 = np.linalg.inv(R) @ (np.linalg.inv(Kf) @ [Kf[0, 2], Kf[1, 2], 1] * lo - t)
        P2 = np.linalg.inv(R) @ (np.linalg.inv(Kf) @ [Kf[0, 2] + 1, Kf[1, 2], 1] * lo - t)
        want_num = (1 / lo - 1 / hi) / (1 / lo - 1 / (lo + np.linalg.norm(P2 - P1)))
        assert abs(dmin - lo) <= 1e-6 and abs(dmax - hi) <= 1e-6
        assert abs(num - want_num) <= 1e-6 * want_num + 1e-6 and abs(interval - (hi - lo) / (want_num - 1)) <= 2e-6


def test_sfm_lines_hold_the_models_numbers(tmp_path_factory):
    cameras, images, points = N.read_model(MODEL, ".bin")
    for ext, F in ((".txt", 1.0), (".bin", 1.0), (".txt", 2.0)):
        d = converted(tmp_path_factory, ext, *(() if F == 1.0 else ("2", "64", "0.5")))
        assert sorted(os.listdir(os.path.join(d, "sfm"))) == ["%08d.txt" % i for i in range(NV)]
        for i, im in enumerate(images):
            want = ["%s %s %s %s %s %d %d %d" % ((repr(float(x / F)), repr(float(y / F))) + tuple(repr(v) for v in points[p][0]) + tuple(points[p][1]))
                    for (x, y), p in zip(im[5], im[6]) if p != -1]
            assert open(os.path.join(d, "sfm", "%08d.txt" % i)).read() == "".join(l + "\n" for l in want), (ext, i)
            assert len(want) > 50


def test_both_formats_read_the_same_model():
    a, b = N.read_model(MODEL, ".txt"), N.read_model(MODEL, ".bin")
    assert a[0] == b[0] and a[2] == b[2] and [im[0] for im in a[1]] == [3, 7, 8, 12, 20, 21]
    for x, y in zip(a[1], b[1]):
        assert x[:5] == y[:5] and np.array_equal(x[5], y[5]) and np.array_equal(x[6], y[6])


def test_float_formatter_equals_pythons_str(tmp_path):
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 64, 7000, dtype=np.uint64).view(np.float64)
    vals = np.concatenate([bits[np.isfinite(bits)][:6000], rng.normal(0, 1, 1500), rng.normal(0, 1, 1500) * 10.0 ** rng.integers(-8, 20, 1500),
                           np.round(rng.normal(0, 100, 500), 2), rng.integers(-10 ** 17, 10 ** 17, 500).astype(np.float64),
                           [1e16, 1e-4, 9.999e-5, 0.1, -0.0, 5e-324, 0.0, 1.0, 1e15, 9999999999999998.0, 1.7976931348623157e308, 2.2250738585072014e-308, 123456.0, 1e22, 1e-5,
                            float("inf"), float("-inf"), float("nan")]])
    assert vals.size >= 10000
    src, dst = str(tmp_path / "v.in"), str(tmp_path / "v.out")
    vals.tofile(src)
    out = N.run_program("fmt", src, dst)
    assert out.returncode == 0, out.stderr
    got = open(dst).read().split("\n")[:-1]
    want = [str(float(v)) for v in vals]
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not bad, bad[:5]


@pytest.mark.parametrize("case", list(SCORE_CASES))
def test_serial_scores_equal_the_numpy_reading(tmp_path, case):
    m = SCORE_CASES[case]
    rc, err, got = N.serial_scores(m, tmp_path)
    assert rc == 0, err
    want = N.scores(m)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(got, got.T) and not np.diag(got).any()


def test_score_cases_say_what_they_claim():
    c = SCORE_CASES
    for S, L in ((1, 0), (1, 1), (4, 3), (4, 4), (8, 6), (8, 7)):
        m = c["s%d_l%d" % (S, L)]
        th = N.pair_angles(m, 0, 1)
        assert th.size == S and int((th < 1).sum()) == L
        assert N.scores(m)[0, 1] == (0 if L > (3 * S) >> 2 else S)
        assert N.scores(m)[0, 2] == 0 and N.pair_angles(m, 0, 2).size == 0      # S = 0
    assert (N.scores(c["close"]) == 0).all() and all(N.pair_angles(c["close"], 0, j).size > 0 for j in range(1, 6))
    for length in (63, 64, 65, 130):
        m = c["track%d" % length]
        counts = np.unique(m["ids"][m["ids"] != -1], return_counts=True)[1]
        assert counts.max() == length + 1                                         # the track of multiplicity 2
    m = c["mult"]
    assert max(np.unique(m["ids"][lo:hi][m["ids"][lo:hi] != -1], return_counts=True)[1].max() for lo, hi in zip(m["offsets"][:-1], m["offsets"][1:])) == 3
    m = c["all_minus_one"]
    assert (m["ids"][m["offsets"][2]:m["offsets"][3]] == -1).all() and m["offsets"][3] > m["offsets"][2] and not N.scores(m)[2].any()
    assert c["cosine_above_one"]["over"] == 3
    assert (N.pair_angles(c["cosine_above_one"], 0, 1) == 0).all() and N.scores(c["cosine_above_one"])[0, 1] == 0
    assert np.isnan(N.pair_angles(c["point_at_centre"], 0, 1)).sum() == 1 and N.scores(c["point_at_centre"])[0, 1] == 2
    assert SCORE_CASES["n2"]["centres"].shape == (2, 3) and SCORE_CASES["n3"]["centres"].shape == (3, 3)


def test_ties_go_to_the_higher_index(tmp_path):
    score = np.array([[0, 5, 5, 0, 7, 5], [5, 0, 0, 0, 0, 0], [5, 0, 0, 3, 3, 3], [0, 0, 3, 0, 9, 9], [7, 0, 3, 9, 0, 1], [5, 0, 3, 9, 1, 0]], np.uint32)
    src, dst = str(tmp_path / "s.in"), str(tmp_path / "s.out")
    open(src, "wb").write(np.array([6], np.int64).tobytes() + score.tobytes())
    assert N.run_program("pairs", src, dst).returncode == 0
    text = open(dst).read()
    assert text == N.pair_text(score)
    rows = text.split("\n")
    assert rows[0] == "6" and rows[1] == "0" and rows[2] == "5 4 7 5 5 2 5 1 5 3 0 "
    assert rows[4] == "5 0 5 5 0 4 0 3 0 2 0 "
    # more than 21 views: 20 entries
    big = np.arange(25 * 25, dtype=np.uint32).reshape(25, 25) % 7
    big = np.triu(big, 1) + np.triu(big, 1).T
    open(src, "wb").write(np.array([25], np.int64).tobytes() + big.astype(np.uint32).tobytes())
    assert N.run_program("pairs", src, dst).returncode == 0
    assert open(dst).read() == N.pair_text(big) and open(dst).read().split("\n")[2].startswith("20 ")


@pytest.mark.parametrize("w,h,pad_w,pad_h,F", N.IMAGE_CASES)
def test_nearest_neighbour_map(tmp_path, w, h, pad_w, pad_h, F):
    out_w, out_h = N.out_size(pad_w, pad_h, F)
    src = N.picture(w, h)
    rc, err, got = N.serial_image(src, pad_w, pad_h, out_w, out_h, tmp_path)
    assert rc == 0, err
    assert np.array_equal(got, N.convert_image(src, pad_w, pad_h, out_w, out_h))
    if F == 1.0:
        assert np.array_equal(got[:h, :w], src) and not got[h:].any() and not got[:, w:].any()


def test_nearest_neighbour_sizes_and_indices():
    assert N.out_size(13, 7, 2.0) == (6, 3) and N.out_size(17, 9, 1.5) == (11, 6)
    assert list(N.nearest_index(6, 13)) == [0, 2, 4, 6, 8, 10] and list(N.nearest_index(11, 17)) == [0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 15]


def broken(tmp_path, edit):
    d = str(tmp_path / "model")
    shutil.copytree(MODEL, d)
    edit(d)
    return d


def rewrite(file, fn):
    data = open(file, "rb").read()
    open(file, "wb").write(fn(data))


ERRORS = {
    "truncated_images_bin": (".bin", lambda d: rewrite(os.path.join(d, "images.bin"), lambda b: b[:len(b) // 2]), r"images\.bin: record \d+: truncated"),
    "truncated_points_bin": (".bin", lambda d: rewrite(os.path.join(d, "points3D.bin"), lambda b: b[:-5]), r"points3D\.bin: record 299: truncated"),
    "truncated_cameras_bin": (".bin", lambda d: rewrite(os.path.join(d, "cameras.bin"), lambda b: b[:40]), r"cameras\.bin: record 0: truncated"),
    "short_image_line": (".txt", lambda d: rewrite(os.path.join(d, "images.txt"), lambda b: b.replace(b" view_7.ppm", b"", 1)), r"images\.txt:\d+: a short line"),
    "short_observation_line": (".txt", lambda d: rewrite(os.path.join(d, "images.txt"), lambda b: b.replace(b" -1\n", b"\n", 1)), r"images\.txt:\d+: a short line"),
    "short_camera_line": (".txt", lambda d: rewrite(os.path.join(d, "cameras.txt"), lambda b: b.replace(b" 24.25\n", b"\n", 1)), r"cameras\.txt:3: a short line \(PINHOLE has 4 parameters\)"),
    "short_point_line": (".txt", lambda d: rewrite(os.path.join(d, "points3D.txt"), lambda b: b.rstrip(b"\n") + b"\n77777 1.0 2.0 3.0 1 2\n"), r"points3D\.txt:303: a short line"),
    "unknown_camera_model": (".txt", lambda d: rewrite(os.path.join(d, "cameras.txt"), lambda b: b.replace(b"PINHOLE", b"PINHOLE_2", 1)), r"cameras\.txt:3: unknown camera model PINHOLE_2"),
    "unknown_camera_model_bin": (".bin", lambda d: rewrite(os.path.join(d, "cameras.bin"), lambda b: b[:12] + struct.pack("<i", 11) + b[16:]), r"cameras\.bin: record 0: unknown camera model 11"),
    "malformed_number": (".txt", lambda d: rewrite(os.path.join(d, "images.txt"), lambda b: b.replace(b"\n21 ", b"\n21 x", 1)), r"images\.txt:4: a malformed number"),
    "dangling_point_id": (".txt", lambda d: rewrite(os.path.join(d, "points3D.txt"), lambda b: b"\n".join(b.split(b"\n")[:-3]) + b"\n"), r"images\.txt:\d+: observation \d+ of image \S+ names point \d+, which is not in points3D"),
    "dangling_point_id_bin": (".bin", lambda d: rewrite(os.path.join(d, "points3D.bin"), lambda b: struct.pack("<Q", 0)), r"images\.bin: record \d+: observation \d+ of image \S+ names point \d+, which is not in points3D"),
    "dangling_camera": (".txt", lambda d: rewrite(os.path.join(d, "cameras.txt"), lambda b: b"\n".join(b.split(b"\n")[:3]) + b"\n"), r"images\.txt:\d+: image \S+ names camera 2, which is not in the model"),
    "missing_file": (".txt", lambda d: os.remove(os.path.join(d, "points3D.txt")), r"cannot open .*points3D\.txt"),
    "bad_extension": (".json", lambda d: None, r"the model format must be \.txt or \.bin"),
}


@pytest.mark.parametrize("case", list(ERRORS))
def test_malformed_input_is_an_error_that_names_the_place(tmp_path, case):
    import re
    ext, edit, message = ERRORS[case]
    d = broken(tmp_path, edit)
    save = str(tmp_path / "save")
    out = N.run_program("model", d, save, ext)
    assert out.returncode == 1 and re.search(message, out.stderr), out.stderr
    assert not os.path.exists(os.path.join(save, "pair.txt")) and not os.path.exists(os.path.join(save, "cams"))


def test_score_argument_errors(tmp_path):
    m = dict(SCORE_CASES["n3"])
    m["point_ids"] = m["point_ids"].copy()
    gone = int(m["point_ids"][0])
    m["point_ids"][0] = 999999
    rc, err, _ = N.serial_scores(m, tmp_path)
    assert rc == 1 and "names point %d, which is not among the points" % gone in err
    m = dict(SCORE_CASES["n3"])
    m["point_ids"] = m["point_ids"].copy()
    m["point_ids"][1] = m["point_ids"][0]
    rc, err, _ = N.serial_scores(m, tmp_path)
    assert rc == 1 and "occurs twice" in err


def test_image_argument_errors(tmp_path):
    src = N.picture(9, 5)
    for args, message in (((8, 7, 9, 5), "the padded size"), ((13, 4, 9, 5), "the padded size"), ((13, 7, 0, 5), "bad output size"), ((13, 7, 9, 70000), "bad output size")):
        rc, err, _ = N.serial_image(src, *args, tmp_path)
        assert rc == 1 and message in err, (args, err)
