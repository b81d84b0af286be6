"""`apd --evaluate --refine-alignment` end to end on the synthetic five-view folder of tests/test_gpu_evaluate_driver.py, with the fused
cloud moved by a known rigid matrix: --evaluate-on gpu and host print the same bytes and save the same matrix; the saved matrix given
back through --transform, without a refinement, prints the same evaluation lines; without the new options the report is, byte for
byte, the restated report of the existing entries' counts.  The figures are printed (pytest -s)."""
import os

import numpy as np
import pytest

import np_cloudicp as C
import np_cloudprep as P
import np_evaluate as N
from conftest import pkg
from test_gpu_evaluate_driver import apd_evaluate, scene      # noqa: F401  (the fixture builds the folder and fuses it)

pytestmark = pytest.mark.gpu

KNOWN = P.rotation(0.5, -0.25, [0.02, -0.01, 0.015])
STAGES = "0.05:0.2:20,0.02:0.05:20"


@pytest.fixture(scope="module")
def moved(scene, tmp_path_factory):
    """the fused cloud moved by the inverse of KNOWN: KNOWN is the matrix that brings it back"""
    recon, truth, _ = scene
    d = tmp_path_factory.mktemp("moved")
    N.build_program()
    rc, err, xyz = N.read_ply(recon, d)
    assert rc == 0, err
    away = (np.linalg.inv(KNOWN.reshape(4, 4)) @ np.concatenate([xyz.astype(np.float64), np.ones((len(xyz), 1))], 1).T).T[:, :3]
    N.write_ply_like_apd(str(d / "moved.ply"), away)
    return str(d / "moved.ply"), truth, d


def test_device_and_host_print_the_same_and_the_matrix_round_trips(moved):
    recon, truth, d = moved
    fine = {w: str(d / ("fine_%s.txt" % w)) for w in ("gpu", "host")}
    out = {w: apd_evaluate(recon, "--against", truth, "--evaluate-on", w, "--refine-alignment", STAGES, "--save-transform", fine[w], "--voxel-size", "0.01") for w in fine}
    assert out["gpu"].returncode == 0, out["gpu"].stderr
    assert out["host"].returncode == 0, out["host"].stderr
    assert out["gpu"].stdout == out["host"].stdout and open(fine["gpu"], "rb").read() == open(fine["host"], "rb").read()
    lines = out["gpu"].stdout.splitlines()
    assert lines[0].startswith("alignment stage 0: ") and lines[1].startswith("alignment stage 1: ") and all(ln.startswith("alignment ") for ln in lines[2:6])
    assert lines[5] == "alignment 0 0 0 1" and open(fine["gpu"]).read().splitlines() == [ln[len("alignment "):] for ln in lines[2:6]]
    M = np.array([float(v) for ln in lines[2:6] for v in ln.split()[1:]])
    print("\n" + out["gpu"].stdout + "start %s, refined %s (degrees, length) from the known matrix" % (C.motion_errors(np.eye(4), KNOWN), C.motion_errors(M, KNOWN)))
    # the saved matrix through --transform and no refinement: the same evaluation lines, on either flavour
    for w in fine:
        again = apd_evaluate(recon, "--against", truth, "--evaluate-on", w, "--transform", fine["gpu"], "--voxel-size", "0.01")
        assert again.returncode == 0 and again.stdout.splitlines() == lines[6:], w
    # with a rough matrix to start from, and a crop-less run of the existing options only: no alignment line, the same shape as before
    plain = apd_evaluate(recon, "--against", truth, "--voxel-size", "0.01")
    assert plain.returncode == 0 and "alignment" not in plain.stdout and [ln.split()[0] for ln in plain.stdout.splitlines()] == [ln.split()[0] for ln in lines[6:]]


def test_without_the_option_the_report_is_the_existing_one(moved, tmp_path):
    """the existing options alone: the report's bytes are the text that tests/np_cloudicp.py restates from the parent commit's format,
    filled with the counts of the existing entries dvp_cloud_evaluate_prepared and dvp_cloud_evaluate on the same clouds; the same on
    both flavours and in the file --out leaves; no alignment line"""
    recon, truth, d = moved
    capi = pkg("capi")
    clouds = []
    for ply in (recon, truth):
        rc, err, xyz = N.read_ply(ply, tmp_path)
        assert rc == 0, err
        clouds.append(xyz)
    tol = N.DEFAULT_TOLERANCES
    rough = str(tmp_path / "rough.txt")
    with open(rough, "w") as f:
        f.write("\n".join(" ".join("%.17g" % v for v in row) for row in KNOWN.reshape(4, 4)) + "\n")
    res = capi.cloud_evaluate_prepared(clouds[0], clouds[1], tol, P.prep(KNOWN, None, 0.01), P.prep(None, None, 0.01))
    want = C.report_text(recon, truth, [len(clouds[0]), len(clouds[1])], res["used"], res["within_recon"], res["within_truth"], tol, res["counts"])
    runs = [apd_evaluate(recon, "--against", truth, "--evaluate-on", w, "--transform", rough, "--voxel-size", "0.01", "--out", str(tmp_path / (w + ".txt"))) for w in ("gpu", "host")]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    assert runs[0].stdout == want and runs[1].stdout == want and open(str(tmp_path / "gpu.txt")).read() == want
    assert len(want.splitlines()) == 11 and "alignment" not in want
    res = capi.cloud_evaluate(clouds[0], clouds[1], tol)
    plain = apd_evaluate(recon, "--against", truth)
    assert plain.returncode == 0 and plain.stdout == C.report_text(recon, truth, [len(clouds[0]), len(clouds[1])], res["used"], res["within_recon"], res["within_truth"], tol)
    out = apd_evaluate(recon, "--against", truth, "--save-transform", str(tmp_path / "none.txt"))
    assert out.returncode == 1 and "--save-transform needs --refine-alignment" in out.stderr
