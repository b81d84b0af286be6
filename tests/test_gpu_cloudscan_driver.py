"""`apd --evaluate --against-scans` end to end on the room of tests/np_cloudscan.py, written as a MeshLab project with one PLY per
scan: --evaluate-on gpu and host print the same bytes - plainly, with --transform, with --voxel-size and with one --refine-alignment
stage -, the plain report is the restated one, and --save-prepared leaves the truth cloud that numpy computes from the scans."""
import os
import subprocess

import numpy as np
import pytest

import np_cloudprep as P
import np_cloudscan as S
import np_evaluate as N
from conftest import ROOT

pytestmark = pytest.mark.gpu

APD = os.path.join(ROOT, "dvp-mvs_amd", "apd")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    S.build_program()
    N.build_program()
    d = tmp_path_factory.mktemp("room")
    room = S.room()
    recon = str(d / "recon.ply")
    N.write_ply_like_apd(recon, room["recon"])
    project, names = S.write_scans(d, room["scans"])
    rough = str(d / "rough.txt")
    M = P.rotation(0.2, -0.1, [0.004, -0.003, 0.002])
    with open(rough, "w") as f:
        f.write("\n".join(" ".join("%.17g" % v for v in row) for row in M.reshape(4, 4)) + "\n")
    return dict(room=room, recon=recon, project=project, names=names, rough=rough, M=M, folder=d)


def both_flavours(files, *args):
    out = {}
    for w in ("gpu", "host"):
        out[w] = subprocess.run([APD, "--evaluate", files["recon"], "--against-scans", files["project"], "--cube-size", str(S.ROOM_R), "--tolerances",
                                 N.tolerance_text(S.ROOM_TOLERANCES), "--evaluate-on", w] + [str(a).replace("@", w) for a in args], capture_output=True, text=True, timeout=300)
        assert out[w].returncode == 0, out[w].stderr
    return out["gpu"].stdout, out["host"].stdout


def test_device_and_host_print_the_same_report(files, tmp_path):
    gpu, host = both_flavours(files)
    assert gpu == host
    room = files["room"]
    rc, err, want = S.serial_evaluate(room["recon"], room["scans"], S.ROOM_TOLERANCES, S.ROOM_R, tmp_path)
    assert rc == 0, err
    assert gpu == S.report_text(files["recon"], files["project"], files["names"], room["scans"], want, S.ROOM_TOLERANCES, len(room["recon"]))
    assert gpu.splitlines()[-3:] == ["%.9g 3000 2000 2000" % float(np.float32(t)) for t in S.ROOM_TOLERANCES]
    print("\n" + gpu)


def test_the_same_with_a_transform_and_with_voxels(files, tmp_path):
    gpu, host = both_flavours(files, "--transform", files["rough"])
    assert gpu == host and gpu.splitlines()[4].startswith("prepared reconstruction: 7000 finite, ")
    gpu, host = both_flavours(files, "--voxel-size", "0.1", "--save-prepared", str(tmp_path / "@_"))
    assert gpu == host
    truth = P.prepare(S.truth_cloud(files["room"]["scans"]), None, None, 0.1)["xyz"]
    for w in ("gpu", "host"):      # the truth cloud that numpy makes of the scans, thinned by numpy's voxels
        rc, err, saved = N.read_ply(str(tmp_path / (w + "_truth.ply")), tmp_path)
        assert rc == 0 and N.same_bits(saved, truth), w
    assert gpu.splitlines()[5] == "prepared ground_truth: 484812 finite, 484812 in the crop volume, %d points" % len(truth)


def test_the_same_with_a_refinement_stage(files, tmp_path):
    gpu, host = both_flavours(files, "--transform", files["rough"], "--refine-alignment", "0.1:0.3:5", "--save-transform", str(tmp_path / "@.txt"))
    assert gpu == host and gpu.startswith("alignment stage 0: ")
    assert open(str(tmp_path / "gpu.txt"), "rb").read() == open(str(tmp_path / "host.txt"), "rb").read()
    assert "tolerance accurate free_space unobserved" in gpu
