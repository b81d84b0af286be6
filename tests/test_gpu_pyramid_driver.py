"""`apd --images-on gpu`: every view's level images made by the engine from the decoded bytes (uploaded once per job) instead of
load_image's float images, LevelImages::Fill and the level prefetch.  Every file of the output folder is byte-identical to a run
with --images-on host — in the default flow, with --sync-io, with two views in flight, with every other device switch on, on a
folder whose levels are float planes (sizes that std::round makes inexact) and on one whose views' files differ in size (padded
and cropped sources, which take the host path without the switch even with resident blocks) — and two ranks with the switch
equal one rank without it."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ON_DEVICE, HOST_PATH = "Images: levels made on the device", "Images: host path"
_MADE = {}


def dataset(tmp_path_factory, W, H, NV, jpg):
    """one synthetic folder per geometry, made once and copied for every run"""
    key = (W, H, NV, jpg)
    if key not in _MADE:
        d = str(tmp_path_factory.mktemp("scene") / "data")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, str(W), str(H), str(NV), "3"] + (["--jpg"] if jpg else []),
                              stdout=subprocess.DEVNULL, timeout=300)
        _MADE[key] = d
    return _MADE[key]


def run_apd(d, *extra):
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0", "--iters", "2", "--passes", "1", "--min-scale", "1", "--seed", "7"] + list(extra),
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, DVP_HOST_TIMING="1"))   # (the log then names every view's image format)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    return out.stdout


def tree(d):
    out = {}
    top = os.path.join(d, "APD")
    for base, _, names in os.walk(top):
        for n in names:
            f = os.path.join(base, n)
            out[os.path.relpath(f, top)] = open(f, "rb").read()
    return out


def read_pgm(f):
    raw = open(f, "rb").read()
    magic, w, h, _, body = raw.split(None, 4)
    assert magic == b"P5"
    return np.frombuffer(body, np.uint8).reshape(int(h), int(w))


def write_pgm(f, a):
    with open(f, "wb") as out:
        out.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        out.write(np.ascontiguousarray(a, np.uint8).tobytes())


def unequal_files(d):
    """view 2's file 24 columns / 16 rows short (zero padding where it is a source), view 1's 16 columns / 8 rows too large (cropped)"""
    f = os.path.join(d, "images", "%08d.pgm" % 2)
    a = read_pgm(f)
    write_pgm(f, a[:a.shape[0] - 16, :a.shape[1] - 24])
    f = os.path.join(d, "images", "%08d.pgm" % 1)
    a = read_pgm(f)
    big = np.random.default_rng(3).integers(0, 256, (a.shape[0] + 8, a.shape[1] + 16), dtype=np.uint8)
    big[:a.shape[0], :a.shape[1]] = a
    write_pgm(f, big)


# flow -> (W, H, NV, jpg, extra flags, change to the folder)
FLOWS = {
    "default": (838, 126, 4, True, ["--previews"], None),
    "sync_io": (838, 126, 4, True, ["--previews", "--sync-io"], None),
    "two_in_flight": (838, 126, 4, True, ["--previews", "--views-in-flight", "2", "--jacobi"], None),
    "all_on_device": (838, 126, 4, True, ["--previews", "--labels", "--edges-on", "gpu", "--labels-on", "gpu", "--cleanup-on", "gpu"], None),
    "float_levels": (837, 125, 4, True, ["--previews"], None),               # 418.5 -> 419, 62.5 -> 63: levels that are no binary16 values
    "unequal_files": (838, 126, 4, False, ["--no-fusion"], unequal_files),   # (.pgm files; the fusion wants views of one size)
}


@pytest.mark.parametrize("flow", list(FLOWS))
def test_apd_images_on_gpu_leaves_the_same_files(tmp_path, tmp_path_factory, flow):
    W, H, NV, jpg, extra, change = FLOWS[flow]
    src = dataset(tmp_path_factory, W, H, NV, jpg)
    dirs, logs = {}, {}
    for tag in ("host", "gpu"):
        dirs[tag] = str(tmp_path / tag)
        shutil.copytree(src, dirs[tag])
        if change:
            change(dirs[tag])
        logs[tag] = run_apd(dirs[tag], "--images-on", tag, *extra)
    assert ON_DEVICE not in logs["host"] and HOST_PATH not in logs["host"]
    passes = 2 * 2                                                           # two levels, an A pass and one geometric pass each
    assert logs["gpu"].count(ON_DEVICE) == NV * passes and HOST_PATH not in logs["gpu"]
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    for kind in ("edges_0.dmb", "edges_1.dmb", "depths.dmb", "APD_normals.dmb", "weak.bin", "selected_views.bin"):
        assert sum(k.endswith(kind) for k in a) == NV, (kind, sorted(a))
    assert ("APD.ply" in a) == ("--no-fusion" not in extra)
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
    assert not any(k.endswith(".part") for k in a)
    if flow == "float_levels":   # the coarse level did run on float planes, the fine one on bytes, on both sides
        for tag in ("host", "gpu"):
            assert "| images f32" in logs[tag] and "| images u8" in logs[tag] and "| images f16" not in logs[tag]
    elif jpg:
        assert "| images f16" in logs["gpu"] and "| images f32" not in logs["gpu"]


def test_a_store_without_room_keeps_the_host_path(tmp_path, tmp_path_factory):
    """DVP_RESIDENT_IMAGES_GB=0: nothing fits the store, every view says so and takes the host path; same files"""
    src = dataset(tmp_path_factory, 838, 126, 4, True)
    dirs = {}
    for tag in ("host", "gpu"):
        dirs[tag] = str(tmp_path / tag)
        shutil.copytree(src, dirs[tag])
    run_apd(dirs["host"], "--images-on", "host")
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), dirs["gpu"], "0", "--iters", "2", "--passes", "1", "--min-scale", "1", "--seed", "7", "--images-on", "gpu"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, DVP_RESIDENT_IMAGES_GB="0"))
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert out.stdout.count(HOST_PATH + " (image ") == 4 * 4 and ON_DEVICE not in out.stdout
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b) and not [k for k in sorted(a) if a[k] != b[k]]


def _apd(d, *args):
    return subprocess.Popen([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_apd_two_ranks_with_images_on_gpu_equal_one_rank_without(tmp_path, tmp_path_factory):
    """two ranks over the host transport: the owners broadcast the decoded bytes once per job and every rank makes its levels on
    its device; every file of every view equals the single-rank --jacobi run that builds its images on the host"""
    W, H, NV = 128, 96, 5
    src = dataset(tmp_path_factory, W, H, NV, False)
    common = ["--iters", "2", "--passes", "2", "--min-scale", "1", "--seed", "5", "--no-fusion"]
    dirs, texts = {}, {}
    for tag in ("single", "world2"):
        dirs[tag] = str(tmp_path / tag)
        shutil.copytree(src, dirs[tag])
        if tag == "single":
            procs = [_apd(dirs[tag], "--jacobi", "--images-on", "host", *common)]
        else:
            procs = [_apd(dirs[tag], "--rank", str(r), "--world", "2", "--job", "job43", "--transport", "host", "--collective-timeout", "120", "--images-on", "gpu", *common)
                     for r in (1, 0)]
        texts[tag] = []
        for p in procs:
            so, se = p.communicate(timeout=900)
            assert p.returncode == 0, so[-1500:] + se[-1500:]
            texts[tag].append(so)
    assert ON_DEVICE not in texts["single"][0]
    per_rank = [t.count(ON_DEVICE) for t in texts["world2"]]
    assert sum(per_rank) == NV * 3 and min(per_rank) > 0 and not any(HOST_PATH in t for t in texts["world2"]), per_rank   # one level: an A pass and two geometric ones
    a, b = tree(dirs["single"]), tree(dirs["world2"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    assert sum(k.endswith("depths.dmb") for k in a) == NV
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
