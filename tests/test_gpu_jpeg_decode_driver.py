"""`apd --decode-on gpu`: the input JPEGs' inverse DCT and colour conversion on the device (dvp_jpeg_decode, dvp_jpeg_decode_into_store),
the entropy decode on the host.  Every file of the output folder is byte-identical to a run with --decode-on host — in the
default flow (the fusion on: APD.ply holds the colour path), with --images-on gpu (the luma plane goes straight into the image
store), with --sync-io, over two pyramid levels, and with every other device switch on — the log names every decoded file once
under gpu and none under host, and an unknown value of the flag is a usage error."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NV = 3
LINE = "Image decode: on the device"
_MADE = {}


def dataset(tmp_path_factory, W, H, prior):
    """one synthetic folder (images/*.jpg) per geometry, made once and copied for every run"""
    key = (W, H, prior)
    if key not in _MADE:
        d = str(tmp_path_factory.mktemp("scene") / "data")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, str(W), str(H), str(NV), "2", "--jpg"] + (["--prior"] if prior else []),
                              stdout=subprocess.DEVNULL, timeout=300)
        _MADE[key] = d
    return _MADE[key]


def run_apd(d, *extra):
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0", "--iters", "2", "--passes", "1", "--min-scale", "1", "--seed", "7"] + list(extra),
                         capture_output=True, text=True, timeout=600)
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


# flow -> (W, H, the folder has dep/ + sfm/, extra flags)
FLOWS = {
    "default": (128, 96, False, []),
    "images_on_gpu": (128, 96, False, ["--images-on", "gpu"]),
    "sync_io": (128, 96, False, ["--sync-io"]),
    "two_levels": (838, 126, False, []),
    "all_on_device": (128, 96, True, ["--labels", "--edges-on", "gpu", "--labels-on", "gpu", "--cleanup-on", "gpu", "--prior-on", "gpu", "--images-on", "gpu"]),
}


@pytest.mark.parametrize("flow", list(FLOWS))
def test_apd_decode_on_gpu_leaves_the_same_files(tmp_path, tmp_path_factory, flow):
    W, H, prior, extra = FLOWS[flow]
    src = dataset(tmp_path_factory, W, H, prior)
    dirs, logs = {}, {}
    for tag in ("host", "gpu"):
        dirs[tag] = str(tmp_path / tag)
        shutil.copytree(src, dirs[tag])
        logs[tag] = run_apd(dirs[tag], "--decode-on", tag, *extra)
    assert LINE not in logs["host"]
    # one line per decoded file: every view's file once as grey (the passes) and once as colour (the fusion)
    lines = re.findall(re.escape(LINE) + r" \((\d{8}\.jpg), (grey|colour)(, into the image store)?\)", logs["gpu"])
    assert logs["gpu"].count(LINE) == len(lines) == len(set(lines)) == 2 * NV, lines
    stored = ", into the image store" if "--images-on" in extra else ""      # the luma planes took dvp_jpeg_decode_into_store
    assert set(lines) == {("%08d.jpg" % i, kind, stored if kind == "grey" else "") for i in range(NV) for kind in ("grey", "colour")}
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    for kind in ("depths.dmb", "APD_normals.dmb", "weak.bin", "selected_views.bin"):
        assert sum(k.endswith(kind) for k in a) == NV, (kind, sorted(a))
    assert "APD.ply" in a
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
    if "--images-on" in extra:
        assert logs["gpu"].count("Images: levels made on the device") == logs["host"].count("Images: levels made on the device") > 0


def test_an_unknown_value_is_a_usage_error(tmp_path):
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), str(tmp_path), "0", "--decode-on", "device"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--decode-on takes host or gpu" in out.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "APD"))
