"""`apd --decode-on gpu --entropy-on gpu`: the input JPEGs' Huffman scan on the device as well (dvp_jpeg_set_entropy(1)).  Every file
of the output folder is byte-identical to a run with --decode-on host — in the default flow, with --images-on gpu, and with every
device switch on — the log names the path once per decoded file, all of them on the device, and --entropy-on gpu without
--decode-on gpu is refused with a usage message before anything is written."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

NV = 3
DECODE, ENTROPY = "Image decode: on the device", "Entropy decode: on the "
_MADE = {}


def dataset(tmp_path_factory, prior):
    """the small folder of the decode driver test (images/*.jpg), made once per kind and copied for every run"""
    if prior not in _MADE:
        d = str(tmp_path_factory.mktemp("scene") / "data")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, "128", "96", str(NV), "2", "--jpg"] + (["--prior"] if prior else []),
                              stdout=subprocess.DEVNULL, timeout=300)
        _MADE[prior] = d
    return _MADE[prior]


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


# flow -> (the folder has dep/ + sfm/, extra flags)
FLOWS = {
    "default": (False, []),
    "images_on_gpu": (False, ["--images-on", "gpu"]),
    "all_on_device": (True, ["--labels", "--edges-on", "gpu", "--labels-on", "gpu", "--cleanup-on", "gpu", "--prior-on", "gpu", "--images-on", "gpu"]),
}


@pytest.mark.parametrize("flow", list(FLOWS))
def test_apd_entropy_on_gpu_leaves_the_same_files(tmp_path, tmp_path_factory, flow):
    prior, extra = FLOWS[flow]
    src = dataset(tmp_path_factory, prior)
    dirs, logs = {}, {}
    for tag, flags in (("host", ["--decode-on", "host"]), ("gpu", ["--decode-on", "gpu", "--entropy-on", "gpu"])):
        dirs[tag] = str(tmp_path / tag)
        shutil.copytree(src, dirs[tag])
        logs[tag] = run_apd(dirs[tag], *flags, *extra)
    assert DECODE not in logs["host"] and ENTROPY not in logs["host"]
    # one line per decoded file: every view's file once as grey (the passes) and once as colour (the fusion), all on the device
    lines = re.findall(re.escape(ENTROPY) + r"(device|host) \((\d{8}\.jpg), (grey|colour)(: [^)]*)?\)", logs["gpu"])
    assert logs["gpu"].count(ENTROPY) == logs["gpu"].count(DECODE) == len(lines) == len(set(lines)) == 2 * NV, lines
    assert set(lines) == {("device", "%08d.jpg" % i, kind, "") for i in range(NV) for kind in ("grey", "colour")}
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    for kind in ("depths.dmb", "APD_normals.dmb", "weak.bin", "selected_views.bin"):
        assert sum(k.endswith(kind) for k in a) == NV, (kind, sorted(a))
    assert "APD.ply" in a
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff


def test_entropy_on_gpu_alone_is_refused(tmp_path):
    for flags in (["--entropy-on", "gpu"], ["--entropy-on", "gpu", "--decode-on", "host"]):
        out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), str(tmp_path), "0"] + flags, capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and out.stderr.startswith("USAGE: ") and "--entropy-on" in out.stderr and "--decode-on gpu" in out.stderr, out.stderr
        assert not os.path.exists(os.path.join(str(tmp_path), "APD"))
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), str(tmp_path), "0", "--decode-on", "gpu", "--entropy-on", "device"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--entropy-on takes host or gpu" in out.stderr
