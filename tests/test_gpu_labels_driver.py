"""`apd --labels-on gpu`: the label prior of every view and level made by a dvp_labels job on the device instead of the helper
threads' LabelSegment.  Every file of the output folder — labels_<s>.dmb, every map, the fused cloud, the previews — is
byte-identical to a run with --labels-on host: in the default flow, with --labels (the maps are loaded and steer the weak
path), with --sync-io (the driver's own thread makes the maps) and over a two-level pyramid; once more with the edge prior and
the view clean-up on the device as well."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_edges_driver import H, NV, W, run_apd, tree       # the folder maker's geometry: 838 x 126, levels 419 x 63 and 838 x 126

pytestmark = pytest.mark.gpu

LINE = "Label map: on the device"


def make_folder(d):
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, str(W), str(H), str(NV), "3", "--jpg"], stdout=subprocess.DEVNULL)
    # flat rectangles into every view — large ones (numbered regions) and small ones (-1): the synthetic scene alone is textured
    # almost everywhere
    from PIL import Image
    for n in sorted(os.listdir(os.path.join(d, "images"))):
        fn = os.path.join(d, "images", n)
        a = np.array(Image.open(fn).convert("L"))
        for k, v in enumerate((60, 128, 200)):
            a[H // 4:H // 4 + 48, 40 + 150 * k:40 + 150 * k + 100] = v
        for k in range(4):
            a[H - 34:H - 34 + 18, 60 + 90 * k:60 + 90 * k + 18 + 2 * k] = 100 + 20 * k
        Image.fromarray(np.stack([a, a, a], 2), "RGB").save(fn, quality=98, subsampling=2)


def apd(d, *extra):
    """run_apd of test_gpu_edges_driver.py passes --min-scale 1 (both levels); the one-level flows run the driver's own default"""
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0", "--iters", "2", "--passes", "1", "--seed", "7", "--previews"] + list(extra),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    return out.stdout


FLOWS = dict(default=(apd, [], 1), labels=(apd, ["--labels"], 1), sync_io=(apd, ["--sync-io"], 1), two_levels=(run_apd, [], 2),
             all_on_device=(run_apd, ["--labels", "--edges-on", "gpu", "--cleanup-on", "gpu"], 2))


@pytest.mark.parametrize("flow", sorted(FLOWS))
def test_apd_labels_on_gpu_leaves_the_same_files(tmp_path, flow):
    run, extra, levels = FLOWS[flow]
    dirs = {}
    for tag in ("host", "gpu"):
        dirs[tag] = str(tmp_path / tag)
        make_folder(dirs[tag])
    log_host = run(dirs["host"], "--labels-on", "host", *extra)
    log_gpu = run(dirs["gpu"], "--labels-on", "gpu", *extra)
    assert LINE not in log_host
    assert log_gpu.count(LINE) == levels * NV          # every view, once per level
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    for s in range(2 - levels, 2):
        maps = [k for k in a if k.endswith("labels_%d.dmb" % s)]
        assert len(maps) == NV, (s, sorted(a))
        for k in maps:
            lab = np.frombuffer(a[k][16:], np.int32)
            assert len(np.unique(lab[lab > 0])) >= 2 and (lab == -1).any() and (lab == 0).any(), (k, np.unique(lab))
    assert "APD.ply" in a
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
    assert not any(k.endswith(".part") for k in a)
