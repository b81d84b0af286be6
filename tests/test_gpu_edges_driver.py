"""`apd --edges-on gpu`: the edge prior of every view made by the engine from the resident image instead of the helper
threads' EdgeSegment.  Every file of the output folder — edges_<s>.dmb, every map, the fused cloud, rawedge_<s>.jpg and the
other previews — is byte-identical to a run without the flag, in the default flow, with one and with two views in flight and
with --sync-io; a second run over the finished folder makes no edge map again and leaves the files as they were."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H, NV = 838, 126, 4      # two pyramid levels: 419 x 63, then 838 x 126


def run_apd(d, *extra):
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0", "--iters", "2", "--passes", "1", "--min-scale", "1", "--seed", "7", "--previews"] + list(extra),
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


@pytest.mark.parametrize("flow", ["default", "one_in_flight", "two_in_flight", "sync_io"])
def test_apd_edges_on_gpu_leaves_the_same_files(tmp_path, flow):
    extra = dict(default=[], one_in_flight=["--views-in-flight", "1"], two_in_flight=["--views-in-flight", "2", "--jacobi"], sync_io=["--sync-io"])[flow]
    dirs = {}
    for tag in ("host", "gpu"):
        dirs[tag] = str(tmp_path / tag)
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), dirs[tag], str(W), str(H), str(NV), "3", "--jpg"], stdout=subprocess.DEVNULL)
    log_host = run_apd(dirs["host"], *extra)
    log_gpu = run_apd(dirs["gpu"], "--edges-on", "gpu", *extra)
    assert "Edge map: made on the device" not in log_host
    assert log_gpu.count("Edge map: made on the device") == 2 * NV          # every view, once per level
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    for kind in ("edges_0.dmb", "edges_1.dmb", "rawedge_0.jpg", "rawedge_1.jpg", "depths.dmb", "weak.bin"):
        assert sum(k.endswith(kind) for k in a) == NV, (kind, sorted(a))
    assert "APD.ply" in a
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
    assert not any(k.endswith(".part") for k in a)
    # a second run over the finished folder: every edges_<s>.dmb is there, none is made again, nothing changes
    log_again = run_apd(dirs["gpu"], "--edges-on", "gpu", *extra)
    assert "Edge map: made on the device" not in log_again
    c = tree(dirs["gpu"])
    assert sorted(c) == sorted(b) and not [k for k in sorted(b) if b[k] != c[k]]
