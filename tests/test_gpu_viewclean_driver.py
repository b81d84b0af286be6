"""`apd --cleanup-on gpu`: the visibility-mask clean-up of every view and pass done by the engine on the staged selected-view
words instead of the background job's Connect loop.  Every file of the output folder is byte-identical to a run with
`--cleanup-on host`, in the default flow, with one and with two views in flight and with --sync-io (which stages no maps and
keeps the host loop); and the clean-up has something to do on this dataset: the words a pass of the host run left differ from
the words it stored."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H, NV = 838, 126, 4      # two pyramid levels: 419 x 63, then 838 x 126
LINE = "Visibility clean-up: on the device"


def run_apd(d, *extra, env=None):
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0", "--iters", "2", "--passes", "1", "--min-scale", "1", "--seed", "7", "--previews"] + list(extra),
                         capture_output=True, text=True, timeout=600, env=env)
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
def test_apd_cleanup_on_gpu_leaves_the_same_files(tmp_path, flow):
    extra = dict(default=[], one_in_flight=["--views-in-flight", "1"], two_in_flight=["--views-in-flight", "2", "--jacobi"], sync_io=["--sync-io"])[flow]
    dirs = {}
    for tag in ("host", "gpu"):
        dirs[tag] = str(tmp_path / tag)
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), dirs[tag], str(W), str(H), str(NV), "3", "--jpg"], stdout=subprocess.DEVNULL)
    raw_dir = tmp_path / "raw"
    raw_dir.mkdir()
    log_host = run_apd(dirs["host"], "--cleanup-on", "host", *extra, env=dict(os.environ, DVP_RAW_VIEWS_DIR=str(raw_dir)))
    log_gpu = run_apd(dirs["gpu"], "--cleanup-on", "gpu", *extra)
    assert LINE not in log_host
    views_done = log_gpu.count(" done!")
    assert views_done >= 2 * NV                                   # every view, at least once per level
    if flow == "default":
        assert log_gpu.count(LINE) == views_done                  # once per view and pass
    if flow == "sync_io":
        assert LINE not in log_gpu                                # no staged maps: the host loop
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    assert sum(k.endswith("selected_views.bin") for k in a) == NV and "APD.ply" in a
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
    assert not any(k.endswith(".part") for k in a)
    # the clean-up had something to do: in the host run at least one view's stored words of the last pass are not the words the
    # pass left, cut to the source bits (what min_region = 0 makes of them)
    changed = 0
    for k in sorted(a):
        if not k.endswith("selected_views.bin"):
            continue
        stored = np.frombuffer(a[k][-W * H * 4:], np.uint32)
        passes = sorted(f for f in os.listdir(raw_dir) if f.startswith(os.path.dirname(k) + "_"))
        last = max(passes, key=lambda f: int(f[:-4].rsplit("_", 1)[1]))
        raw = np.fromfile(os.path.join(raw_dir, last), np.uint32)
        assert raw.size == W * H
        nsrc = int(np.max(stored)).bit_length()
        changed += int((stored != (raw & np.uint32((1 << nsrc) - 1))).any())
    assert changed >= 1
