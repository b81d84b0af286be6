"""`apd --strong-wide on`: views with more than 16 sources take the split strong update (DVP_STRONG_WIDE=1 for the engine).  A
folder of 19 views with 18 sources each: every file of the output folder is byte-identical to a run without the flag; with the
flag every view logs "Strong update: split form, 18 views" once per pass, without it never."""
import os
import re
import subprocess
import sys

from conftest import ROOT
import pytest

from test_gpu_edges_driver import run_apd, tree

pytestmark = pytest.mark.gpu

W, H, NV, NSRC = 96, 72, 19, 18
LINE = "Strong update: split form, %d views" % NSRC


def test_apd_strong_wide_leaves_the_same_files(tmp_path, monkeypatch):
    monkeypatch.delenv("DVP_STRONG_WIDE", raising=False)
    dirs = {}
    for tag in ("off", "on"):
        dirs[tag] = str(tmp_path / tag)
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), dirs[tag], str(W), str(H), str(NV), str(NSRC), "--jpg"], stdout=subprocess.DEVNULL)
    log_off = run_apd(dirs["off"])
    log_on = run_apd(dirs["on"], "--strong-wide", "on")
    assert "Strong update:" not in log_off
    done = len(re.findall(r"Processing image: \d+ done!", log_on))      # one per view and pass
    assert done >= 2 * NV and done % NV == 0, done
    assert done == len(re.findall(r"Processing image: \d+ done!", log_off))
    assert log_on.count(LINE) == done, (log_on.count(LINE), done)
    assert log_on.count("Strong update:") == done
    a, b = tree(dirs["off"]), tree(dirs["on"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    assert sum(k.endswith("depths.dmb") for k in a) == NV and "APD.ply" in a
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
