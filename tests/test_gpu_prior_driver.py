"""`apd --prior-on gpu`: the FIRST_INIT plane prior of every view made by the engine (dvp_plane_prior) instead of the driver
thread's BuildPlanePrior.  Every file of the output folder is byte-identical to a run with --prior-on host and both runs log
"Plane prior from dep/ and sfm/" for every view: at a single-level size, over the two-level pyramid of test_gpu_driver.py's
neighbours (838 x 126 files, a 419 x 63 coarsest level: the FIRST_INIT pass rescales the dep map), and with one view's sfm/ file
removed, which draws random planes for that view in both modes."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from test_gpu_edges_driver import run_apd, tree       # run_apd passes --min-scale 1: every pyramid level

pytestmark = pytest.mark.gpu

NV = 3
LINE, RANDOM = "Plane prior from dep/ and sfm/", "No dep/ + sfm/ prior: random plane initialisation"


@pytest.mark.parametrize("size,drop_sfm", [((128, 96), False), ((838, 126), False), ((128, 96), True)], ids=["one_level", "two_levels", "one_view_without_sfm"])
def test_apd_prior_on_gpu_leaves_the_same_files(tmp_path, size, drop_sfm):
    W, H = size
    dirs, logs = {}, {}
    for tag in ("host", "gpu"):
        dirs[tag] = str(tmp_path / tag)
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), dirs[tag], str(W), str(H), str(NV), "2", "--prior"], stdout=subprocess.DEVNULL)
        if drop_sfm:
            os.remove(os.path.join(dirs[tag], "sfm", "%08d.txt" % 1))
        logs[tag] = run_apd(dirs[tag], "--prior-on", tag)
    for tag in ("host", "gpu"):      # one FIRST_INIT pass per view, at the coarsest level
        assert logs[tag].count(LINE) == NV - int(drop_sfm), (tag, logs[tag][-1500:])
        assert logs[tag].count(RANDOM) == int(drop_sfm), (tag, logs[tag][-1500:])
    a, b = tree(dirs["host"]), tree(dirs["gpu"])
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    assert sum(k.endswith("depths.dmb") for k in a) == NV and "APD.ply" in a
    diff = [k for k in sorted(a) if a[k] != b[k]]
    assert not diff, diff
