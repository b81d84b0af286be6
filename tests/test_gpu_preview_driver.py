"""`apd --previews`: the reference's preview files (show_medium_result, main.cpp:219-223, 383-384, 396-403) in every view's
result folder, byte-identical to libjpeg-turbo's encoding of np_preview applied to the maps the driver stored; --sync-io
gives the same bytes; without the flag no image appears and every map is byte-identical."""
import glob
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import np_preview as P
from test_gpu_driver import read_binmat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NV = 160, 120, 3


def run_apd(d, *extra):
    out = subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0", "--iters", "2", "--passes", "1", "--min-scale", "1", "--seed", "11",
                          "--no-fusion"] + list(extra), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    return sorted({int(i) for i in re.findall(r"Iteration: (\d+)", out.stdout)})


def depth_range(d, v):
    rng = open(os.path.join(d, "cams", "%08d_cam.txt" % v)).read().split()[-4:]
    return np.float32(rng[0]) * np.float32(0.6), np.float32(rng[3]) * np.float32(1.2)   # APD.cpp:1109-1110


def files(d, pattern):
    return {os.path.relpath(f, d): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(d, "APD", "*", pattern)))}


@pytest.mark.gpu
def test_apd_previews(tmp_path):
    dirs = {}
    for tag in ("plain", "previews", "sync"):
        dirs[tag] = str(tmp_path / tag)
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), dirs[tag], str(W), str(H), str(NV), "2"],
                              stdout=subprocess.DEVNULL)
    its = run_apd(dirs["previews"], "--previews")
    assert len(its) >= 2
    run_apd(dirs["sync"], "--previews", "--sync-io")
    run_apd(dirs["plain"])
    d = dirs["previews"]
    for v in range(NV):
        r = os.path.join(d, "APD", "%08d" % v)
        for it in its:
            for k in ("depth", "normal", "weak"):
                assert os.path.exists(os.path.join(r, "%s_%d.jpg" % (k, it))), (v, k, it)
        assert glob.glob(os.path.join(r, "rawedge_*.jpg")), v
        # the final pass' files: np_preview of the stored maps, encoded by libjpeg-turbo at the engine's restart interval
        dmin, dmax = depth_range(d, v)
        depth = read_binmat(os.path.join(r, "depths.dmb"))
        normal = read_binmat(os.path.join(r, "APD_normals.dmb"))
        weak = read_binmat(os.path.join(r, "weak.bin"))
        ref = dict(depth=P.depth_preview(depth, dmin, dmax), normal=P.normal_preview(normal), weak=P.weak_preview(weak))
        for k, img in ref.items():
            got = open(os.path.join(r, "%s_%d.jpg" % (k, its[-1])), "rb").read()
            assert got == P.pil_jpeg(img, 95, P.dri(got)), (v, k)
        from PIL import Image
        png = np.asarray(Image.open(os.path.join(r, "weak.png")))
        assert png.shape == (H, W, 3) and np.array_equal(png, ref["weak"][..., ::-1]), v
        # rawedge: a grey JPEG of the edge map at the pass' scale
        raw = open(glob.glob(os.path.join(r, "rawedge_*.jpg"))[0], "rb").read()
        assert np.asarray(Image.open(io.BytesIO(raw))).ndim == 2
    # --sync-io: planes downloaded and unpacked on the host; the same preview bytes
    assert files(d, "*.jpg") and files(d, "*.jpg") == files(dirs["sync"], "*.jpg")
    assert files(d, "*.png") == files(dirs["sync"], "*.png")
    # without the flag: no image at all, and every map the same bytes as with it
    assert not files(dirs["plain"], "*.jpg") and not files(dirs["plain"], "*.png")
    for pat in ("*.dmb", "*.bin"):
        a, b = files(dirs["plain"], pat), files(d, pat)
        assert a.keys() == b.keys() and all(a[k] == b[k] for k in a), pat
