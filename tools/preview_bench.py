"""Cost of `apd --previews` (the preview JPEGs rendered and encoded on the device, csrc/dvp_jpeg.hip).

  python3 tools/preview_bench.py [--sizes 3104x2064,6208x4128] [--schedule WxH] [--reps N]

Prints, per size: wall time of dvp_preview_begin (render + encode of the three previews, its one wait included) and of the
three dvp_preview_finish fetches, the bytes of each file, and what the engine's restart interval costs against the same image
written by libjpeg-turbo without restart markers; the same for a grey edge-like map through dvp_jpeg_encode.  With
--schedule: wall time of a ten-view `apd --passes 1 --min-scale 1` run on a tools/make_dataset.py set with and without
--previews."""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene_state(W, H, dmin, dmax, rs):
    """a depth map with smooth structure and noise, unit normals, mostly STRONG pixels: what a pass leaves"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    d = dmin + (dmax - dmin) * (0.5 + 0.3 * np.sin(x / 300.0) * np.cos(y / 200.0) + 0.05 * rs.standard_normal((H, W)).astype(np.float32))
    n = np.stack([np.sin(x / 500.0), np.cos(y / 400.0), -np.ones_like(x)], -1) + 0.02 * rs.standard_normal((H, W, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    planes = np.concatenate([n.reshape(-1, 3), d.reshape(-1, 1)], 1).astype(np.float32)
    weak = (rs.random_sample(H * W) < 0.03).astype(np.uint8) ^ 1
    return planes, weak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3104x2064,6208x4128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--schedule", default="")
    a = ap.parse_args()
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    pkg = importlib.import_module("dvp-mvs_amd")
    capi, synth = pkg.get_capi(), pkg.synth
    import np_preview as P
    kinds = dict(depth=capi.PREVIEW_DEPTH, normal=capi.PREVIEW_NORMAL, weak=capi.PREVIEW_WEAK)
    for s in a.sizes.split(","):
        W, H = map(int, s.split("x"))
        rs = np.random.RandomState(0)
        p = synth.default_params(2)
        p["depth_min"], p["depth_max"] = np.float32(1.5), np.float32(7.8)
        planes, weak = scene_state(W, H, 1.5, 7.8, rs)
        ctx = capi.Context(W, H, 2)
        ctx.set_params(p)
        ctx.upload_state(planes=planes, weak=weak)
        tb, tf = [], []
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            ctx.preview_begin(7, 95)
            t1 = time.perf_counter()
            out = {k: ctx.preview_finish(v) for k, v in kinds.items()}
            t2 = time.perf_counter()
            if r:
                tb.append((t1 - t0) * 1e3)
                tf.append((t2 - t1) * 1e3)
        print("%dx%d: preview_begin (render + encode of 3 previews, incl. its sync) median %.2f ms (min %.2f); 3 x preview_finish %.2f ms"
              % (W, H, np.median(tb), min(tb), np.median(tf)))
        for k, v in kinds.items():
            pix = ctx.preview_pixels(v)
            R = P.dri(out[k])
            plain = len(P.pil_jpeg(pix, 95, None))
            t0 = time.perf_counter()
            P.pil_jpeg(pix, 95, None)
            t_pil = (time.perf_counter() - t0) * 1e3
            print("  %-6s %9d bytes, R=%d MCUs: +%.2f %% against %d bytes without restart markers; libjpeg-turbo (Pillow, this host) %.1f ms"
                  % (k, len(out[k]), R, 100.0 * (len(out[k]) - plain) / plain, plain, t_pil))
        ctx.close()
        edge = (rs.random_sample((H, W)) < 0.05).astype(np.uint8) * 255
        t0 = time.perf_counter()
        g = capi.jpeg_encode(edge, 95)
        t_g = (time.perf_counter() - t0) * 1e3
        plain = len(P.pil_jpeg(edge, 95, None))
        print("  grey edge map via dvp_jpeg_encode (host in/out, allocations included) %.1f ms, %d bytes, R=%d: +%.2f %%"
              % (t_g, len(g), P.dri(g), 100.0 * (len(g) - plain) / plain))
    if a.schedule:
        W, H = map(int, a.schedule.split("x"))
        with tempfile.TemporaryDirectory() as tmp:
            res = {}
            for tag, extra in (("plain", []), ("previews", ["--previews"]), ("plain2", []), ("previews2", ["--previews"])):
                d = os.path.join(tmp, tag)
                subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, str(W), str(H), "10", "4"], stdout=subprocess.DEVNULL)
                t0 = time.perf_counter()
                subprocess.run([os.path.join(ROOT, "dvp-mvs_amd", "apd"), d, "0", "--passes", "1", "--min-scale", "1", "--no-fusion"] + extra,
                               check=True, stdout=subprocess.DEVNULL, timeout=1200)
                res[tag] = time.perf_counter() - t0
            for tag, t in res.items():
                print("ten-view apd schedule %dx%d %-9s: %.2f s" % (W, H, tag, t))
            base = min(res["plain"], res["plain2"])
            print("  --previews adds %.1f %% (best of two each)" % (100.0 * (min(res["previews"], res["previews2"]) - base) / base))


if __name__ == "__main__":
    main()
