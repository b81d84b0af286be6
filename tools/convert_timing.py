#!/usr/bin/env python3
"""Times the device steps of `apd --convert-from` on cuda:0 against the same text on the host, and appends the lines to
profiles/convert.txt: dvp_view_scores on the synthetic model of tools/make_convert_golden.py --big (default 1000 images x 10000
observations; the arrays are made in memory, no model files), dvp_convert_image per image at 6208 x 4128, and dvp_undistort_image
(--undistort on) of a 6208 x 4128 THIN_PRISM_FISHEYE picture.
usage: convert_timing.py [N_IMAGES [N_OBS]] [--no-host] [--undistort-only]"""
import importlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import np_convert as N  # noqa: E402
import np_undistort as U  # noqa: E402
from make_convert_golden import big_arrays  # noqa: E402


def median_ms(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), min(t), max(t)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    host = "--no-host" not in sys.argv
    n_images = int(args[0]) if args else 1000
    n_obs = int(args[1]) if len(args) > 1 else 10000
    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    lines = []
    W, H = 6208, 4128
    src = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if "--undistort-only" not in sys.argv:
        scores_and_images(capi, lines, n_images, n_obs, host, src)
    p = U.params("THIN_PRISM_FISHEYE", W, H)
    med, lo, hi = median_ms(lambda: capi.undistort_image(src, "THIN_PRISM_FISHEYE", p), 5)
    line = "undistorted image, %d x %d THIN_PRISM_FISHEYE: dvp_undistort_image %.1f ms per image (%.1f ... %.1f; upload of %.0f MB and read-back of %.0f MB included)" % (W, H, med, lo, hi, src.nbytes / 1e6, src.nbytes / 1e6)
    if host:
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            rc, err, want = U.serial_image(src, "THIN_PRISM_FISHEYE", p, tmp)
            dt = time.perf_counter() - t0
        assert rc == 0, err
        line += "; the same text on the host, one thread (tests/undistort_host image; the two 77-MB files written and read included): %.0f ms; equal: %s" % (
            1e3 * dt, bool(np.array_equal(capi.undistort_image(src, "THIN_PRISM_FISHEYE", p), want)))
    lines.append(line)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "convert.txt"), "a") as f:
        f.write(text)


def scores_and_images(capi, lines, n_images, n_obs, host, src):
    W, H = src.shape[1], src.shape[0]
    centres, xyz, seen, tracks = big_arrays(n_images, n_obs)
    m = N.model([list(s + 1) for s in seen], centres, np.arange(len(xyz)) + 1, xyz)
    work = sum(len(t) * (len(t) - 1) // 2 for t in tracks)
    got = capi.view_scores(m["offsets"], m["ids"], m["centres"], m["point_ids"], m["xyz"])
    med, lo, hi = median_ms(lambda: capi.view_scores(m["offsets"], m["ids"], m["centres"], m["point_ids"], m["xyz"]), 3)
    lines.append("view scores, %d images x %d observations, %d points, %d pair items, %d of %d pairs with score 0 (nothing shared, or zeroed): dvp_view_scores %.0f ms (%.0f ... %.0f; the host's track build, uploads and read-back included)"
                 % (n_images, n_obs, len(xyz), work, int((got[np.triu_indices(n_images, 1)] == 0).sum()), n_images * (n_images - 1) // 2, med, lo, hi))
    if host:
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            rc, err, want = N.serial_scores(m, tmp)
            dt = time.perf_counter() - t0
        assert rc == 0, err
        lines.append("  the same text on the host, one thread (tests/convert_host scores; the 80-MB array file written and read included): %.0f ms; equal to the device's matrix: %s"
                     % (1e3 * dt, bool(np.array_equal(got, want))))
    for F in (1.0, 2.0):
        ow, oh = N.out_size(W, H, F)
        med, lo, hi = median_ms(lambda: capi.convert_image(src, W, H, ow, oh), 5)
        t0 = time.perf_counter()
        want = N.convert_image(src, W, H, ow, oh)
        dt = time.perf_counter() - t0
        lines.append("written image, %d x %d -> %d x %d: dvp_convert_image %.1f ms per image (%.1f ... %.1f; upload of %.0f MB and read-back of %.0f MB included); numpy fancy indexing on the host %.0f ms; equal: %s"
                     % (W, H, ow, oh, med, lo, hi, src.nbytes / 1e6, ow * oh * 3 / 1e6, 1e3 * dt, bool(np.array_equal(capi.convert_image(src, W, H, ow, oh), want))))


if __name__ == "__main__":
    main()
