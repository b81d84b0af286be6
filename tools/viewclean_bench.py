#!/usr/bin/env python3
"""Cost of the visibility-mask clean-up on the device (csrc/dvp_viewclean.hip) against the host's Connect loop.

  python3 tools/viewclean_bench.py [--sizes 1552x1032,3104x2064,6208x4128] [--planes 9] [--reps N] [--stages]
                                   [--views FILE --views-size WxH] [--schedule WxH] [--out FILE]

Per size, on a synthetic map of `planes` bit planes (smooth-field thresholds per bit + 2 % salt noise, min_region = 1280; or the
raw words of an actual pass: --views, a file `apd` wrote under DVP_RAW_VIEWS_DIR): the scratch bytes; the wall time of
dvp_download_maps_begin on a two-image context holding these words, with the clean-up off and on (the call ends with a wait for
the context's stream, so the difference is the device time the clean-up adds in front of that wait); the host mirror's clean-up
(host/cc.cpp's Connect + the fill rule, eight threads as the driver's background job) on the same words.  At 6208x4128 the two
results are compared once — the only place the full size is compared.  --stages runs each size once more under
`rocprofv3 --kernel-trace --stats` in a child process and prints the time of every dvp_vc_* kernel and the bytes per second of the
tile-local launch (it reads every word once and writes two words per plane and pixel).  --schedule: wall time of a ten-view
`apd --passes 1 --min-scale 1` run on a tools/make_dataset.py folder, three runs each with --cleanup-on host and --cleanup-on gpu
(best and spread); the first host run keeps the words its passes left (DVP_RAW_VIEWS_DIR) and the words of a full-size pass are then
measured like the synthetic maps.  Appends what it prints to profiles/view_cleanup.txt."""
import argparse
import csv
import glob
import importlib
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MIN_REGION = 1280


def child(path, planes):
    """one stateless call, for the kernel trace"""
    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    capi.clean_selected_views(np.load(path), planes, MIN_REGION)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1552x1032,3104x2064,6208x4128")
    ap.add_argument("--planes", type=int, default=9)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--views", default="")
    ap.add_argument("--views-size", default="")
    ap.add_argument("--schedule", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_cleanup.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.planes)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pkg = importlib.import_module("dvp-mvs_amd")
    capi = pkg.get_capi()
    import np_viewclean as V
    say("# tools/viewclean_bench.py %s" % " ".join(sys.argv[1:]))
    inputs = []
    for s in [x for x in a.sizes.split(",") if x]:
        W, H = map(int, s.split("x"))
        inputs.append(("synthetic", W, H, V.smooth_words(W, H, a.planes)))
    if a.views:
        W, H = map(int, a.views_size.split("x"))
        inputs.append((os.path.basename(a.views), W, H, np.fromfile(a.views, np.uint32).reshape(H, W)))
    if a.schedule:
        W, H = map(int, a.schedule.split("x"))
        src = tempfile.mkdtemp()
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), src, str(W), str(H), "10", "9", "--jpg", "--torch"], stdout=subprocess.DEVNULL)
        raw_dir = tempfile.mkdtemp()
        for where in ("host", "gpu"):
            runs = []
            for k in range(3):
                shutil.rmtree(os.path.join(src, "APD"), ignore_errors=True)
                env = dict(os.environ)
                if where == "host" and k == 0:          # this run also keeps the words its passes left (100 MB per full-size view, written by the background jobs)
                    env["DVP_RAW_VIEWS_DIR"] = raw_dir
                t0 = time.perf_counter()
                subprocess.check_call([os.path.join(ROOT, "dvp-mvs_amd", "apd"), src, "0", "--iters", "3", "--passes", "1", "--min-scale", "1", "--seed", "3", "--cleanup-on", where],
                                      stdout=subprocess.DEVNULL, env=env)
                runs.append(time.perf_counter() - t0)
            say("schedule %dx%d, 10 views, 9 sources, --cleanup-on %s: %.2f s best of 3 (%s)" % (W, H, where, min(runs), ", ".join("%.2f" % r for r in runs)))
        shutil.rmtree(src, ignore_errors=True)
        full = sorted(f for f in os.listdir(raw_dir) if os.path.getsize(os.path.join(raw_dir, f)) == W * H * 4)
        if full:   # the words the last full-size pass of the first view left
            last = max(full, key=lambda f: (int(f[:-4].rsplit("_", 1)[1]), f == full[0]))
            inputs.append(("apd pass " + last, W, H, np.fromfile(os.path.join(raw_dir, last), np.uint32).reshape(H, W)))
        shutil.rmtree(raw_dir, ignore_errors=True)
    for name, W, H, views in inputs:
        px = W * H
        c = capi.Context(W, H, 2)
        c.upload_state(views=views.ravel())
        t = {False: [], True: []}
        for on in (False, True):
            c.set_view_cleanup(on, a.planes, MIN_REGION)
            for _ in range(a.reps + 1):     # (the first repetition allocates the staging / the scratch)
                c.synchronize()
                t0 = time.perf_counter()
                c.download_maps_begin()
                t[on].append(time.perf_counter() - t0)
                got = c.download_maps_finish()[2].reshape(H, W)
        c.close()
        os.environ["OMP_NUM_THREADS"] = "8"
        th = 1e9
        for _ in range(2 if px > 8000000 else 3):
            t0 = time.perf_counter()
            want = V.mirror_clean(views, a.planes, MIN_REGION)
            th = min(th, time.perf_counter() - t0)
        clear = np.mean([(((views >> np.uint32(b)) & 1) == 0).mean() for b in range(a.planes)])
        say("%s %dx%d, %d planes (%.1f %% of the bits clear, %.2f %% of the words changed): scratch %.1f MB; dvp_download_maps_begin %.3f ms with the clean-up off, "
            "%.3f ms with it on; host mirror (8 threads) %.1f ms; words identical to the host mirror's: %s"
            % (name, W, H, a.planes, 100 * clear, 100.0 * (want != views).mean(), 8.0 * a.planes * px / 1e6, min(t[False][1:]) * 1e3, min(t[True][1:]) * 1e3, th * 1e3,
               bool(np.array_equal(got, want))))
        if a.stages and shutil.which("rocprofv3"):
            d = tempfile.mkdtemp()
            np.save(os.path.join(d, "views.npy"), views)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "vc", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "--child", os.path.join(d, "views.npy"), "--planes", str(a.planes)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
            for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                rows = [r for r in csv.DictReader(open(f)) if "dvp_vc_" in r.get("Name", "")]
                tot = sum(float(r.get("TotalDurationNs", 0)) for r in rows)
                for r in rows:
                    ns = float(r.get("TotalDurationNs", 0))
                    extra = ""
                    if "dvp_vc_tiles" in r["Name"] and ns > 0:
                        extra = "  %.0f GB/s (4 + 8 x %d bytes per pixel)" % ((4 + 8 * a.planes) * px / ns, a.planes)
                    say("    %-28s %8.3f ms  %5.1f %%%s" % (r["Name"].split("(")[0], ns / 1e6, 100 * ns / max(tot, 1), extra))
                say("    all four launches: %.3f ms, %.3f ns per pixel and plane" % (tot / 1e6, tot / max(px * a.planes, 1)))
            shutil.rmtree(d, ignore_errors=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
