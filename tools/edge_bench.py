#!/usr/bin/env python3
"""Cost of the edge prior on the device (csrc/dvp_edges.hip) against the host's EdgeSegment.

  python3 tools/edge_bench.py [--sizes 1552x1032,3104x2064,6208x4128] [--reps N] [--stages] [--schedule WxH [--apd PATH,...]]

Per size, on a two-image context whose image 0 is a smooth field with steps and noise: wall time of dvp_edge_map_begin up to
the end of its device work (the call itself does not wait; the stream is synchronised for the measurement), of
dvp_edge_map_finish (the copy to the host), and of `test_host --edges` — the host mirror's EdgeSegment on the same bytes, a
process that also reads the image file and writes the map, with OMP_NUM_THREADS 1 and 2 (two = a helper's team; EdgeSegment
itself is one loop nest on one thread).  --stages runs each size once more under `rocprofv3 --kernel-trace --stats` in a child
process and prints the time of every dvp_edge_* kernel.  --schedule: wall time, best of three, of a ten-view
`apd --passes 1 --min-scale 1` run on a tools/make_dataset.py folder with --edges-on host and --edges-on gpu (--apd: other
builds of the driver to run the host mode of, e.g. the parent commit's).  Writes what it prints to profiles/edge_map.txt."""
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


def field(W, H, rs):
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    f = 110 + 60 * np.sin(x / 61.0) * np.cos(y / 47.0) + 40 * (((x // 300) + (y // 220)) % 2)
    f += rs.randint(-25, 26, (H, W)).astype(np.float32)
    return np.clip(f, 0, 255).astype(np.float32)


def context(capi, synth, W, H):
    img = field(W, H, np.random.RandomState(0))
    c = capi.Context(W, H, 2)
    c.set_images([img, img])
    return c, np.rint(img).astype(np.uint8)


def child(size):
    """one begin + finish, for the kernel trace"""
    pkg = importlib.import_module("dvp-mvs_amd")
    W, H = map(int, size.split("x"))
    c, _ = context(pkg.get_capi(), pkg.synth, W, H)
    c.edge_map_begin(True)
    c.edge_map_finish()
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1552x1032,3104x2064,6208x4128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--schedule", default="")
    ap.add_argument("--apd", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_map.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pkg = importlib.import_module("dvp-mvs_amd")
    capi, synth = pkg.get_capi(), pkg.synth
    import np_edges as E
    say("# tools/edge_bench.py %s" % " ".join(sys.argv[1:]))
    for s in [x for x in a.sizes.split(",") if x]:
        W, H = map(int, s.split("x"))
        c, u8 = context(capi, synth, W, H)
        tb, tf = [], []
        for _ in range(a.reps + 1):     # (the first repetition allocates the scratch)
            c.synchronize()
            t0 = time.perf_counter()
            c.edge_map_begin(True)
            t1 = time.perf_counter()
            c.synchronize()
            t2 = time.perf_counter()
            got = c.edge_map_finish()
            t3 = time.perf_counter()
            tb.append((t2 - t0, t1 - t0))
            tf.append(t3 - t2)
        c.close()
        th = {}
        for threads in (1, 2):
            os.environ["OMP_NUM_THREADS"] = str(threads)
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                want = E.host_tool_edges(u8)
                best = min(best, time.perf_counter() - t0)
            th[threads] = best
        same = bool(np.array_equal(got, want))
        px = W * H
        say("%dx%d  begin: %.3f ms to the end of the device work (the call returns after %.3f ms), finish: %.3f ms; %.1f %% edge pixels; "
            "test_host --edges (file in, file out): %.1f ms with 1 thread, %.1f ms with 2; maps identical: %s; device %.2f ns/px"
            % (W, H, min(t[0] for t in tb[1:]) * 1e3, min(t[1] for t in tb[1:]) * 1e3, min(tf[1:]) * 1e3, 100.0 * (got > 0).mean(), th[1] * 1e3, th[2] * 1e3, same,
               min(t[0] for t in tb[1:]) * 1e9 / px))
        if a.stages and shutil.which("rocprofv3"):
            d = tempfile.mkdtemp()
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "edge", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", s],
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
            for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                rows = [r for r in csv.DictReader(open(f)) if "dvp_edge_" in r.get("Name", "")]
                tot = sum(float(r.get("TotalDurationNs", 0)) for r in rows)
                for r in rows:
                    ns = float(r.get("TotalDurationNs", 0))
                    say("    %-28s %8.3f ms  %5.1f %%" % (r["Name"].split("(")[0], ns / 1e6, 100 * ns / max(tot, 1)))
            shutil.rmtree(d, ignore_errors=True)
    if a.schedule:
        W, H = map(int, a.schedule.split("x"))
        builds = [("--edges-on host", os.path.join(ROOT, "dvp-mvs_amd", "apd"), ["--edges-on", "host"]), ("--edges-on gpu", os.path.join(ROOT, "dvp-mvs_amd", "apd"), ["--edges-on", "gpu"])]
        builds += [("other build %s" % p, p, []) for p in a.apd.split(",") if p]
        src = tempfile.mkdtemp()
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), src, str(W), str(H), "10", "9", "--jpg", "--torch"], stdout=subprocess.DEVNULL)
        for name, exe, extra in builds:
            best = 1e9
            for _ in range(3):
                shutil.rmtree(os.path.join(src, "APD"), ignore_errors=True)
                t0 = time.perf_counter()
                subprocess.check_call([exe, src, "0", "--iters", "3", "--passes", "1", "--min-scale", "1", "--seed", "3"] + extra, stdout=subprocess.DEVNULL)
                best = min(best, time.perf_counter() - t0)
            say("schedule %dx%d, 10 views, 9 sources, %s: %.2f s (best of 3)" % (W, H, name, best))
        shutil.rmtree(src, ignore_errors=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
