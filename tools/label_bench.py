#!/usr/bin/env python3
"""Cost of the label prior on the device (csrc/dvp_labels.hip) against the host mirror's LabelSegment.

  python3 tools/label_bench.py [--sizes 1552x1032,3104x2064,6208x4128] [--scales 0,1] [--reps N] [--stages] [--schedule WxH]
                               [--out FILE]

Per size and scale, on a synthetic full-size grey image (flat walls with grain, textured bands and blocks with flat islands, a
ramp): the wall time of dvp_labels_run on a kept job — split by the job's own clock into device part A (upload, two halvings,
Roberts cross, components, region map back), the host middle (outline pass, Hough transform, lines; with the regions and outline
points it saw) and device part B (lines in, resize, clean-up, components, numbering, label map back) — and the host mirror's
LabelSegment on the same bytes with a team of two threads, the team a helper thread of the driver has.  The two maps are
compared at every size; for 6208x4128 this is the only place that does.  --stages runs each size once more under
`rocprofv3 --kernel-trace --stats` in a child process and prints the time of every kernel of the run.  --schedule: wall time of a
ten-view `apd --passes 1 --min-scale 1` run on a tools/make_dataset.py folder, three runs each with --labels-on host and
--labels-on gpu, alternating (best and spread).  Appends what it prints to profiles/label_map.txt."""
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


def picture(W, H):
    rs = np.random.RandomState(17)
    img = np.full((H, W), 90, np.uint8)
    img[:, W // 2:] = 170
    img[H // 3:H // 3 + H // 25, :] = rs.randint(0, 256, (H // 25, W))
    img[:, W // 2 - W // 50:W // 2 + W // 50] = rs.randint(0, 256, (H, 2 * (W // 50)))
    bh, bw = H // 8, W // 10
    for k in range(12):
        y, x = rs.randint(0, H - bh), rs.randint(0, W - bw)
        img[y:y + bh, x:x + bw] = rs.randint(0, 256, (bh, bw))
        img[y + bh // 4:y + bh // 4 + (bh // 16) * (k + 1) // 2, x + bw // 4:x + bw // 4 + (bw // 16) * (k + 1) // 2] = 30 + 15 * k
    x0, x1 = W // 20, W // 2 - W // 20
    img[H - H // 6:H - H // 12, x0:x1] = (np.linspace(20, 250, x1 - x0)[None, :]).astype(np.uint8)
    img += rs.randint(0, 2, (H, W)).astype(np.uint8)
    return img


def child(path, scale):
    """one run on a fresh job, for the kernel trace"""
    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    capi.label_map(np.load(path), scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1552x1032,3104x2064,6208x4128")
    ap.add_argument("--scales", default="0,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--schedule", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--scale", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_map.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.scale)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        del lines[:]

    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    import np_labels as N
    say("# tools/label_bench.py %s" % " ".join(sys.argv[1:]))
    job = capi.LabelJob()
    for s in [x for x in a.sizes.split(",") if x]:
        W, H = map(int, s.split("x"))
        img = picture(W, H)
        for scale in [int(x) for x in a.scales.split(",") if x != ""]:
            best, parts = 1e9, None
            for _ in range(a.reps + 1):        # (the first repetition allocates the scratch)
                t0 = time.perf_counter()
                got = job.run(img, scale)
                dt = time.perf_counter() - t0
                if _ and dt < best:
                    best, parts = dt, job.timings()
            th = 1e9
            for _ in range(2 if W * H > 8000000 else 3):
                t0 = time.perf_counter()
                want = N.mirror(img, scale, threads=2)
                th = min(th, time.perf_counter() - t0)
            lab = want["labels"]
            say("%dx%d scale %d (level %dx%d, %d regions numbered, %.1f %% of the level pixels flat): dvp_labels_run %.2f ms = part A %.2f + host middle %.2f "
                "(%d regions with an outline, %d outline points) + part B %.2f; host mirror LabelSegment (2 threads) %.1f ms; maps identical: %s"
                % (W, H, scale, lab.shape[1], lab.shape[0], len(np.unique(lab[lab > 0])), 100.0 * (lab != 0).mean(), best * 1e3, parts["part_a_ms"], parts["host_ms"],
                   parts["regions"], parts["outline_points"], parts["part_b_ms"], th * 1e3, bool(np.array_equal(got, lab))))
            if a.stages and shutil.which("rocprofv3"):
                d = tempfile.mkdtemp()
                np.save(os.path.join(d, "img.npy"), img)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "lab", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                                "--child", os.path.join(d, "img.npy"), "--scale", str(scale)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
                for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                    rows = [r for r in csv.DictReader(open(f)) if "dvp_lab_" in r.get("Name", "") or "dvp_vc_" in r.get("Name", "")]
                    tot = sum(float(r.get("TotalDurationNs", 0)) for r in rows)
                    for r in rows:
                        ns = float(r.get("TotalDurationNs", 0))
                        say("    %-28s x%-2s %8.3f ms  %5.1f %%" % (r["Name"].split("(")[0], r.get("Calls", "?"), ns / 1e6, 100 * ns / max(tot, 1)))
                    say("    all kernels of the run: %.3f ms" % (tot / 1e6))
                shutil.rmtree(d, ignore_errors=True)
            flush()
    job.close()
    if a.schedule:
        W, H = map(int, a.schedule.split("x"))
        src = tempfile.mkdtemp()
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), src, str(W), str(H), "10", "9", "--jpg", "--torch"], stdout=subprocess.DEVNULL)
        runs = dict(host=[], gpu=[])
        for k in range(3):
            for where in ("host", "gpu"):
                shutil.rmtree(os.path.join(src, "APD"), ignore_errors=True)
                t0 = time.perf_counter()
                subprocess.check_call([os.path.join(ROOT, "dvp-mvs_amd", "apd"), src, "0", "--iters", "3", "--passes", "1", "--min-scale", "1", "--seed", "3", "--labels-on", where],
                                      stdout=subprocess.DEVNULL)
                runs[where].append(time.perf_counter() - t0)
        for where in ("host", "gpu"):
            say("schedule %dx%d, 10 views, 9 sources, --labels-on %s: %.2f s best of 3, spread %.2f s (%s)"
                % (W, H, where, min(runs[where]), max(runs[where]) - min(runs[where]), ", ".join("%.2f" % r for r in runs[where])))
        shutil.rmtree(src, ignore_errors=True)
        flush()


if __name__ == "__main__":
    main()
