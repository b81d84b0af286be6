#!/usr/bin/env python3
"""The weak update in the regime of the default schedule's last level, on its three image formats (dvp_image_format):
a REFINE_ITER pass with geometric consistency at 3104x2064, S = 9, ~25 % WEAK pixels (workloads.quarter_level_pass), timed per
launch site with dvp_get_timings.

  f16  the scene's 8-bit images box-filtered 2x2 (multiples of 0.25): format 2, binary16 planes
  f32  the same images with DVP_NO_IMAGES16=1: format 0, float planes (what such levels read before format 2)
  u8   the unfiltered 8-bit images: format 1, byte planes (the integer twin)

The three contexts are prepared once; the timed passes (dvp_restore_state + dvp_run_patchmatch) alternate f16, f32, u8 for
--repeats rounds.  The f16 and f32 runs must leave identical buffers.  One JSON document on stdout (and in --out).
usage: half_planes_bench.py [--repeats 5] [--out profiles/r07_half_planes.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUFFERS = ["planes", "costs", "selected_views", "view_weight", "weak_info", "radius", "fit_planes", "edge_neigh", "candidate",
           "weak_nearest_strong", "weak_reliable", "neighbours", "complex", "label_boundary"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3104)
    ap.add_argument("--height", type=int, default=2064)
    ap.add_argument("--sources", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--weak", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()      # torch's HIP runtime before libdvp_mvs_hip.so (the order bench.py uses)
    wl = importlib.import_module("dvp-mvs_amd.workloads")
    W, H, S, iters = args.width, args.height, args.sources, args.iters
    variants = (("f16", "box", {}, 2), ("f32", "box", {"DVP_NO_IMAGES16": "1"}, 0), ("u8", "int", {}, 1))
    eng = {}
    for tag, images, env, fmt in variants:
        env = dict({"DVP_NO_IMAGES8": None, "DVP_NO_IMAGES16": None}, **env)
        eng[tag] = wl.quarter_level_pass(W, H, S, iters, args.weak, images=images, env=env)["g"]
        got = eng[tag].image_format()
        if got != fmt:
            raise SystemExit("%s: image format %d, expected %d" % (tag, got, fmt))
    weak_frac = eng["f16"].weak_count() / float(W * H)
    times = {tag: dict(weak_update=[], total=[]) for tag, *_ in variants}
    identical = None
    for rep in range(args.repeats + 1):          # round 0 warms up (code objects, first touch of the planes) and is not counted
        for tag, *_ in variants:
            g = eng[tag]
            g.restore_state()
            g.timings(reset=True)
            g.run_patchmatch()
            t = g.timings()
            if rep > 0:
                times[tag]["weak_update"].append(t["stage_ms"]["weak_update"])
                times[tag]["total"].append(t["total_ms"])
        if rep == 0:
            diff = {n: int(np.count_nonzero(eng["f16"].get(n).view(np.uint8) != eng["f32"].get(n).view(np.uint8))) for n in BUFFERS}
            identical = all(v == 0 for v in diff.values())
            if not identical:
                raise SystemExit("f16 and f32 runs differ: %s" % {k: v for k, v in diff.items() if v})
    summ = {}
    for tag, *_ in variants:
        w = times[tag]["weak_update"]
        summ[tag] = dict(weak_update_ms_median=round(statistics.median(w), 2), weak_update_ms_min=round(min(w), 2),
                         weak_update_ms_max=round(max(w), 2), weak_update_ms_runs=[round(x, 2) for x in w],
                         pass_total_ms_median=round(statistics.median(times[tag]["total"]), 2),
                         pass_total_ms_runs=[round(x, 2) for x in times[tag]["total"]])
    med = {tag: summ[tag]["weak_update_ms_median"] for tag in summ}
    doc = dict(tool="tools/half_planes_bench.py", size="%dx%d" % (W, H), sources=S, iterations=iters, state="REFINE_ITER",
               geom_consistency=1, weak_fraction=round(weak_frac, 4), repeats=args.repeats, order="alternating f16, f32, u8 per round",
               per_pass=summ, f16_and_f32_buffers_identical=identical,
               ratios=dict(f16_over_f32=round(med["f16"] / med["f32"], 3), f16_over_u8=round(med["f16"] / med["u8"], 3),
                           f32_over_u8=round(med["f32"] / med["u8"], 3)))
    for g in eng.values():
        g.close()
    s = json.dumps(doc, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
