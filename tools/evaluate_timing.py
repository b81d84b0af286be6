#!/usr/bin/env python3
"""Times `apd --evaluate`'s query (dvp_cloud_evaluate) on cuda:0 and appends the lines to profiles/evaluate.txt.  The data: a
synthetic surface cloud of the size of a ten-view full-size fusion (default 45 M points, 50 000 per square metre: noisy, 2 % outliers,
92 % of the area) and a truth cloud of the same size sampled on its own, in shuffled order, with the six default tolerances.
  --device        the call as shipped (wall time, nothing waiting between the phases) and, from a second, serialised run with
                  DVP_CLOUD_TIMING=1 (a wait for the stream after every phase), the phases' times: in the default query form at
                  POINTS, and in both query forms at FORM_POINTS points of the same density (the lane form at full size takes minutes)
  --host          the serial host text (tests/cloudeval_host, grid walk) on the queries of a square of 1 / 16 of the side - 1 / 256
                  of the points - against the targets around them, scaled by the query counts and labelled as such
  --kd            scipy's cKDTree.query(..., distance_upper_bound=T, workers=16) in float64 on the same data, both directions
  --prepare       the preparation in front of the query (dvp_cloud_evaluate_prepared; lines go to profiles/evaluate_prepare.txt): the
                  reconstruction moved by a rigid matrix and given its inverse, both clouds cropped with a concave 12-gon prism over
                  the middle of the scene and down-sampled with voxels of half the smallest tolerance; the call as shipped against
                  plain dvp_cloud_evaluate on the same clouds, the phases from a serialised run, and the serial host text
                  (tests/cloudprep_host) on the first 1 / 16 of each cloud, scaled by the point counts and labelled as such
usage: evaluate_timing.py [--device] [--host] [--kd] [--prepare] [POINTS [FORM_POINTS]]"""
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
import np_evaluate as N  # noqa: E402

DENSITY = 50000.0      # points per square metre of surface


def surface(x, y):
    return 2.0 + 0.5 * np.sin(0.7 * x) * np.cos(0.5 * y) + 0.02 * x


def clouds(points, seed=7):
    """(recon, truth, side): recon in rows of x (a fusion writes view after view), truth in no useful order"""
    rng = np.random.default_rng(seed)
    side = float(np.sqrt(points / DENSITY))
    x, y = np.sort(rng.random(points, np.float32)) * np.float32(0.92 * side), rng.random(points, np.float32) * np.float32(side)
    z = surface(x, y) + rng.normal(0, 0.004, points).astype(np.float32)
    out = rng.random(points) < 0.02
    z[out] += rng.uniform(-1, 1, int(out.sum())).astype(np.float32)
    recon = np.stack([x, y, z], 1).astype(np.float32)
    x, y = rng.random(points, np.float32) * np.float32(side), rng.random(points, np.float32) * np.float32(side)
    truth = np.stack([x, y, surface(x, y)], 1).astype(np.float32)
    return recon, truth, side


def with_stderr(fn):
    """(fn's result, what the library wrote to stderr meanwhile)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode().strip()


def device_lines(lines, points, form_points):
    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    tol = N.DEFAULT_TOLERANCES
    capi.cloud_evaluate(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), tol)      # the runtime's start-up
    results = {}
    for n, forms in ((form_points, ("wave", "lane")), (points, ("wave",))):
        recon, truth, side = clouds(n)
        for form in forms:
            os.environ["DVP_CLOUD_QUERY"] = form
            # the call as a user makes it: nothing waits between the phases
            os.environ.pop("DVP_CLOUD_TIMING", None)
            plain = []
            for _ in range(2):
                t0 = time.perf_counter()
                got = capi.cloud_evaluate(recon, truth, tol)
                plain.append(1e3 * (time.perf_counter() - t0))
            results[(n, form)] = got
            # ... and once more with a wait after every phase, for the phases' shares: a serialised run, not the shipped path
            os.environ["DVP_CLOUD_TIMING"] = "1"
            t0 = time.perf_counter()
            again, text = with_stderr(lambda: capi.cloud_evaluate(recon, truth, tol))
            dt = time.perf_counter() - t0
            assert all(np.array_equal(got[k], again[k]) for k in ("within_recon", "within_truth", "used"))
            lines.append("device, %d + %d points on %.1f x %.1f m, %s form: the call as shipped (wall time around capi.cloud_evaluate, two calls) %s ms; "
                         "with DVP_CLOUD_TIMING=1, which waits for the stream after every phase, the call %.0f ms; %s" % (
                             n, n, side, side, form, " ".join("%.0f" % v for v in plain), 1e3 * dt, text))
            print(lines[-1], flush=True)
        same = all(np.array_equal(results[(n, forms[0])][k], results[(n, f)][k]) for f in forms for k in ("within_recon", "within_truth", "used"))
        got = results[(n, forms[0])]
        lines.append("  %saccuracy %s, completeness %s (percent)" % (
            "counts equal between the forms: %s; " % same if len(forms) > 1 else "", " ".join("%.3f" % (100 * v) for v in got["accuracy"]), " ".join("%.3f" % (100 * v) for v in got["completeness"])))
        print(lines[-1], flush=True)


def host_lines(lines, points):
    recon, truth, side = clouds(points)
    T = N.DEFAULT_TOLERANCES[-1]
    lo, hi = side / 2, side / 2 + side / 16      # a square in the middle; its targets reach one cell edge further on every side

    def inside(p, margin):
        return p[((p[:, :2] >= lo - margin) & (p[:, :2] < hi + margin)).all(1)]
    N.build_program()
    scaled = 0.0
    parts = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, query, target in (("recon -> truth", recon, truth), ("truth -> recon", truth, recon)):
            q, t = inside(query, 0.0), inside(target, 1.01 * T)
            t0 = time.perf_counter()
            rc, err, d2 = N.serial_distances(q, t, T, tmp, "grid")
            dt = time.perf_counter() - t0
            assert rc == 0, err
            scaled += dt * points / len(q)
            parts.append("%s: %d queries against the %d targets around them %.1f s" % (name, len(q), len(t), dt))
    lines.append("serial host text (tests/cloudeval_host distances ... grid, one thread) on the queries of a %.2f m square in the middle of the %d + %d points: %s; SCALED by the query "
                 "counts to the whole clouds: %.0f s" % (hi - lo, points, points, "; ".join(parts), scaled))
    print(lines[-1], flush=True)


def kd_lines(lines, points):
    from scipy.spatial import cKDTree
    recon, truth, _ = clouds(points)
    T = float(np.float32(N.DEFAULT_TOLERANCES[-1]))
    r64, t64 = recon.astype(np.float64), truth.astype(np.float64)
    total = 0.0
    parts = []
    for name, query, target in (("recon -> truth", r64, t64), ("truth -> recon", t64, r64)):
        t0 = time.perf_counter()
        tree = cKDTree(target)
        t1 = time.perf_counter()
        d, _ = tree.query(query, distance_upper_bound=T, workers=16)
        t2 = time.perf_counter()
        parts.append("%s: build %.1f s, query %.1f s, %.3f %% within %.9g" % (name, t1 - t0, t2 - t1, 100.0 * np.isfinite(d).mean(), T))
        total += t2 - t0
        del tree, d
    lines.append("scipy cKDTree.query(..., distance_upper_bound=%.9g, workers=16), float64, %d + %d points: %.1f s in all; %s" % (T, points, points, total, "; ".join(parts)))
    print(lines[-1], flush=True)


def prepare_lines(lines, points):
    import np_cloudprep as P
    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    tol = N.DEFAULT_TOLERANCES
    recon, truth, side = clouds(points)
    m = P.rotation(25.0, -15.0, [3.0, -2.0, 1.5]).reshape(4, 4)
    moved = np.ascontiguousarray((recon.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32))
    inverse = np.linalg.inv(m).reshape(-1)
    crop = P.crop_of(2, 1.0, 3.5, P.polygon_3d(2, 0.1 * side + 0.8 * side * np.array(P.CONCAVE_12)))
    voxel = 0.5 * float(np.float32(tol[0]))
    pr, pt = P.prep(inverse, crop, voxel), P.prep(None, crop, voxel)
    capi.cloud_evaluate(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), tol)      # the runtime's start-up
    os.environ.pop("DVP_CLOUD_TIMING", None)
    plain, prepared = [], []
    for _ in range(2):
        t0 = time.perf_counter()
        capi.cloud_evaluate(recon, truth, tol)
        plain.append(1e3 * (time.perf_counter() - t0))
    for _ in range(2):
        t0 = time.perf_counter()
        got = capi.cloud_evaluate_prepared(moved, truth, tol, pr, pt)
        prepared.append(1e3 * (time.perf_counter() - t0))
    os.environ["DVP_CLOUD_TIMING"] = "1"
    t0 = time.perf_counter()
    again, text = with_stderr(lambda: capi.cloud_evaluate_prepared(moved, truth, tol, pr, pt))
    dt = time.perf_counter() - t0
    os.environ.pop("DVP_CLOUD_TIMING", None)
    assert all(np.array_equal(got[k], again[k]) for k in ("within_recon", "within_truth", "used", "counts"))
    lines.append("device, %d + %d points on %.1f x %.1f m, transform + crop (12-gon prism) + voxel %.9g: plain dvp_cloud_evaluate on the unprepared clouds (wall time, two calls) %s ms; "
                 "dvp_cloud_evaluate_prepared as shipped (wall time, two calls) %s ms; with DVP_CLOUD_TIMING=1, which waits for the stream after every phase, the call %.0f ms" % (
                     points, points, side, side, voxel, " ".join("%.0f" % v for v in plain), " ".join("%.0f" % v for v in prepared), 1e3 * dt))
    lines += ["  " + ln for ln in text.splitlines()]
    lines.append("  counts (finite, after the transform, in the crop volume, output): reconstruction %s, ground truth %s; accuracy %s, completeness %s (percent)" % (
        got["counts"][0].tolist(), got["counts"][1].tolist(), " ".join("%.3f" % (100 * v) for v in got["accuracy"]), " ".join("%.3f" % (100 * v) for v in got["completeness"])))
    P.build_program()
    part = points // 16
    scaled, parts = 0.0, []
    with tempfile.TemporaryDirectory() as tmp:
        for name, xyz, one in (("reconstruction", moved, pr), ("ground truth", truth, pt)):
            sub = xyz[:: 16][:part]      # every 16th point: the same volume at 1 / 16 of the density
            t0 = time.perf_counter()
            rc, err, out = P.serial(sub, tmp, **one)
            dt = time.perf_counter() - t0
            assert rc == 0, err
            scaled += dt * points / len(sub)
            parts.append("%s: every 16th point, %d points -> %d, %.1f s with the files' reading and writing" % (name, len(sub), out["counts"][3], dt))
    lines.append("serial host text (tests/cloudprep_host prepare, one thread): %s; SCALED by the point counts to the whole clouds: %.0f s" % ("; ".join(parts), scaled))
    for ln in lines[-(4 + len(text.splitlines())):]:
        print(ln, flush=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    points = int(args[0]) if args else 45000000
    form_points = int(args[1]) if len(args) > 1 else 2000000
    lines = ["$ tools/evaluate_timing.py " + " ".join(sys.argv[1:])]
    if "--device" in sys.argv:
        device_lines(lines, points, form_points)
    if "--host" in sys.argv:
        host_lines(lines, points)
    if "--kd" in sys.argv:
        kd_lines(lines, points)
    if "--prepare" in sys.argv:
        prepare_lines(lines, points)
        with open(os.path.join(ROOT, "profiles", "evaluate_prepare.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    with open(os.path.join(ROOT, "profiles", "evaluate.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
