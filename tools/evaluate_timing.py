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
  --refine        the alignment refinement (dvp_cloud_refine_alignment; lines go to profiles/evaluate_refine.txt): the reconstruction
                  moved by a rigid matrix and given its inverse, perturbed by a tenth of a degree and a few centimetres, the three
                  protocol stages at tau = 1 cm; the call as shipped and the laps of a serialised run, both search forms and both
                  neighbourhoods at FORM_POINTS and the wave form with both neighbourhoods at POINTS (the lane form stays at
                  FORM_POINTS, as under --device), and dvp_cloud_evaluate / dvp_cloud_evaluate_prepared at POINTS on the clouds and with the
                  options of --device and --prepare, for comparison with the profiles they have
  --refine-host   no device: the serial host text (tests/cloudicp_host refine) on the sources of a square of 1 / 32 of the side against
                  the targets within the first stage's distance around it, scaled by the source counts and labelled as such, and a
                  float64 ICP around scipy's cKDTree at FORM_POINTS
  --scans         the observed-space accuracy against laser scans (dvp_cloud_evaluate_scans; lines go to profiles/evaluate_scans.txt):
                  a synthetic hall of 16 x 12 x 7.5 m seen by four scanners, each a sweep of SCAN_POINTS returns (default 10 M) in
                  sweep order, and a reconstruction of POINTS points of which 90 % lie on the walls, 8 % behind them and 2 % inside
                  the hall; at cube sizes 1 024 and 2 048 the call as shipped against plain dvp_cloud_evaluate_prepared on the same
                  clouds, the laps of a serialised run, and the serial host text (tests/cloudscan_host gaps) on every 64th point of the
                  scans and of the reconstruction, scaled by the point counts and labelled as such
usage: evaluate_timing.py [--device] [--host] [--kd] [--prepare] [--refine] [--refine-host] [--scans] [POINTS [FORM_POINTS | SCAN_POINTS]]"""
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


TAU = 0.01
REFINE_STAGES = [(TAU, 80 * TAU, 20), (TAU / 2, 20 * TAU, 20), (TAU / 2, 2 * TAU, 20)]


def refine_scene(points):
    """(moved reconstruction, truth, the known matrix that brings it back, that matrix perturbed, side)"""
    import np_cloudprep as P
    recon, truth, side = clouds(points)
    m = P.rotation(25.0, -15.0, [3.0, -2.0, 1.5]).reshape(4, 4)
    moved = np.ascontiguousarray((recon.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32))
    known = np.linalg.inv(m)
    wrong = P.rotation(0.1, -0.05, [0.03, -0.02, 0.025]).reshape(4, 4)
    return moved, truth, known.reshape(-1), (wrong @ known).reshape(-1), side


def refine_lines(lines, points, form_points):
    import np_cloudicp as C
    import np_cloudprep as P
    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    tol = N.DEFAULT_TOLERANCES
    capi.cloud_evaluate(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), tol)      # the runtime's start-up
    for n, forms in ((form_points, (("wave", "125"), ("wave", "27"), ("lane", "125"), ("lane", "27"))), (points, (("wave", "27"), ("wave", "125")))):
        moved, truth, known, initial, side = refine_scene(n)
        first = None
        for form, cells in forms:
            os.environ["DVP_CLOUD_QUERY"], os.environ["DVP_CLOUD_ICP_CELLS"] = form, cells
            os.environ.pop("DVP_CLOUD_TIMING", None)
            t0 = time.perf_counter()
            got = capi.cloud_refine_alignment(moved, truth, REFINE_STAGES, initial)
            plain = 1e3 * (time.perf_counter() - t0)
            os.environ["DVP_CLOUD_TIMING"] = "1"
            t0 = time.perf_counter()
            again, text = with_stderr(lambda: capi.cloud_refine_alignment(moved, truth, REFINE_STAGES, initial))
            dt = 1e3 * (time.perf_counter() - t0)
            os.environ.pop("DVP_CLOUD_TIMING", None)
            assert again["matrix"].tobytes() == got["matrix"].tobytes() and (first is None or first["matrix"].tobytes() == got["matrix"].tobytes())
            first = got
            lines.append("device, %d + %d points on %.1f x %.1f m, %s form, %s cells: dvp_cloud_refine_alignment as shipped (wall time) %.0f ms; with DVP_CLOUD_TIMING=1, which waits "
                         "for the stream after every phase, %.0f ms; steps per stage %s; start %.4f deg %.4f m, refined %.6f deg %.6f m from the known matrix" % (
                             (n, n, side, side, form, cells, plain, dt, [len([g for g in got["log"] if g[0] == s]) for s in range(3)]) + C.motion_errors(initial, known) + C.motion_errors(got["matrix"], known)))
            steps = [ln for ln in text.splitlines() if "step timing" in ln]
            for s in range(3):      # the first step of every stage, in full; the laps of the others differ little
                at = sum(len([g for g in got["log"] if g[0] == k]) for k in range(s))
                if at < len(steps):
                    lines.append("  stage %d (voxel %.9g, distance %.9g), %d sources, rmse %.6f -> %.6f: %s" % (
                        s, REFINE_STAGES[s][0], REFINE_STAGES[s][1], got["log"][at][2], got["log"][at][4], [g for g in got["log"] if g[0] == s][-1][4], steps[at]))
            lines += ["  " + ln for ln in text.splitlines() if "step timing" not in ln][:6]
            for ln in lines[-10:]:
                print(ln, flush=True)
        del os.environ["DVP_CLOUD_QUERY"], os.environ["DVP_CLOUD_ICP_CELLS"]
        if n == points:      # the two existing entries beside it, for comparison with profiles/evaluate.txt and evaluate_prepare.txt
            t = []
            recon = clouds(n)[0]
            for _ in range(2):
                t0 = time.perf_counter()
                capi.cloud_evaluate(recon, truth, tol)
                t.append(1e3 * (time.perf_counter() - t0))
            del recon
            crop = P.crop_of(2, 1.0, 3.5, P.polygon_3d(2, 0.1 * side + 0.8 * side * np.array(P.CONCAVE_12)))
            pr, pt = P.prep(known, crop, 0.5 * float(np.float32(tol[0]))), P.prep(None, crop, 0.5 * float(np.float32(tol[0])))
            for _ in range(2):
                t0 = time.perf_counter()
                res = capi.cloud_evaluate_prepared(moved, truth, tol, pr, pt)
                t.append(1e3 * (time.perf_counter() - t0))
            lines.append("  beside it: dvp_cloud_evaluate on the unmoved clouds (wall time, two calls) %.0f %.0f ms; dvp_cloud_evaluate_prepared with the known matrix, the 12-gon prism and voxel %.9g (two calls) "
                         "%.0f %.0f ms; accuracy %s (percent)" % (t[0], t[1], 0.5 * float(np.float32(tol[0])), t[2], t[3], " ".join("%.3f" % (100 * v) for v in res["accuracy"])))
            print(lines[-1], flush=True)


def refine_host_lines(lines, points, form_points):
    import np_cloudicp as C
    import np_cloudprep as P
    recon, truth, side = clouds(points)
    m = np.linalg.inv(refine_scene(1000)[2].reshape(4, 4))
    d = REFINE_STAGES[0][1]
    lo, hi = side / 2, side / 2 + side / 32

    def inside(p, margin):
        return (p[:, :2] >= lo - margin).all(1) & (p[:, :2] < hi + margin).all(1)
    src = recon[inside(recon, 0.0)]
    moved = np.ascontiguousarray((src.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32))
    tgt = truth[inside(truth, 1.01 * d)]
    _, _, known, initial, _ = refine_scene(1000)
    C.build_program()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        rc, err, got = C.serial_refine(moved, tgt, tmp, initial, None, REFINE_STAGES)
        dt = time.perf_counter() - t0
    assert rc == 0, err
    lines.append("serial host text (tests/cloudicp_host refine, one thread) on the %d sources of a %.2f m square in the middle of the %d + %d points against the %d targets within %.9g m "
                 "around it: %.1f s for %s steps per stage; SCALED by the source counts to the whole clouds: %.0f s" % (
                     len(src), hi - lo, points, points, len(tgt), d, dt, [len([g for g in got["log"] if g[0] == s]) for s in range(3)], dt * points / len(src)))
    print(lines[-1], flush=True)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        lines.append("scipy is not importable here: no cKDTree line")
        return
    moved, truth, known, initial, side = refine_scene(form_points)
    t0 = time.perf_counter()
    M, steps = np.asarray(initial, np.float64).reshape(4, 4), []
    for v, dist, k in REFINE_STAGES:
        s64 = P.prepare(moved, M.reshape(-1), None, v)["xyz"].astype(np.float64)
        t64 = P.prepare(truth, None, None, v)["xyz"].astype(np.float64)
        tree = cKDTree(t64)
        D, last = np.eye(4), None
        for it in range(1, k + 1):
            p = s64 @ D[:3, :3].T + D[:3, 3]
            e, j = tree.query(p, distance_upper_bound=dist, workers=16)
            has = np.isfinite(e)
            now = (has.mean(), np.sqrt((e[has] ** 2).mean()))
            if last is not None and abs(now[0] - last[0]) < 1e-6 and abs(now[1] - last[1]) < 1e-6:
                break
            last = now
            a, b = p[has], t64[j[has]]
            U, _, Vt = np.linalg.svd((a - a.mean(0)).T @ (b - b.mean(0)))
            R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
            E = np.eye(4)
            E[:3, :3], E[:3, 3] = R, b.mean(0) - R @ a.mean(0)
            D = E @ D
        steps.append(it)
        M = D @ M
    dt = time.perf_counter() - t0
    lines.append("float64 ICP around scipy cKDTree.query(..., distance_upper_bound=d, workers=16) with numpy's preparation, %d + %d points: %.1f s for %s steps per stage; refined %.6f deg "
                 "%.6f m from the known matrix" % ((form_points, form_points, dt, steps) + C.motion_errors(M.reshape(-1), known)))
    print(lines[-1], flush=True)


HALL = np.array([16.0, 12.0, 7.5])
HALL_SCANNERS = [[3.0, 2.5, 1.6], [12.5, 3.0, 1.7], [8.0, 9.0, 1.5], [2.5, 9.5, 1.8]]


def hall_hits(origin, direction):
    """where the rays from origin (3,) along direction (n, 3) leave the hall [0, HALL]"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(direction > 0, (HALL - origin) / direction, np.where(direction < 0, -origin / direction, np.inf))
    return origin + direction * t.min(1)[:, None]


def hall_scene(points, scan_points, seed=11):
    """(scans [(xyz in the scanner's frame, matrix)], reconstruction): every scan a sweep of rows of equal elevation, as a terrestrial
    scanner stores it"""
    import np_cloudprep as P
    rng = np.random.default_rng(seed)
    scans = []
    rows = int(np.sqrt(scan_points / 2))
    for k, o in enumerate(HALL_SCANNERS):
        i = np.arange(scan_points)
        azimuth, elevation = 2 * np.pi * (i % (2 * rows)) / (2 * rows), np.pi * ((i // (2 * rows)) + 0.5) / (scan_points / (2 * rows)) - np.pi / 2
        d = np.stack([np.cos(elevation) * np.cos(azimuth), np.cos(elevation) * np.sin(azimuth), np.sin(elevation)], 1)
        hit = hall_hits(np.asarray(o), d) + rng.normal(0, 0.001, (scan_points, 3))
        m = P.rotation(30.0 * k, 0.0, o).reshape(4, 4)
        scans.append((np.ascontiguousarray(((hit - m[:3, 3]) @ m[:3, :3]).astype(np.float32)), m.reshape(-1)))      # q = R^T (g - o)
        del d, hit
    d = rng.normal(0, 1, (points, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    centre = HALL / 2 + rng.uniform(-2, 2, (points, 3)) * [1, 1, 0.5]
    wall = hall_hits(centre, d)
    kind = rng.random(points)
    recon = wall + rng.normal(0, 0.004, (points, 3))
    behind = kind < 0.08
    recon[behind] = wall[behind] + d[behind] * rng.uniform(0.6, 2.0, (int(behind.sum()), 1))
    inside = kind > 0.98
    recon[inside] = centre[inside] + (wall[inside] - centre[inside]) * rng.uniform(0.1, 0.8, (int(inside.sum()), 1))
    return scans, np.ascontiguousarray(recon.astype(np.float32))


def scans_lines(lines, points, scan_points):
    import np_cloudscan as S
    capi = importlib.import_module("dvp-mvs_amd").get_capi()
    tol = N.DEFAULT_TOLERANCES
    scans, recon = hall_scene(points, scan_points)
    truth = S.truth_cloud(scans)
    capi.cloud_evaluate(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), tol)      # the runtime's start-up
    os.environ.pop("DVP_CLOUD_TIMING", None)
    plain = []
    for _ in range(2):
        t0 = time.perf_counter()
        base = capi.cloud_evaluate_prepared(recon, truth, tol)
        plain.append(1e3 * (time.perf_counter() - t0))
    lines.append("device, a hall of %g x %g x %g m, %d scans of %d points each in sweep order, a reconstruction of %d points: plain dvp_cloud_evaluate_prepared on the reconstruction and "
                 "the truth cloud of the scans (wall time, two calls) %s ms; accuracy over all points %s (percent)" % (
                     HALL[0], HALL[1], HALL[2], len(scans), scan_points, points, " ".join("%.0f" % v for v in plain), " ".join("%.3f" % (100 * v) for v in base["accuracy"])))
    print(lines[-1], flush=True)
    for R in (1024, 2048):
        shipped = []
        for _ in range(2):
            t0 = time.perf_counter()
            got = capi.cloud_evaluate_scans(recon, scans, tol, cube_size=R)
            shipped.append(1e3 * (time.perf_counter() - t0))
        os.environ["DVP_CLOUD_TIMING"] = "1"
        t0 = time.perf_counter()
        again, text = with_stderr(lambda: capi.cloud_evaluate_scans(recon, scans, tol, cube_size=R))
        dt = time.perf_counter() - t0
        os.environ.pop("DVP_CLOUD_TIMING", None)
        assert all(np.array_equal(got[k], again[k]) for k in ("within_recon", "within_truth", "used", "free_space")) and np.array_equal(got["within_recon"], base["within_recon"])
        lines.append("  cube size %d: dvp_cloud_evaluate_scans as shipped (wall time, two calls) %s ms; with DVP_CLOUD_TIMING=1, which waits for the stream after every phase, the call %.0f ms" % (
            R, " ".join("%.0f" % v for v in shipped), 1e3 * dt))
        lines += ["    " + ln for ln in text.splitlines()]
        lines.append("    accurate %s, free_space %s, unobserved %s; observed-space accuracy %s, completeness %s (percent)" % (
            got["within_recon"].tolist(), got["free_space"].tolist(), got["unobserved"].tolist(), " ".join("%.3f" % (100 * v) for v in got["accuracy"]),
            " ".join("%.3f" % (100 * v) for v in got["completeness"])))
        for ln in lines[-(3 + len(text.splitlines())):]:
            print(ln, flush=True)
    S.build_program()
    with tempfile.TemporaryDirectory() as tmp:
        part = [(x[::64], m) for x, m in scans]
        q = recon[::64]
        for R in (1024, 2048):
            t0 = time.perf_counter()
            rc, err, out = S.serial_gaps(part, q, R, tmp)
            dt = time.perf_counter() - t0
            assert rc == 0, err
            lines.append("serial host text (tests/cloudscan_host gaps, one thread), cube size %d: every 64th point, %d scan points and %d queries, truth points, maps and gaps %.1f s with the files' "
                         "reading and writing; SCALED by the point counts to the whole scene: %.0f s (the distances are profiles/evaluate.txt's)" % (
                             R, sum(len(x) for x, _ in part), len(q), dt, dt * 64))
            print(lines[-1], flush=True)


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
    if "--refine" in sys.argv or "--refine-host" in sys.argv:
        if "--refine" in sys.argv:
            refine_lines(lines, points, form_points)
        else:
            refine_host_lines(lines, points, form_points)
        with open(os.path.join(ROOT, "profiles", "evaluate_refine.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    if "--scans" in sys.argv:
        scans_lines(lines, points, int(args[1]) if len(args) > 1 else 10000000)
        with open(os.path.join(ROOT, "profiles", "evaluate_scans.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    if "--prepare" in sys.argv:
        prepare_lines(lines, points)
        with open(os.path.join(ROOT, "profiles", "evaluate_prepare.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    with open(os.path.join(ROOT, "profiles", "evaluate.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
