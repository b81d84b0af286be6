"""TEST INFRASTRUCTURE: the alignment refinement of `apd --evaluate --refine-alignment` (csrc/dvp_cloudicp.hpp) read independently in
numpy - brute-force binary32 distances with argmin (whose first minimum is the smallest index), binary64 leaves, the tree sums as
a[0::2] + a[1::2] repeated -, an independent float64 Kabsch and a float64 ICP, the case table that the host and the device tests share,
and the runner of tests/cloudicp_host."""
import os
import subprocess

import numpy as np

import np_cloudprep as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "cloudicp_host", "cloudicp_host")
IDENTITY = np.eye(4).reshape(-1)

cloud = P.cloud


def padded(n):
    N = 1
    while N < n:
        N *= 2
    return N


# ---- the definition -------------------------------------------------------------------------------------------------------------
def image(src, D):
    """(p' (n, 3) float64, r (n, 3) float32, ok (n,) bool)"""
    x = cloud(src)
    p = x.astype(np.float64)
    m = np.asarray(D, np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        pp = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], 1)
        r = pp.astype(np.float32)
    return pp, r, np.isfinite(x).all(1) & np.isfinite(r).all(1)


def reference_point(tgt):
    t = cloud(tgt)
    if len(t) == 0:
        return np.zeros(3)
    lo, hi = t.min(0).astype(np.float64), t.max(0).astype(np.float64)
    return lo + (hi - lo) * 0.5


def tree_sum(leaves):
    """the balanced pairwise tree over the rows of a (N, k) array, N a power of two"""
    a = np.asarray(leaves, np.float64)
    while len(a) > 1:
        a = a[0::2] + a[1::2]
    return a[0]


def step(src, tgt, D=None, d=0.1, chunk=512):
    """dict(nearest (n,) int32, e (n,) float32, sums (16,) float64, count, leaves (N, 16)) of one step"""
    D = IDENTITY if D is None else D
    t = cloud(tgt)
    pp, r, ok = image(src, D)
    n = len(r)
    d32 = np.float32(d)
    d2max = d32 * d32
    nearest, e = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32)
    rows = np.flatnonzero(ok)
    with np.errstate(all="ignore"):
        for at in range(0, len(rows) if len(t) else 0, chunk):
            i = rows[at:at + chunk]
            dx, dy, dz = (r[i, None, a] - t[None, :, a] for a in range(3))
            e2 = (dx * dx + dy * dy) + dz * dz
            j = np.argmin(e2, 1)
            best = e2[np.arange(len(i)), j]
            good = best <= d2max
            nearest[i[good]], e[i[good]] = j[good], best[good]
    c = reference_point(t)
    leaves = np.zeros((padded(max(n, 1)), 16), np.float64)
    has = np.flatnonzero(nearest >= 0)
    a, b = pp[has] - c, t[nearest[has]].astype(np.float64) - c
    leaves[has, 0:3], leaves[has, 3:6] = a, b
    for row in range(3):
        for col in range(3):
            leaves[has, 6 + 3 * row + col] = a[:, row] * b[:, col]
    leaves[has, 15] = e[has].astype(np.float64)
    return dict(nearest=nearest, e=e, sums=tree_sum(leaves), count=len(has), leaves=leaves)


def kabsch(sums, n, c):
    """the (16,) rigid matrix from the sums by an SVD with the determinant fix, in float64: independent of the Jacobi solve"""
    S = np.asarray(sums, np.float64)
    mua, mub = S[0:3] / n, S[3:6] / n
    H = S[6:15].reshape(3, 3) - np.outer(S[0:3], S[3:6]) / n
    U, _, Vt = np.linalg.svd(H)
    fix = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ fix @ U.T
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = (mub + c) - R @ (mua + c)
    return E.reshape(-1)


def float64_icp(recon, truth, transform, crop, stages):
    """the stages in float64 throughout: numpy's preparation, float64 distances, Kabsch; the (16,) matrix"""
    M = np.asarray(transform, np.float64).reshape(4, 4)
    for v, d, k in stages:
        src = P.prepare(recon, M.reshape(-1), crop, v)["xyz"].astype(np.float64)
        tgt = P.prepare(truth, None, crop, v)["xyz"].astype(np.float64)
        tgt = tgt[np.isfinite(tgt).all(1)]
        D, last = np.eye(4), None
        for s in range(1, k + 1):
            p = src @ D[:3, :3].T + D[:3, 3]
            j, e = np.zeros(len(p), np.int64), np.zeros(len(p))
            for at in range(0, len(p) if len(tgt) else 0, 2048):      # |p|^2 + |q|^2 - 2 p.q picks the target, its distance is then taken directly
                part = p[at:at + 2048]
                j[at:at + 2048] = np.argmin((part * part).sum(1)[:, None] + (tgt * tgt).sum(1)[None, :] - 2.0 * (part @ tgt.T), 1)
                e[at:at + 2048] = ((part - tgt[j[at:at + 2048]]) ** 2).sum(1)
            if not len(tgt):
                e[:] = np.inf
            has = e <= d * d
            n = int(has.sum())
            now = (n / max(len(p), 1), np.sqrt(e[has].sum() / n) if n else 0.0)
            if n < 3 or (last is not None and abs(now[0] - last[0]) < 1e-6 and abs(now[1] - last[1]) < 1e-6):
                break
            last = now
            a, b = p[has], tgt[j[has]]
            H = (a - a.mean(0)).T @ (b - b.mean(0))
            U, _, Vt = np.linalg.svd(H)
            R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
            E = np.eye(4)
            E[:3, :3], E[:3, 3] = R, b.mean(0) - R @ a.mean(0)
            D = E @ D
        M = D @ M
    return M.reshape(-1)


def motion_errors(M, known):
    """(rotation error in degrees, translation error) of a (16,) matrix against the known one"""
    A, B = np.asarray(M, np.float64).reshape(4, 4), np.asarray(known, np.float64).reshape(4, 4)
    R = A[:3, :3] @ B[:3, :3].T
    angle = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    return angle, float(np.linalg.norm(A[:3, 3] - B[:3, 3]))


# ---- the project's text on the host ---------------------------------------------------------------------------------------------
def build_program():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROGRAM)])


def run_program(*args):
    return subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def hexes(values):
    return [float(v).hex() for v in np.asarray(values, np.float64).reshape(-1)]


def serial_step(src, tgt, tmp, D=None, d=0.1, cells=None, search=None):
    """(return code, stderr, dict or None) of cloudicp_host step"""
    files = [os.path.join(str(tmp), n) for n in ("src.bin", "tgt.bin", "params.txt", "nearest.out", "e.out", "sums.out")]
    cloud(src).tofile(files[0])
    cloud(tgt).tofile(files[1])
    words = ["distance", float(np.float32(d)).hex()] + ([] if D is None else ["increment"] + hexes(D))
    words += ([] if cells is None else ["cells", str(cells)]) + ([] if search is None else ["search", search])
    with open(files[2], "w") as f:
        f.write(" ".join(words) + "\n")
    out = run_program("step", *files)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    return 0, out.stderr, dict(nearest=np.fromfile(files[3], np.int32), e=np.fromfile(files[4], np.float32), sums=np.fromfile(files[5], np.float64),
                               count=int(out.stdout.split()[1]))


def serial_refine(recon, truth, tmp, transform=None, crop=None, stages=(), cells=None):
    """(return code, stderr, dict(matrix (16,), log [(stage, step, n_src, n, rmse)]) or None) of cloudicp_host refine"""
    files = [os.path.join(str(tmp), n) for n in ("recon.bin", "truth.bin", "refine.txt", "matrix.out")]
    cloud(recon).tofile(files[0])
    cloud(truth).tofile(files[1])
    words = [] if transform is None else ["transform"] + hexes(transform)
    if crop is not None:
        poly = np.asarray(crop["polygon"], np.float64).reshape(-1)
        words += ["crop", str(int(crop["axis"])), float(crop["axis_min"]).hex(), float(crop["axis_max"]).hex(), str(len(poly) // 3)] + hexes(poly)
    for v, d, k in stages:
        words += ["stage", float(v).hex(), float(d).hex(), str(int(k))]
    words += [] if cells is None else ["cells", str(cells)]
    with open(files[2], "w") as f:
        f.write(" ".join(words) + "\n")
    out = run_program("refine", *files)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    log = [(int(w[1]), int(w[2]), int(w[3]), int(w[4]), float.fromhex(w[5])) for w in (line.split() for line in out.stdout.splitlines()) if w and w[0] == "log"]
    return 0, out.stderr, dict(matrix=np.fromfile(files[3], np.float64), log=log)


def serial_solve(sums, n, c):
    out = run_program("solve", int(n), *(hexes(sums) + hexes(c)))
    assert out.returncode == 0, out.stderr
    return np.array([float.fromhex(w) for w in out.stdout.split()], np.float64)


def same_step(got, want):
    """"" or what differs between two steps (e and sums bit for bit; nearest and count exactly)"""
    if got["count"] != want["count"]:
        return "count: %d, expected %d" % (got["count"], want["count"])
    if not np.array_equal(got["nearest"], want["nearest"]):
        bad = np.flatnonzero(got["nearest"] != want["nearest"])
        return "nearest differs at %s: %s, expected %s" % (list(bad[:5]), got["nearest"][bad[:5]].tolist(), want["nearest"][bad[:5]].tolist())
    if got["e"].tobytes() != want["e"].tobytes():
        return "e differs"
    if np.asarray(got["sums"], np.float64).tobytes() != np.asarray(want["sums"], np.float64).tobytes():
        return "sums differ: %s, expected %s" % (hexes(got["sums"]), hexes(want["sums"]))
    return ""


# ---- the case table: name -> dict(src, tgt, D, d) ----------------------------------------------------------------------------------
def case(src, tgt, D=None, d=0.1):
    return dict(src=cloud(src), tgt=cloud(tgt), D=None if D is None else np.asarray(D, np.float64).reshape(-1), d=float(np.float32(d)))


def near(tgt, n, pattern, rng, d=0.1):
    """n sources of which all, none or every other one lie within d / 4 of some target"""
    tgt = cloud(tgt)
    src = tgt[rng.integers(0, len(tgt), n)].astype(np.float64) + (rng.random((n, 3)) - 0.5) * (d / 4)
    if pattern == "none":
        src += 50.0
    if pattern == "alternate":
        src[1::2] += 50.0
    return src


def cell_edge(d, R):
    return float(np.float32(d)) * (1.0 + 1.0 / 1024.0) / R


def every_cell(R, d=0.1):
    """one (source, target) pair per cell of the (2R + 1)^3 neighbourhood: target 0 at the origin is the minimum, so the grid's origin is
    -(2R + 1) h and cell t covers [origin + t h, origin + (t + 1) h); the pairs are 8 cells apart"""
    h = cell_edge(d, R)
    origin = -(2 * R + 1) * h
    frac = {0: 0.5, 1: 0.95, 2: 0.95, -1: 0.05, -2: 0.05}
    move = {0: 0.0, 1: 0.5, 2: 1.1, -1: -0.5, -2: -1.1}
    src, tgt, offsets = [], [[0.0, 0.0, 0.0]], []
    W = 2 * R + 1
    for n in range(W ** 3):
        o = (n // (W * W) - R, (n // W) % W - R, n % W - R)
        base = [20 + 8 * (o[a] + R) for a in range(3)]
        s = [origin + (base[a] + frac[o[a]]) * h for a in range(3)]
        src.append(s)
        tgt.append([s[a] + move[o[a]] * h for a in range(3)])
        offsets.append(o)
    return case(src, tgt, None, d), offsets


def cell_offsets(c, R):
    """the cell offset (target - source) of every corresponding source under the grid of radius R, from the definition"""
    res = step(c["src"], c["tgt"], c["D"], c["d"])
    h = cell_edge(c["d"], R)
    origin = c["tgt"].min(0).astype(np.float64) - (2 * R + 1) * h
    _, r, _ = image(c["src"], IDENTITY if c["D"] is None else c["D"])
    has = res["nearest"] >= 0
    cs = np.floor((r[has].astype(np.float64) - origin) / h)
    ct = np.floor((c["tgt"][res["nearest"][has]].astype(np.float64) - origin) / h)
    return {tuple(int(v) for v in row) for row in (ct - cs)}


def cases():
    rng = np.random.default_rng(23)
    c = {}
    base = rng.random((200, 3))
    # the wave, work-group and second-level seams of the tree; all, none and alternate sources corresponding
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        for pattern in ("all", "none", "alternate"):
            c["tree_%s_%d" % (pattern, n)] = case(near(base, n, pattern, rng), base)
    c["tree_second_level_seam"] = case(near(base[:5], 256 * 1024 + 300, "alternate", rng), base[:5])
    two = near(base, 10, "none", rng)
    two[[3, 8]] -= 50.0
    c["exactly_two"] = case(two, base)
    c["no_target"] = case(base[:70], np.zeros((0, 3)))
    c["one_target"] = case(base[:70], base[:1], d=0.5)
    # ties: duplicates, and two targets at equal distance in different cells; the smallest index wins
    dup = np.concatenate([base[:50], base[20:30], base[:50]])
    c["duplicate_targets"] = case(near(base[:50], 130, "all", rng), dup)
    c["equidistant_other_cells"] = case([[1, 1, 1], [3, 1, 1]], [[0, 0, 0], [1.09375, 1, 1], [0.90625, 1, 1], [2.90625, 1, 1], [3.09375, 1, 1]], d=0.125)
    cluster = 2.0 + 0.004 * rng.random((64, 3))
    many = np.concatenate([cluster, cluster, cluster[:1]])      # 129 targets in one cell, k and k + 64 the same point: two chunks of 64 records
    c["equidistant_other_chunks"] = case(near(cluster, 100, "all", rng, 0.002), many)
    # the distance itself
    c["target_at_d"] = case([[0, 0, 0]], [[0.125, 0, 0]], d=0.125)
    c["target_ulp_beyond_d"] = case([[0, 0, 0]], [[float(np.nextafter(np.float32(0.125), np.float32(1))), 0, 0]], d=0.125)
    c["target_at_d_tenth"] = case([[0, 0, 0]], [[0, float(np.float32(0.1)), 0]], d=0.1)
    c["target_ulp_beyond_d_tenth"] = case([[0, 0, 0]], [[0, float(np.nextafter(np.float32(0.1), np.float32(1))), 0]], d=0.1)
    c["every_cell_27"], _ = every_cell(1)
    c["every_cell_125"], _ = every_cell(2)
    for n in (63, 64, 65, 129):
        one = 3.0 + 0.01 * rng.random((n, 3))
        c["one_cell_%d" % n] = case(near(one, 150, "alternate", rng, 0.02), one)
    bad = near(base, 200, "all", rng)
    for k, i in enumerate((0, 63, 64, 127, 128, 199)):
        bad[i, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    c["non_finite_sources"] = case(bad, base)
    over = np.eye(4)
    over[0, 0] = 1e38
    flat = near(base, 70, "all", rng)
    flat[:, 0] = 0.0
    flat[33, 0] = 10.0
    flat_tgt = base.copy()
    flat_tgt[:, 0] = 0.0
    c["image_overflows_binary32"] = case(flat, flat_tgt, over)
    far = 1e4 + 0.2 * rng.random((3000, 3))
    c["near_1e4"] = case(far[:2000] + rng.normal(0, 0.003, (2000, 3)), far, d=0.01)
    neg = -5 + 2 * rng.random((2000, 3))
    c["negative_coordinates"] = case(neg[:1500] + rng.normal(0, 0.02, (1500, 3)), neg)
    shift = np.eye(4)
    shift[:3, 3] = [1000.0, -2000.0, 500.0]
    c["large_translation"] = case(near(base, 300, "alternate", rng) - shift[:3, 3], base, shift)
    turn = P.rotation(25.0, -10.0, [0.3, -0.2, 0.1]).reshape(4, 4)
    moved = (np.linalg.inv(turn) @ np.concatenate([near(base, 300, "all", rng), np.ones((300, 1))], 1).T).T[:, :3]
    c["rotation"] = case(moved, base, turn)
    # a = +0 and b < 0: every product is -0.0, which only a tree that stops at N keeps
    c["negative_zero_2"] = case([[0, 0, 0]] * 2, [[-1, -1, -1], [1, 1, 1]], d=2.0)
    c["negative_zero_3"] = case([[0, 0, 0]] * 3, [[-1, -1, -1], [1, 1, 1]], d=2.0)
    c["random_3000"] = case(rng.random((3000, 3)), rng.random((3000, 3)), d=0.05)
    return c


# ---- `apd --evaluate`'s report without a refinement, restated ------------------------------------------------------------------------
def report_text(recon, truth, num, used, within_recon, within_truth, tolerances, counts=None):
    """the report's bytes from the counts of the existing entries: the two cloud lines (skipped = every point dropped for a non-finite
    coordinate, as read, after the transform or after the rounding of a prepared point), with counts (2, 4) the two `prepared` lines,
    then one line per tolerance with the figures as percentages"""
    c = None if counts is None else np.asarray(counts, np.int64).reshape(2, 4)
    skipped = [int(num[k] - used[k]) if c is None else int((num[k] - c[k, 1]) + (c[k, 3] - used[k])) for k in range(2)]
    text = "reconstruction %s %d points (%d skipped)\nground_truth %s %d points (%d skipped)\n" % (recon, used[0], skipped[0], truth, used[1], skipped[1])
    for k in range(2 if c is not None else 0):
        text += "prepared %s: %d finite, %d in the crop volume, %d points\n" % (("reconstruction", "ground_truth")[k], c[k, 0], c[k, 2], c[k, 3])
    text += "tolerance accuracy completeness f1\n"
    for k, t in enumerate(tolerances):
        a = int(within_recon[k]) / int(used[0]) if used[0] else 0.0
        b = int(within_truth[k]) / int(used[1]) if used[1] else 0.0
        f = 0.0 if a + b == 0.0 else 2.0 * a * b / (a + b)
        text += "%.9g %.6f %.6f %.6f\n" % (float(np.float32(t)), 100.0 * a, 100.0 * b, 100.0 * f)
    return text


# ---- the scene of the refinement tests-----------------------------------------------------------------------------------------------
STAGES = [(0.04, 0.4, 20), (0.02, 0.1, 20), (0.02, 0.03, 20)]      # the protocol's three stages at tau = 0.005, scaled to this scene


def refine_scene(seed=41, n=6000):
    """(recon, truth, known (16,), initial (16,), crop): 6000 truth points, a noisy subset moved by the inverse of a known matrix, and
    that matrix perturbed by a few degrees and a few centimetres"""
    rng = np.random.default_rng(seed)
    truth = cloud(rng.random((n, 3)) * [1.4, 1.4, 1.0] - [0.2, 0.2, 0.0])
    moved = truth[: n - 500] + rng.normal(0, 0.003, (n - 500, 3)).astype(np.float32)
    known = P.rotation(30.0, 10.0, [0.1, -0.05, 0.02]).reshape(4, 4)
    recon = cloud((np.linalg.inv(known) @ np.concatenate([moved.astype(np.float64), np.ones((len(moved), 1))], 1).T).T[:, :3])
    recon[7, 1] = np.nan
    truth[11, 0] = np.inf
    wrong = P.rotation(2.0, -1.5, [0.02, -0.015, 0.01]).reshape(4, 4)
    crop = P.crop_of(2, 0.1, 0.8, P.polygon_3d(2, P.CONCAVE_12))
    return recon, truth, known.reshape(-1), (wrong @ known).reshape(-1), crop
