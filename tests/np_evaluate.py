"""TEST INFRASTRUCTURE: the definition behind `apd --evaluate` (csrc/dvp_cloudeval.hpp) restated in numpy - blocked brute force in
np.float32 with the header's operation order, and the counts -, the grid's cell keys and home slots in numpy's binary64 / uint64, the
case table that the host and the device tests share, the runner of tests/cloudeval_host, and PLY writers."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "cloudeval_host", "cloudeval_host")
DEFAULT_TOLERANCES = [0.01, 0.02, 0.05, 0.1, 0.2, 0.5]
F = np.float32


def cloud(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


# ---- the definition -----------------------------------------------------------------------------------------------------------
def brute_d2(query, target, T, block=512):
    """d2 of every query: min over the finite targets of (dx*dx + dy*dy) + dz*dz in binary32, +inf above T*T, NaN for a non-finite query"""
    q, t = cloud(query), cloud(target)
    t = t[np.isfinite(t).all(1)]
    T2 = F(T) * F(T)
    out = np.full(len(q), np.inf, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for first in range(0, len(q), block):
            p = q[first:first + block]
            if len(t):
                dx, dy, dz = (p[:, None, a] - t[None, :, a] for a in range(3))
                m = ((dx * dx + dy * dy) + dz * dz).min(1)
                assert m.dtype == np.float32
                out[first:first + block] = np.where(m <= T2, m, F(np.inf))
    out[~np.isfinite(q).all(1)] = np.nan
    return out


def counts(d2, tolerances):
    """(within (K,), used) of one direction"""
    ok = ~np.isnan(d2)
    return np.array([int((d2[ok] <= F(t) * F(t)).sum()) for t in tolerances], np.int64), int(ok.sum())


def evaluate(recon, truth, tolerances):
    T = tolerances[-1]
    a, c = brute_d2(recon, truth, T), brute_d2(truth, recon, T)
    (wr, ur), (wt, ut) = counts(a, tolerances), counts(c, tolerances)
    return dict(d2_recon=a, d2_truth=c, within_recon=wr, within_truth=wt, used=np.array([ur, ut], np.int64))


# ---- the grid and the table ---------------------------------------------------------------------------------------------------
def grid_of(recon, truth, T):
    pts = np.concatenate([cloud(recon), cloud(truth)])
    pts = pts[np.isfinite(pts).all(1)]
    return pts.min(0).astype(np.float64), float(F(T)) * (1.0 + 2.0 ** -10)


def cell_indices(points, origin, h):
    """(N, 3) int64 cell indices as stored (+ 1)"""
    return np.floor((cloud(points).astype(np.float64) - origin) / h).astype(np.int64) + 1


def cell_keys(points, origin, h):
    c = cell_indices(points, origin, h).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def hash_keys(keys):
    k = keys.astype(np.uint64)
    with np.errstate(over="ignore"):
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return k ^ (k >> np.uint64(31))


def table_capacity(points):
    cap = 64
    while cap < 2 * points:
        cap *= 2
    return cap


# ---- the project's text on the host -------------------------------------------------------------------------------------------
def build_program():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROGRAM)])


def run_program(*args):
    return subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def tolerance_text(tolerances):
    return ",".join("%.9g" % float(F(t)) for t in tolerances)


def serial(recon, truth, tolerances, tmp, mode="grid"):
    """(return code, stderr, dict or None) of cloudeval_host evaluate"""
    r, t = cloud(recon), cloud(truth)
    files = [os.path.join(str(tmp), n) for n in ("recon.bin", "truth.bin", "d2.out")]
    r.tofile(files[0])
    t.tofile(files[1])
    out = run_program("evaluate", files[0], files[1], tolerance_text(tolerances), mode, files[2])
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    lines = dict((ln.split()[0], [int(v) for v in ln.split()[1:]]) for ln in out.stdout.splitlines())
    d2 = np.fromfile(files[2], np.float32)
    return 0, out.stderr, dict(d2_recon=d2[:len(r)], d2_truth=d2[len(r):], within_recon=np.array(lines["within_recon"], np.int64),
                               within_truth=np.array(lines["within_truth"], np.int64), used=np.array(lines["used"], np.int64))


def serial_distances(query, target, T, tmp, mode="grid"):
    """(return code, stderr, d2 of every query or None) of cloudeval_host distances"""
    files = [os.path.join(str(tmp), n) for n in ("query.bin", "target.bin", "d2_query.out")]
    cloud(query).tofile(files[0])
    cloud(target).tofile(files[1])
    out = run_program("distances", files[0], files[1], "%.9g" % float(F(T)), mode, files[2])
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    return 0, out.stderr, np.fromfile(files[2], np.float32)


def home_slot(recon, truth, T, point, tmp):
    """(capacity, home slot, key) of the cell of `point`, as the host tool has them"""
    files = [os.path.join(str(tmp), n) for n in ("slot_recon.bin", "slot_truth.bin")]
    cloud(recon).tofile(files[0])
    cloud(truth).tofile(files[1])
    out = run_program("slot", files[0], files[1], "%.9g" % float(F(T)), *["%.9g" % float(v) for v in point])
    assert out.returncode == 0, out.stderr
    return tuple(int(v) for v in out.stdout.split())


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_result(got, want):
    """"" or what differs between two results (d2 bit for bit, NaN == NaN; the counts exactly)"""
    for k in ("d2_recon", "d2_truth"):
        if k in got and not same_bits(got[k], want[k]):
            bad = np.flatnonzero(~((got[k].view(np.uint32) == want[k].view(np.uint32)) | (np.isnan(got[k]) & np.isnan(want[k])))) if got[k].shape == want[k].shape else []
            return "%s differs at %s" % (k, list(bad[:5]))
    for k in ("within_recon", "within_truth", "used"):
        if not np.array_equal(got[k], want[k]):
            return "%s: %s, expected %s" % (k, list(got[k]), list(want[k]))
    return ""


# ---- the case table: name -> (recon, truth, tolerances) -------------------------------------------------------------------------
H1 = 1.0 + 2.0 ** -10   # the cell edge at T = 1


def corner_scene():
    """T = 1.  26 sub-scenes four cells apart along x: a query near the face, edge or corner of its cell towards neighbour (i, j, k),
    its nearest target just across in that neighbour, a farther target in the query's own cell.  Anchors fix the origin at 0."""
    q, t = [], [[0.0, 0.0, 0.0], [120 * H1, 10 * H1, 10 * H1]]
    n = 0
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            for k in (-1, 0, 1):
                if (i, j, k) == (0, 0, 0):
                    continue
                d = np.array([i, j, k], np.float64)
                centre = np.array([(4 * n + 5.5) * H1, 5.5 * H1, 5.5 * H1])
                q.append(centre + 0.49 * H1 * d)
                t.append(centre + 0.52 * H1 * d)      # the nearest: in the neighbour cell
                t.append(centre + 0.25 * H1 * d)      # farther, in the query's cell
                n += 1
    return cloud(q), cloud(t), [0.1, 1.0]


def one_cell(n_query, n_target, seed):
    """T = 0.5: all targets in one cell, all queries in one cell (the same one)"""
    rng = np.random.default_rng(seed)
    anchor = [[0.0, 0.0, 0.0]]
    q = 2.6 + 0.3 * rng.random((n_query, 3))
    t = 2.6 + 0.3 * rng.random((n_target, 3))
    return cloud(np.concatenate([q, anchor])), cloud(np.concatenate([t, anchor])), [0.05, 0.2, 0.5]


def table_scene(seed=5):
    """T = 1, 8192 points in all, so the table has its smallest capacity for them (16384): 6000 recon points in cells of their own,
    2192 truth points next to some of them"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(40 * 40 * 40)[:6000]
    base = np.stack([cells // 1600, (cells // 40) % 40, cells % 40], 1).astype(np.float64)
    recon = (base + 0.2 + 0.6 * rng.random((6000, 3))) * H1
    truth = recon[:2192] + rng.normal(0, 0.05, (2192, 3))
    recon[0] = 0.0       # the origin
    return cloud(recon), cloud(truth), [0.05, 0.1, 1.0]


def cases():
    rng = np.random.default_rng(11)
    one = np.float32(0.5)
    beyond = np.nextafter(one, np.float32(1))
    c = {}
    c["one_one"] = (cloud([[0.1, 0.2, 0.3]]), cloud([[0.15, 0.2, 0.3]]), [0.1])
    same = cloud(rng.random((10, 3)))
    c["same"] = (same, same.copy(), [0.01, 0.5])
    c["no_queries"] = (cloud([]), cloud(rng.random((5, 3))), [0.1, 0.5])
    c["no_targets"] = (cloud(rng.random((5, 3))), cloud([]), [0.1, 0.5])
    c["both_empty"] = (cloud([]), cloud([]), [0.5])
    c["at_T"] = (cloud([[0, 0, 0], [3, 3, 3]]), cloud([[one, 0, 0], [3, 3 + one, 3]]), [0.25, 0.5])
    c["beyond_T"] = (cloud([[0, 0, 0], [3, 3, 0]]), cloud([[beyond, 0, 0], [3, 3, beyond]]), [0.25, 0.5])
    c["two_cells_away"] = (cloud([[0, 0, 0], [5, 5, 5]]), cloud([[1.1, 0, 0], [5, 5, 6.05]]), [0.5])
    for n in (63, 64, 65, 129):
        c["targets_%d" % n] = one_cell(3, n, n)
        c["queries_%d" % n] = one_cell(n, 5, 1000 + n)
    c["corners"] = corner_scene()
    c["table"] = table_scene()
    c["identical_targets"] = (cloud(1.0 + 0.2 * rng.random((70, 3))), cloud(np.tile([[1.1, 1.05, 1.0]], (200, 1))), [0.05, 0.1, 0.5])
    c["negative"] = (cloud(-5 + 2 * rng.random((300, 3))), cloud(-5 + 2 * rng.random((280, 3))), [0.1, 0.3])
    c["near_1e4"] = (cloud(1e4 + 0.5 * rng.random((300, 3))), cloud(1e4 + 0.5 * rng.random((310, 3))), [0.002, 0.005, 0.01])
    bad_r, bad_t = rng.random((40, 3)), rng.random((45, 3))
    bad_r[3, 0], bad_r[7, 1], bad_r[11, 2] = np.nan, np.inf, -np.inf
    bad_t[0, 2], bad_t[9, 0], bad_t[44, 1] = np.nan, np.inf, -np.inf
    c["non_finite"] = (cloud(bad_r), cloud(bad_t), [0.1, 0.2, 0.5])
    c["only_non_finite_targets"] = (cloud(rng.random((6, 3))), cloud([[np.nan, 0, 0], [0, np.inf, 0]]), [0.5])
    c["ragged_1000_777"] = (cloud(rng.random((1000, 3))), cloud(rng.random((777, 3))), [0.02, 0.05, 0.1])
    c["ragged_257_65"] = (cloud(rng.random((257, 3))), cloud(rng.random((65, 3))), [0.05, 0.1, 0.2, 0.4])
    c["eight_tolerances"] = (cloud(rng.random((130, 3))), cloud(rng.random((140, 3))), [0.01, 0.02, 0.04, 0.08, 0.12, 0.16, 0.2, 0.3])
    return c


def contention_scene(seed=9):
    """T = 0.05: 20 000 targets and 5 000 queries inside a 3 x 3 x 3 block of cells"""
    rng = np.random.default_rng(seed)
    h = float(F(0.05)) * (1.0 + 2.0 ** -10)
    return cloud(rng.random((5000, 3)) * 2.99 * h), cloud(rng.random((20000, 3)) * 2.99 * h), [0.002, 0.01, 0.05]


def random_scene(seed, n=4000):
    rng = np.random.default_rng(seed)
    return cloud(rng.random((n, 3))), cloud(rng.random((n, 3))), DEFAULT_TOLERANCES


# ---- PLY files ----------------------------------------------------------------------------------------------------------------
def write_ply_like_apd(path, xyz, bgr=None):
    """the bytes of ExportPointCloud (host/io.cpp)"""
    xyz = cloud(xyz)
    rec = np.zeros(len(xyz), np.dtype([("xyz", "<f4", 3), ("bgr", "u1", 3)]))
    rec["xyz"] = xyz
    if bgr is not None:
        rec["bgr"] = bgr
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(xyz)
    head += "property uchar diffuse_blue\nproperty uchar diffuse_green\nproperty uchar diffuse_red\nend_header\n"
    with open(path, "wb") as f:
        f.write(head.encode() + rec.tobytes())


def read_ply(path, tmp):
    """(return code, stderr, (N, 3) float32 or None) of cloudeval_host ply"""
    dst = os.path.join(str(tmp), "ply.out")
    out = run_program("ply", path, dst)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    return 0, out.stderr, np.fromfile(dst, np.float32).reshape(-1, 3)
