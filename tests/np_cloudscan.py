"""TEST INFRASTRUCTURE: the observed-space accuracy of `apd --evaluate --against-scans` (csrc/dvp_cloudscan.hpp) read independently in
numpy, binary32 step by step - the truth points, texel_of, the range maps with np.minimum.at, the gaps, the counts -, the case table
and the room scene that the host and the device tests share, the writers of a MeshLab project and its scans, the report restated, and
the runner of tests/cloudscan_host."""
import os
import subprocess

import numpy as np

import np_cloudprep as P
import np_evaluate as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "cloudscan_host", "cloudscan_host")
F = np.float32
IDENTITY = np.eye(4).reshape(-1)

cloud = P.cloud


def matrix(m):
    return np.asarray(m, np.float64).reshape(-1)


def scan(xyz, m=None):
    return (cloud(xyz), IDENTITY.copy() if m is None else matrix(m))


def moved_to(o):
    """the matrix of a scanner that stands at o and is not turned"""
    m = np.eye(4)
    m[:3, 3] = o
    return m.reshape(-1)


# ---- the definition -------------------------------------------------------------------------------------------------------------
def truth_points(xyz, m):
    """g = M q in binary64 by the preparation's formula, rounded once to binary32, whatever q holds"""
    p = cloud(xyz).astype(np.float64)
    m = matrix(m).reshape(4, 4)
    with np.errstate(all="ignore"):
        g = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], 1)
        return g.astype(np.float32).reshape(-1, 3)


def scanner(m):
    return matrix(m)[[3, 7, 11]].astype(np.float32)


def truth_cloud(scans):
    return np.concatenate([truth_points(x, m) for x, m in scans] + [np.zeros((0, 3), np.float32)])


def texel_of(x, o, R):
    """(t (n,) int64, r2 (n,) float32, ok (n,) bool): texel and squared range of every point seen from o; ok = not void"""
    x = cloud(x)
    with np.errstate(all="ignore"):
        d = x - np.asarray(o, np.float32)[None, :]
        assert d.dtype == np.float32
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = np.isfinite(d).all(1) & np.isfinite(r2) & (r2 != 0)
        ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
        a = np.where((ax >= ay) & (ax >= az), 0, np.where(ay >= az, 1, 2))
        da = np.where(a == 0, d[:, 0], np.where(a == 1, d[:, 1], d[:, 2]))
        du = np.where(a == 0, d[:, 1], d[:, 0])
        dv = np.where(a == 2, d[:, 1], d[:, 2])
        f = 2 * a + (da < 0)
        m = np.where(ok, np.abs(da), F(1))
        half = F(0.5) * F(R)
        idx = []
        for s in (du, dv):
            su = np.where(ok, s, F(0)) / m
            assert su.dtype == np.float32
            idx.append(np.minimum(R - 1, np.floor((su + F(1)) * half).astype(np.int64)))
    t = (f.astype(np.int64) * R + idx[1]) * R + idx[0]
    return np.where(ok, t, 0), r2, ok


def maps(scans, R):
    """(S, 6 R R) float32: the smallest r2 per texel, +inf where no return fell"""
    out = np.full((len(scans), 6 * R * R), np.inf, np.float32)
    for s, (x, m) in enumerate(scans):
        t, r2, ok = texel_of(truth_points(x, m), scanner(m), R)
        np.minimum.at(out[s], t[ok], r2[ok])
    return out


def gaps(queries, scans, R, made=None):
    """(n,) float32: NaN for a non-finite query, -inf where no scan observes the query's direction"""
    q = cloud(queries)
    made = maps(scans, R) if made is None else made
    best = np.full(len(q), -np.inf, np.float32)
    for s, (x, m) in enumerate(scans):
        t, r2, ok = texel_of(q, scanner(m), R)
        behind = made[s][t]
        with np.errstate(all="ignore"):
            g = np.sqrt(behind) - np.sqrt(r2)
            assert g.dtype == np.float32
        seen = ok & np.isfinite(behind)
        best = np.where(seen & (g > best), g, best)
    best[~np.isfinite(q).all(1)] = np.nan
    return best


def free_space(d2, gap, tolerances):
    with np.errstate(invalid="ignore"):
        return np.array([int((~(d2 <= F(t) * F(t)) & (gap > F(t))).sum()) for t in tolerances], np.int64)


def evaluate(recon, scans, tolerances, R, prep_recon=None, prep_truth=None, d2=None):
    """the whole evaluation; d2 (of the prepared reconstruction) may be given where the brute force would take too long - the
    distances are then not restated, and within_truth is left out"""
    truth = truth_cloud(scans)
    r = P.prepare(recon, **(prep_recon or {}))
    t = P.prepare(truth, **(prep_truth or {}))
    out = dict(recon=r["xyz"], truth=t["xyz"], counts=np.stack([r["counts"], t["counts"]]))
    if d2 is None:
        e = N.evaluate(r["xyz"], t["xyz"], tolerances)
        d2 = e["d2_recon"]
        out.update(within_truth=e["within_truth"], used=e["used"])
    else:
        out.update(used=np.array([int(np.isfinite(r["xyz"]).all(1).sum()), int(np.isfinite(t["xyz"]).all(1).sum())], np.int64))
    out.update(d2_recon=d2, within_recon=N.counts(d2, tolerances)[0], gap=gaps(r["xyz"], scans, R))
    out["free_space"] = free_space(d2, out["gap"], tolerances)
    out["unobserved"] = out["used"][0] - out["within_recon"] - out["free_space"]
    return out


# ---- the project's text on the host ---------------------------------------------------------------------------------------------
def build_program():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROGRAM)])


def run_program(*args):
    return subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def write_scan_list(scans, tmp):
    """scans.txt of the test tool; a scan may carry a count of its own as a third item"""
    path = os.path.join(str(tmp), "scans.txt")
    with open(path, "w") as f:
        for k, s in enumerate(scans):
            name = os.path.join(str(tmp), "scan%d.bin" % k)
            cloud(s[0]).tofile(name)
            f.write(" ".join([name] + [float(v).hex() for v in matrix(s[1])] + ([str(int(s[2]))] if len(s) > 2 else [])) + "\n")
    return path


def serial_gaps(scans, queries, R, tmp):
    """(return code, stderr, dict(gap, maps (S, 6 R R), truth) or None) of cloudscan_host gaps"""
    files = [os.path.join(str(tmp), n) for n in ("query.bin", "gap.out", "maps.out", "truth.out")]
    cloud(queries).tofile(files[0])
    out = run_program("gaps", write_scan_list(scans, tmp), R, *files)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    return 0, out.stderr, dict(gap=np.fromfile(files[1], np.float32), maps=np.fromfile(files[2], np.float32).reshape(len(scans), -1),
                               truth=np.fromfile(files[3], np.float32).reshape(-1, 3))


def serial_evaluate(recon, scans, tolerances, R, tmp, prep_recon=None, prep_truth=None):
    """(return code, stderr, dict or None) of cloudscan_host evaluate"""
    d = str(tmp)
    files = [os.path.join(d, n) for n in ("recon.bin", "tolerances.txt", "prep_recon.txt", "prep_truth.txt", "d2.out", "gap.out", "recon.out", "truth.out")]
    cloud(recon).tofile(files[0])
    with open(files[1], "w") as f:
        f.write(" ".join(float(F(t)).hex() for t in tolerances) + "\n")
    for path, prep in ((files[2], prep_recon), (files[3], prep_truth)):
        with open(path, "w") as f:
            f.write("none\n" if prep is None else P.prep_text(**prep))
    out = run_program("evaluate", files[0], write_scan_list(scans, tmp), R, *files[1:])
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    rows = {w[0]: np.array([int(v) for v in w[1:]], np.int64) for w in (line.split() for line in out.stdout.splitlines()) if w}
    rows.update(d2_recon=np.fromfile(files[4], np.float32), gap=np.fromfile(files[5], np.float32), recon=np.fromfile(files[6], np.float32).reshape(-1, 3),
                truth=np.fromfile(files[7], np.float32).reshape(-1, 3))
    rows["counts"] = rows["counts"].reshape(2, 4)
    return 0, out.stderr, rows


def same_gaps(got, want):
    """"" or what differs (gap, maps and truth bit for bit, NaN == NaN)"""
    for name in ("truth", "maps", "gap"):
        a, b = np.ascontiguousarray(got[name], np.float32), np.ascontiguousarray(want[name], np.float32)
        if a.shape != b.shape:
            return "%s: shape %s, expected %s" % (name, a.shape, b.shape)
        bad = np.flatnonzero(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).reshape(-1))
        if len(bad):
            return "%s differs at %s: %s, expected %s" % (name, bad[:5].tolist(), a.reshape(-1)[bad[:5]].tolist(), b.reshape(-1)[bad[:5]].tolist())
    return ""


def same_evaluation(got, want, distances=True):
    """"" or what differs between two evaluations (counts exactly; d2, gap and the prepared clouds bit for bit)"""
    for name in ("within_recon", "within_truth", "used", "free_space", "counts"):
        if name in want and not np.array_equal(np.asarray(got[name]).reshape(-1), np.asarray(want[name]).reshape(-1)):
            return "%s: %s, expected %s" % (name, np.asarray(got[name]).tolist(), np.asarray(want[name]).tolist())
    for name in (("d2_recon", "gap", "recon", "truth") if distances else ()):
        if name in got and name in want and not N.same_bits(got[name], want[name]):
            return "%s differs" % name
    return ""


# ---- a MeshLab project and its scans ------------------------------------------------------------------------------------------------
def mlp_text(names, matrices):
    """the bytes MeshLab writes for a project of meshes with their matrices"""
    text = "<!DOCTYPE MeshLabDocument>\n<MeshLabProject>\n <MeshGroup>\n"
    for name, m in zip(names, matrices):
        rows = "".join(" ".join(repr(float(v)) for v in row) + " \n" for row in matrix(m).reshape(4, 4))
        text += '  <MLMesh label="%s" filename="%s">\n   <MLMatrix44>\n%s</MLMatrix44>\n  </MLMesh>\n' % (name, name, rows)
    return text + " </MeshGroup>\n <RasterGroup/>\n</MeshLabProject>\n"


def write_mlp(path, names, matrices):
    with open(path, "w") as f:
        f.write(mlp_text(names, matrices))


def write_scans(folder, scans, name="scan_alignment.mlp"):
    """the scans as scan<k>.ply beside the project; returns the project's path and the names"""
    names = ["scan%d.ply" % (k + 1) for k in range(len(scans))]
    for n, (x, m) in zip(names, scans):
        N.write_ply_like_apd(os.path.join(str(folder), n), x)
    write_mlp(os.path.join(str(folder), name), names, [m for _, m in scans])
    return os.path.join(str(folder), name), names


def report_text(recon, project, names, scans, res, tolerances, num_recon, prepares=False):
    """the report's bytes of `apd --evaluate --against-scans` from an evaluation's counts"""
    used, c = res["used"], np.asarray(res["counts"], np.int64).reshape(2, 4)
    num = [num_recon, sum(len(x) for x, _ in scans)]
    skipped = [int((num[k] - c[k, 1]) + (c[k, 3] - used[k])) if prepares else int(num[k] - used[k]) for k in range(2)]
    text = "reconstruction %s %d points (%d skipped)\nground_truth %s %d points (%d skipped)\n" % (recon, used[0], skipped[0], project, used[1], skipped[1])
    for n, (x, m) in zip(names, scans):
        text += "scan %s: %d points, scanner at %s\n" % (n, len(x), " ".join("%.9g" % float(v) for v in scanner(m)))
    for k in range(2 if prepares else 0):
        text += "prepared %s: %d finite, %d in the crop volume, %d points\n" % (("reconstruction", "ground_truth")[k], c[k, 0], c[k, 2], c[k, 3])
    text += "tolerance accuracy completeness f1\n"
    for k, t in enumerate(tolerances):
        judged = int(res["within_recon"][k]) + int(res["free_space"][k])
        a = int(res["within_recon"][k]) / judged if judged else 0.0
        b = int(res["within_truth"][k]) / int(used[1]) if used[1] else 0.0
        f = 0.0 if a + b == 0.0 else 2.0 * a * b / (a + b)
        text += "%.9g %.6f %.6f %.6f\n" % (float(F(t)), 100.0 * a, 100.0 * b, 100.0 * f)
    text += "tolerance accurate free_space unobserved\n"
    for k, t in enumerate(tolerances):
        text += "%.9g %d %d %d\n" % (float(F(t)), res["within_recon"][k], res["free_space"][k], used[0] - res["within_recon"][k] - res["free_space"][k])
    return text


# ---- the case table: name -> dict(scans, queries, R) -------------------------------------------------------------------------------
def case(scans, queries, R=16):
    """a scan is an array of points (the identity) or a tuple (points, matrix)"""
    return dict(scans=[scan(*s) if isinstance(s, tuple) else scan(s) for s in scans], queries=cloud(queries), R=R)


def directions():
    """the 6 axes, the 12 face diagonals and the 8 corners"""
    out = []
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            for z in (-1, 0, 1):
                if (x, y, z) != (0, 0, 0):
                    out.append((x, y, z))
    return np.array(out, np.float64)


def cases():
    rng = np.random.default_rng(31)
    c = {}
    c["one_point"] = case([[[1, 0, 0]]], [[0.5, 0, 0], [2, 0, 0], [0, 1, 0]])
    c["empty_scan"] = case([np.zeros((0, 3))], [[0.5, 0, 0], [0, 0, 0], [np.nan, 0, 0]])
    ray = np.array([1.0, 0.01, 0.01])
    for n in (63, 64, 65, 129):      # one texel: the atomic under contention, the ragged last wave; as many queries
        c["one_texel_%d" % n] = case([ray[None, :] * (1.0 + 2.0 * rng.random((n, 1)))], ray[None, :] * (0.5 + 3.0 * rng.random((n, 1))))
    dirs = directions()
    for R in (16, 64, 1024):
        # the tie rule (|dx| == |dy|), su == 1 exactly (the clamp to R - 1), two ranges per direction
        c["directions_R%d" % R] = case([np.concatenate([2.0 * dirs, 2.5 * dirs])], np.concatenate([dirs, 3.0 * dirs, 2.0 * dirs]), R)
    c["clamp"] = case([[[2, 2, 0.5], [-2, 0.5, 2], [0.25, -3, -3], [1, 1, -1]]], [[1, 1, 0.25], [-1, 0.25, 1], [0.125, -1.5, -1.5], [3, 3, -3]])
    zero = np.array([[1, -0.0, 0.0], [-0.0, 1, 0.0], [0.0, -0.0, -1], [-1, -0.0, -0.0]])
    c["negative_zero"] = case([2.0 * zero], np.concatenate([zero, 3.0 * zero]))
    # void pairs: a point at the scanner, coordinates 3e38 apart, NaN and infinities on either side
    o = [0.5, -0.3, 0.2]
    seen = [[0, 0, 0], [1, 0, 0], [0, 2, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [-1, 0, 0]]
    c["void_at_scanner"] = case([(seen, moved_to(o))], [o, [1.0, -0.3, 0.2], [np.nan, 1, 1], [np.inf, 0, 0], [0.5, 1.0, 0.2], [-np.inf, np.nan, 0], [-2, -0.3, 0.2]])
    c["void_overflow"] = case([([[-3e38, 0, 0], [-3.4e38, 1, 0], [1e30, 0, 0], [0, 1e20, 0], [0, 1e10, 0], [0, 0, -5e18]], moved_to([3e38, 0, 0]))],
                              [[-3e38, 0, 0], [2.9e38, 0, 0], [0, 0, 0], [3.4e38, 0, 0], [3e38, 5, 0], [3e38, 0, -1e19]])
    # two scans of which one observes and one does not; a query in front of a farther surface
    c["two_scans"] = case([([[5, 0, 0], [5, 0.05, 0]], IDENTITY), ([[0.05, -10, 0], [0, 5, 0]], moved_to([1, 10, 0]))], [[1, 0, 0], [4, 0, 0], [6, 0, 0], [1, 12, 0], [0, 0, 7]])
    many = []
    for s in range(64):
        at = rng.normal(0, 2.0, 3)
        many.append((rng.normal(0, 5.0, (40, 3)), P.rotation(7.0 * s, -3.0 * s, at)))
    c["scans_64"] = case(many, rng.normal(0, 1.0, (100, 3)), 16)
    far = P.rotation(33.0, -12.0, [1.0e4, -2.0e4, 0.5e4])
    c["far_transform"] = case([(rng.normal(0, 3.0, (3000, 3)), far)], rng.normal(0, 2.0, (200, 3)) + [1.0e4, -2.0e4, 0.5e4], 16)
    return c


def random_case(seed=7, scans=3, points=5000, queries=4000):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(scans):
        x = rng.normal(0, 2.0, (points, 3))
        x[rng.integers(0, points, 5), rng.integers(0, 3, 5)] = (np.nan, np.inf, -np.inf, np.nan, np.inf)
        out.append(scan(x, P.rotation(20.0 * s, 10.0 - 5.0 * s, rng.normal(0, 0.5, 3))))
    q = rng.normal(0, 1.5, (queries, 3))
    q[rng.integers(0, queries, 4), rng.integers(0, 3, 4)] = (np.nan, np.inf, -np.inf, np.nan)
    return out, cloud(q)


# the threshold: one scan point at (3, 4, 0), range 5; the query (3, 3.4375, 0) lies in the same texel of a 16-cube at range 4.5625
# (48 : 55 : 73 scaled by 1 / 16; every square and both roots are exact), so its gap is exactly 0.4375 while its distance to the
# truth point is 0.5625.  With the tolerances (0.4375 - 1 ulp, 0.4375) the gap is one ulp above the first and equal to the second.
THRESHOLD = dict(scans=[scan([[3, 4, 0]])], recon=cloud([[3, 3.4375, 0]]), tolerances=[float(np.nextafter(F(0.4375), F(0))), 0.4375], R=16)
# accurate wins: (1, 0, 0) is within 0.1 of the second scan's truth point (1.05, 0, 0) and 4 in front of the first scan's wall
ACCURATE_FIRST = dict(scans=[scan([[5, 0, 0]]), scan([[0.05, -10, 0]], moved_to([1, 10, 0]))], recon=cloud([[1, 0, 0], [2, 0, 0]]), tolerances=[0.1, 0.5], R=16)


# ---- the room ---------------------------------------------------------------------------------------------------------------------
ROOM_R = 64
ROOM_SCANNERS = [[0.0, 0.0, 0.0], [0.5, -0.3, 0.2]]
ROOM_TOLERANCES = [0.05, 0.1, 0.5]


def room_walls(step=0.02, half=2.0):
    """the six walls of a cube of edge 2 half, sampled every `step`"""
    n = int(round(2 * half / step)) + 1
    a = np.linspace(-half, half, n)
    u, v = (g.reshape(-1) for g in np.meshgrid(a, a, indexing="ij"))
    walls = []
    for axis in range(3):
        for side in (-half, half):
            w = np.empty((len(u), 3))
            w[:, axis] = side
            w[:, (axis + 1) % 3], w[:, (axis + 2) % 3] = u, v
            walls.append(w)
    return np.concatenate(walls)


def room(seed=13, inner=2000, outer=2000, on_walls=3000, scanners=2):
    """dict(scans, recon, inner, outer, walls: index ranges into recon): every scanner sees all six walls; the reconstruction holds
    points in the inner +-1.4 m box, points 0.6 m outside a wall, and wall samples as the first scan brought them into the scene"""
    rng = np.random.default_rng(seed)
    walls = room_walls()
    scans = [scan((walls - np.asarray(o)).astype(np.float32), moved_to(o)) for o in ROOM_SCANNERS[:scanners]]
    inside = rng.uniform(-1.4, 1.4, (inner, 3))
    outside = rng.uniform(-1.9, 1.9, (outer, 3))
    axis, side = rng.integers(0, 3, outer), rng.choice([-2.6, 2.6], outer)
    outside[np.arange(outer), axis] = side
    sampled = truth_points(*scans[0])[rng.choice(len(walls), on_walls, replace=False)]
    return dict(scans=scans, recon=cloud(np.concatenate([inside, outside, sampled])), inner=slice(0, inner), outer=slice(inner, inner + outer),
                walls=slice(inner + outer, inner + outer + on_walls))


def plate_scene():
    """(scans with the plate in the first one, the points behind it): a plate at x = 1, 0.6 m wide, between the first scanner and the
    wall x = 2; the points at x = 1.5 lie behind it as the first scanner sees them and in the open as the second one does"""
    r = room()
    a = np.arange(-0.3, 0.3001, 0.01)
    y, z = (g.reshape(-1) for g in np.meshgrid(a, a, indexing="ij"))
    plate = np.stack([np.full(len(y), 1.0), y, z], 1)
    first = scan(np.concatenate([r["scans"][0][0], cloud(plate)]), r["scans"][0][1])
    rng = np.random.default_rng(3)
    behind = np.stack([np.full(50, 1.5), rng.uniform(-0.1, 0.1, 50), rng.uniform(-0.1, 0.1, 50)], 1)
    return [first, r["scans"][1]], cloud(behind)
