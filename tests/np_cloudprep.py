"""TEST INFRASTRUCTURE: the preparation in front of `apd --evaluate` (csrc/dvp_cloudprep.hpp) read independently in numpy - binary64
arrays, one rounding per operator, np.add.at on uint64 for the fixed-point sums -, the case table that the host and the device tests
share, and the runner of tests/cloudprep_host.  A preparation is a dict(transform=16 numbers or None, crop=dict(axis, axis_min,
axis_max, polygon (n, 3)) or None, voxel=s or 0.0)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "cloudprep_host", "cloudprep_host")
TWO32 = 4294967296.0


def cloud(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def prep(transform=None, crop=None, voxel=0.0):
    return dict(transform=transform, crop=crop, voxel=voxel)


def crop_of(axis, axis_min, axis_max, polygon):
    return dict(axis=axis, axis_min=float(axis_min), axis_max=float(axis_max), polygon=np.asarray(polygon, np.float64).reshape(-1, 3))


def uv_of(axis):
    return ((1, 2), (0, 2), (0, 1))[axis]


def polygon_3d(axis, uv, w=0.0):
    """(n, 3) vertices from (n, 2) (u, v) pairs; the coordinate along the axis is never read"""
    uv = np.asarray(uv, np.float64)
    out = np.full((len(uv), 3), w, np.float64)
    u, v = uv_of(axis)
    out[:, u], out[:, v] = uv[:, 0], uv[:, 1]
    return out


# ---- the definition -------------------------------------------------------------------------------------------------------------
def inside_crop(p, crop):
    """bool per row of the (N, 3) float64 points"""
    w = crop["axis"]
    u, v = uv_of(w)
    V = crop["polygon"]
    pu, pv = p[:, u], p[:, v]
    crossings = np.zeros(len(p), np.int64)
    with np.errstate(all="ignore"):
        for i in range(len(V)):
            j = (i + 1) % len(V)
            iu, iv, ju, jv = V[i, u], V[i, v], V[j, u], V[j, v]
            crosses = ((iv < pv) & (jv >= pv)) | ((jv < pv) & (iv >= pv))
            side = iu + (pv - iv) / (jv - iv) * (ju - iu) < pu
            crossings += crosses & side
    return (crop["axis_min"] <= p[:, w]) & (p[:, w] <= crop["axis_max"]) & (crossings % 2 == 1)


def voxel_parts(p, s):
    """(o (3,), i (N, 3) float64, q (N, 3) uint64) of the kept points"""
    o = p.min(0) - s * 0.5
    t = (p - o) / s
    i = np.floor(t)
    q = np.floor((t - i) * TWO32).astype(np.uint64)
    return o, i, q


def prepare(xyz, transform=None, crop=None, voxel=0.0):
    """dict(xyz (M, 3) float32, first_index (M,) int64, counts (4,) int64)"""
    x = cloud(xyz)
    index = np.flatnonzero(np.isfinite(x).all(1))
    p = x[index].astype(np.float64)
    counts = [len(index)]
    with np.errstate(all="ignore"):
        if transform is not None:
            m = np.asarray(transform, np.float64).reshape(4, 4)
            p = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], 1)
            ok = np.isfinite(p).all(1)
            p, index = p[ok], index[ok]
        counts.append(len(index))
        if crop is not None:
            ok = inside_crop(p, crop)
            p, index = p[ok], index[ok]
        counts.append(len(index))
        if voxel != 0.0 and len(p):
            s = float(voxel)
            o, i, q = voxel_parts(p, s)
            _, first, inverse = np.unique(i, axis=0, return_index=True, return_inverse=True)
            inverse = inverse.reshape(-1)
            Q = np.zeros((len(first), 3), np.uint64)
            np.add.at(Q, inverse, q)
            n = np.bincount(inverse, minlength=len(first))
            c = o + (i[first] + (Q.astype(np.float64) / n.astype(np.float64)[:, None]) * (1.0 / TWO32)) * s
            order = np.argsort(first, kind="stable")
            p, index = c[order], index[first[order]]
        out = p.astype(np.float32)
    counts.append(len(index))
    return dict(xyz=out.reshape(-1, 3), first_index=index.astype(np.int64), counts=np.array(counts, np.int64))


# ---- the project's text on the host ---------------------------------------------------------------------------------------------
def build_program():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROGRAM)])


def run_program(*args):
    return subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def prep_text(transform=None, crop=None, voxel=0.0):
    words = []
    if transform is not None:
        words += ["transform"] + [float(v).hex() for v in np.asarray(transform, np.float64).reshape(-1)]
    if crop is not None:
        poly = np.asarray(crop["polygon"], np.float64).reshape(-1)
        words += ["crop", str(int(crop["axis"])), float(crop["axis_min"]).hex(), float(crop["axis_max"]).hex(), str(len(poly) // 3)] + [float(v).hex() for v in poly]
    if voxel != 0.0:
        words += ["voxel", float(voxel).hex()]
    return " ".join(words) + "\n"


def serial(xyz, tmp, transform=None, crop=None, voxel=0.0):
    """(return code, stderr, dict or None) of cloudprep_host prepare"""
    files = [os.path.join(str(tmp), n) for n in ("cloud.bin", "prep.txt", "xyz.out", "index.out")]
    cloud(xyz).tofile(files[0])
    with open(files[1], "w") as f:
        f.write(prep_text(transform, crop, voxel))
    out = run_program("prepare", *files)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    counts = np.array([int(v) for v in out.stdout.split()[1:]], np.int64)
    return 0, out.stderr, dict(xyz=np.fromfile(files[2], np.float32).reshape(-1, 3), first_index=np.fromfile(files[3], np.int64), counts=counts)


def same_result(got, want):
    """"" or what differs between two prepared clouds (xyz bit for bit; first_index and counts exactly)"""
    if not np.array_equal(got["counts"], want["counts"]):
        return "counts: %s, expected %s" % (list(got["counts"]), list(want["counts"]))
    if not np.array_equal(got["first_index"], want["first_index"]):
        return "first_index differs"
    a, b = got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)
    if a.shape != b.shape or not (a == b).all():
        bad = np.flatnonzero((a != b).any(1)) if a.shape == b.shape else []
        return "xyz differs at %s: %s, expected %s" % (list(bad[:5]), got["xyz"][bad[:2]].tolist(), want["xyz"][bad[:2]].tolist())
    return ""


# ---- the case table: name -> (xyz, preparation) -----------------------------------------------------------------------------------
BIG_SQUARE = [[-100, -100], [100, -100], [100, 100], [-100, 100]]
CONCAVE = [[0, 0], [4, 0], [4, 4], [2, 2], [0, 4]]      # a horizontal edge at v = 0, two slanted edges that meet at the vertex (2, 2)
CONCAVE_12 = [[0.0, 0.0], [0.35, 0.1], [0.7, 0.0], [0.6, 0.3], [1.0, 0.5], [0.65, 0.6], [0.75, 1.0], [0.45, 0.7], [0.2, 0.95], [0.3, 0.55], [-0.1, 0.45], [0.15, 0.3]]


def kept_by_z(n, pattern, rng):
    """n points of which a crop along z with bounds [-1, 1] keeps all, none or every other one"""
    x = rng.random((n, 3))
    x[:, 2] = {"all": 0.0, "none": 10.0}.get(pattern, 0.0)
    if pattern == "alternate":
        x[1::2, 2] = 10.0
    return cloud(x), prep(crop=crop_of(2, -1.0, 1.0, polygon_3d(2, BIG_SQUARE)))


def edge_points(axis, axis_min, axis_max):
    """every (u, v) of the integer grid -1 ... 5 around CONCAVE - its vertices' v exactly, points on the horizontal edge, on the two
    slanted edges and on either side of them - at five places along the axis: on both bounds, one ulp outside either, in between"""
    lo, hi = np.float32(axis_min), np.float32(axis_max)
    ws = [lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)), np.float32(0.5) * (lo + hi)]
    u, v = uv_of(axis)
    pts = []
    for w in ws:
        for a in range(-1, 6):
            for b in range(-1, 6):
                p = np.zeros(3, np.float32)
                p[axis], p[u], p[v] = w, a, b
                pts.append(p)
    return cloud(pts), prep(crop=crop_of(axis, float(lo), float(hi), polygon_3d(axis, CONCAVE)))


def rotation(deg_z, deg_x, translation):
    a, b = np.radians(deg_z), np.radians(deg_x)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    m = np.eye(4)
    m[:3, :3] = rz @ rx
    m[:3, 3] = translation
    return m.reshape(-1)


def table_cloud(seed=5):
    """6000 points in 6000 voxels of edge 1: the table has 16384 slots, the smallest capacity for them"""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(40 * 40 * 40)[:6000]
    base = np.stack([cells // 1600, (cells // 40) % 40, cells % 40], 1).astype(np.float64)
    pts = base + 0.6 + 0.3 * rng.random((6000, 3))
    pts[0] = 0.5      # the minimum: o = 0
    return cloud(pts)


def combined_scene(n=20000, seed=21):
    rng = np.random.default_rng(seed)
    x = cloud(rng.random((n, 3)) * [1.4, 1.4, 1.0] - [0.2, 0.2, 0.0])
    x[rng.integers(0, n, 20), rng.integers(0, 3, 20)] = np.nan
    m = rotation(30.0, 10.0, [0.1, -0.05, 0.02])
    return x, prep(transform=m, crop=crop_of(2, 0.1, 0.8, polygon_3d(2, CONCAVE_12)), voxel=0.04)


def cases():
    rng = np.random.default_rng(17)
    c = {}
    # compaction: the wave's ballot word, the work-group's four words, the ragged tail
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        for pattern in ("all", "none", "alternate"):
            c["keep_%s_%d" % (pattern, n)] = kept_by_z(n, pattern, rng)
    c["keep_scan_seam"] = kept_by_z(1024 * 256 + 300, "alternate", rng)      # more work-groups than one scan block covers
    bad = rng.random((200, 3))
    for k, i in enumerate((0, 63, 64, 127, 128, 199)):
        bad[i, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    c["non_finite"] = (cloud(bad), prep())
    c["non_finite_voxel"] = (cloud(bad), prep(voxel=0.1))
    over = rng.random((70, 3))
    over[:, 0] = 0.0
    over[33, 0] = 1e10
    big = np.eye(4)
    big[0, 0] = 1e300
    c["transform_overflows_one"] = (cloud(over), prep(transform=big.reshape(-1)))
    # crop
    for axis in range(3):
        c["crop_edges_axis%d" % axis] = edge_points(axis, -0.75, 1.5)
        c["crop_concave_axis%d" % axis] = (cloud(rng.random((700, 3)) * 1.4 - 0.2), prep(crop=crop_of(axis, 0.1, 0.9, polygon_3d(axis, CONCAVE_12))))
    c["crop_triangle"] = (cloud(rng.random((500, 3))), prep(crop=crop_of(1, 0.0, 1.0, polygon_3d(1, [[0.1, 0.1], [0.9, 0.2], [0.4, 0.95]]))))
    angle = 2 * np.pi * np.arange(256) / 256
    c["crop_256_gon"] = (cloud(rng.random((900, 3))), prep(crop=crop_of(0, -1.0, 2.0, polygon_3d(0, 0.5 + 0.45 * np.stack([np.cos(angle), np.sin(angle)], 1)))))
    # transform
    plain = cloud(rng.random((300, 3)) + 0.5)
    c["transform_identity"] = (plain, prep(transform=np.eye(4).reshape(-1)))
    c["transform_rigid_1e4"] = (plain, prep(transform=rotation(40.0, -25.0, [1e4, -1e4, 1e4])))
    # voxels
    c["voxel_one_point"] = (cloud([[0.3, -0.2, 7.0]]), prep(voxel=0.05))
    c["voxel_65_in_one"] = (cloud(1.0 + 0.04 * rng.random((65, 3))), prep(voxel=0.25))
    c["voxel_4097_in_one"] = (cloud(1.0 + 0.04 * rng.random((4097, 3))), prep(voxel=0.25))
    # s = 0.5, the minimum 0: o = -0.25, the point at 0.25 has t = 1 exactly (on the face), the minimum itself t = 0.5
    c["voxel_face_and_minimum"] = (cloud([[0, 0, 0], [0.25, 0, 0], [0.2499, 0, 0], [0, 0.25, 0.25], [0.75, 0.75, 0.75], [0.7499, 0.75, 0.1]]), prep(voxel=0.5))
    c["voxel_near_1e4"] = (cloud(1e4 + 0.02 * rng.random((3000, 3))), prep(voxel=0.0025))
    c["voxel_table"] = (table_cloud(), prep(voxel=1.0))
    c["voxel_negative"] = (cloud(-5 + 2 * rng.random((2000, 3))), prep(voxel=0.1))
    c["voxel_shared"] = (cloud(rng.random((5000, 3))), prep(voxel=0.1))
    c["combined"] = combined_scene()
    return c
