"""numpy / Python model of the monocular-depth plane prior of a FIRST_INIT pass, written from the reference's text
(APD.cpp:24-80, 1210-1424) and the definitions host/prior.cpp states: the barycentric sweep over a triangle list, the rate map, the
division, RescaleMatToTargetSize to the working size and PlanesFromDepth.  Typed arithmetic: np.float32 / np.float64 scalars and
arrays wherever the C++ has that type, one IEEE operation per operator.  The sweep is the source's two loops — every triangle in
list order, every row of it, the row's columns as one typed array in column order — and simply overwrites: the model knows
nothing of owner maps.  What it records on the way (who reached a pixel first, how many did) is what the tests' claims need.

The triangle list is an input: it comes from the serial host build (tests/prior_host), whose Delaunay construction the existing
test_host_oracles.py test holds against scipy.  CASES are the smallest shapes at which the kernels can still go wrong."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

f32, f64 = np.float32, np.float64
TRI_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4"), ("x3", "<i4"), ("y3", "<i4"),
                      ("r1", "<f4"), ("r2", "<f4"), ("r3", "<f4"), ("step", "<f4")])
assert TRI_DTYPE.itemsize == 40


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def differing(a, b):
    return int((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).sum())


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def sequence(step):
    """the values a float loop counter takes: `for (float p = 0; p < 1.0; p += step)`"""
    out, p = [], f32(0)
    while f64(p) < f64(1.0):
        out.append(p)
        p = f32(p + f32(step))
    return np.array(out, f32)


def _area(ax, ay, bx, by, cx, cy):
    """triangleArea (APD.cpp:24-28), binary64"""
    return f64(0.5) * np.abs(ax * (by - cy) + bx * (cy - ay) + cx * (ay - by))


def calculate_z(t, x, y):
    """calculateZ (APD.cpp:30-49) of triangle t at the integer pixels (x, y), binary64"""
    ax, ay, az = f64(t["x1"]), f64(t["y1"]), f64(t["r1"])
    bx, by, bz = f64(t["x2"]), f64(t["y2"]), f64(t["r2"])
    cx, cy, cz = f64(t["x3"]), f64(t["y3"]), f64(t["r3"])
    px, py = x.astype(f64), y.astype(f64)
    abc = _area(ax, ay, bx, by, cx, cy)
    u = _area(px, py, bx, by, cx, cy) / abc
    v = _area(px, py, cx, cy, ax, ay) / abc
    w = _area(px, py, ax, ay, bx, by) / abc
    return u * az + v * bz + w * cz


def sweep(tris, middle_rate, cols, rows):
    """the rate map of APD.cpp:1276-1350 from the triangle list.  Returns dict(rate, owner = the triangle whose value the pixel
    holds (-1: none), first = the first triangle that reached it, reached = how many triangles did, differ = pixels that two
    triangles gave different values, rows = sweep rows over all triangles)"""
    rate = np.full((rows, cols), f32(middle_rate), f32)
    owner = np.full((rows, cols), -1, np.int32)
    first = np.full((rows, cols), -1, np.int32)
    reached = np.zeros((rows, cols), np.int32)
    differ = np.zeros((rows, cols), bool)
    total_rows = 0
    for k, t in enumerate(tris):
        seq = sequence(t["step"])               # q restarts at 0 in every row: one sequence per triangle serves p and q
        total_rows += len(seq)
        x1, x2, x3 = f32(t["x1"]), f32(t["x2"]), f64(t["x3"])
        y1, y2, y3 = f32(t["y1"]), f32(t["y2"]), f64(t["y3"])
        seen = np.zeros((rows, cols), bool)
        for p in seq:
            limit = f64(1.0) - f64(p)
            ok = seq.astype(f64) < limit
            n = len(seq) if ok.all() else int(np.argmin(ok))     # the loop ends at the first q that fails
            q = seq[:n]
            third = (f64(1.0) - f64(p) - q.astype(f64))
            x = ((p * x1 + q * x2).astype(f64) + third * x3).astype(np.int32)    # float * float, float + float, + double, truncated
            y = ((p * y1 + q * y2).astype(f64) + third * y3).astype(np.int32)
            assert ((x >= 0) & (x < cols) & (y >= 0) & (y < rows)).all(), (k, t)
            z = calculate_z(t, x, y).astype(f32)
            other = (owner[y, x] >= 0) & (owner[y, x] != k)
            differ[y[other], x[other]] |= rate[y[other], x[other]].view(np.uint32) != z[other].view(np.uint32)
            rate[y, x] = z                        # (a repeated pixel gets the same value: it depends on (x, y) only)
            owner[y, x] = k
            seen[y, x] = True
        first[seen & (first < 0)] = k
        reached += seen
    return dict(rate=rate, owner=owner, first=first, reached=reached, differ=differ, rows=total_rows)


def working_depth(raw, rate, W, H):
    """dep <- (255 - dep) / rate (APD.cpp:1221-1225, 1352-1356), then RescaleMatToTargetSize (APD.cpp:1773-1795) unless the sizes
    agree: nearest neighbour, the ROW index over the WIDTH ratio, the column index over the height ratio, 0 outside the source"""
    rows, cols = raw.shape
    with np.errstate(all="ignore"):
        metric = (f32(255) - raw) / rate
    if (cols, rows) == (W, H):
        return metric
    scale_x, scale_y = f32(W) / f32(cols), f32(H) / f32(rows)
    o_r = (np.arange(H).astype(f32) / scale_x).astype(np.int32)
    o_c = (np.arange(W).astype(f32) / scale_y).astype(np.int32)
    ok = ((o_r >= 0) & (o_r < rows))[:, None] & ((o_c >= 0) & (o_c < cols))[None, :]
    out = np.zeros((H, W), f32)
    rr, cc = np.nonzero(ok)
    out[rr, cc] = metric[o_r[rr], o_c[cc]]
    return out


def planes_from_depth(dep, cam):
    """APD.cpp:1365-1422: (H, W, 4) float32, world normal and depth; border pixels keep a zero normal"""
    H, W = dep.shape
    K, R = cam["K"].astype(f32).reshape(9), cam["R"].astype(f32).reshape(9)
    out = np.zeros((H, W, 4), f32)
    out[:, :, 3] = dep
    if H < 3 or W < 3:
        return out
    ys, xs = np.mgrid[1:H - 1, 1:W - 1]

    def point(x, y, d):     # Get3DPoint (APD.cpp:527-534): int - float, one product, one division
        return d * (x.astype(f32) - K[2]) / K[0], d * (y.astype(f32) - K[5]) / K[4], d

    with np.errstate(all="ignore"):
        X = point(xs, ys, dep[1:H - 1, 1:W - 1])
        Xdx = point(xs + 1, ys, dep[1:H - 1, 2:W])
        Xdy = point(xs, ys + 1, dep[2:H, 1:W - 1])
        ax, ay, az = Xdx[0] - X[0], Xdx[1] - X[1], Xdx[2] - X[2]
        bx, by, bz = Xdy[0] - X[0], Xdy[1] - X[1], Xdy[2] - X[2]
        n = [ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx]
        assert all(v.dtype == f32 for v in n)
        n64 = [v.astype(f64) for v in n]
        length = np.sqrt(n64[0] * n64[0] + n64[1] * n64[1] + n64[2] * n64[2])     # cv::normalize: binary64, zero stays zero
        inv = np.where(length != 0, f64(1.0) / length, f64(0.0))
        n = [(v * inv).astype(f32) for v in n64]
        norm = np.sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2])
        v = [X[0] / norm, X[1] / norm, X[2] / norm]
        flip = (n[0] * v[0] + n[1] * v[1] + n[2] * v[2]) > f32(0)
        n = [np.where(flip, -c, c) for c in n]
        out[1:H - 1, 1:W - 1, 0] = R[0] * n[0] + R[3] * n[1] + R[6] * n[2]
        out[1:H - 1, 1:W - 1, 1] = R[1] * n[0] + R[4] * n[1] + R[7] * n[2]
        out[1:H - 1, 1:W - 1, 2] = R[2] * n[0] + R[5] * n[1] + R[8] * n[2]
    assert out.dtype == f32
    return out


def model(raw, tris, middle_rate, W, H, cam):
    """every stage from the triangle list on"""
    rows, cols = raw.shape
    m = sweep(tris, middle_rate, cols, rows)
    m["depth"] = working_depth(raw, m["rate"], W, H)
    m["planes"] = planes_from_depth(m["depth"], cam)
    return m


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def camera():
    """one camera record for every case: the file camera and the working-size reference camera (test_host --prior uses the file's
    for both)"""
    import importlib
    synth = importlib.import_module("dvp-mvs_amd.synth")
    return synth.make_scene(96, 72, 1)["cameras"][0].copy()


def _raw_map(cols, rows):
    yy, xx = np.mgrid[0:rows, 0:cols].astype(f64)
    z = 4.0 + 0.9 * xx / cols + 0.6 * yy / rows + 0.15 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
    scale = 20.0 * (1.0 + 0.3 * xx / cols - 0.2 * yy / rows)
    return (255.0 - scale * z).astype(f32), z


def _world(cam, px, py, z):
    """the world point that the camera sees at image position (px, py) and depth z, float32"""
    K, R, t = cam["K"].astype(f64).reshape(3, 3), cam["R"].astype(f64).reshape(3, 3), cam["t"].astype(f64)
    Xc = np.array([z * (px - K[0, 2]) / K[0, 0], z * (py - K[1, 2]) / K[1, 1], z])
    return (R.T @ (Xc - t)).astype(f32)


def _points(cam, z, positions):
    """positions: (x, y) or (x, y, (proj_x, proj_y)) or (x, y, (proj_x, proj_y), depth factor): the image position the file
    names and, if it differs, where the 3-D point projects to"""
    xy, xyz = [], []
    for item in positions:
        x, y = item[0], item[1]
        qx, qy = item[2] if len(item) > 2 else (x, y)
        zi = z[min(max(int(qy), 0), z.shape[0] - 1), min(max(int(qx), 0), z.shape[1] - 1)] * (item[3] if len(item) > 3 else 1.0)
        xy.append((x, y))
        xyz.append(_world(cam, qx, qy, zi))
    return np.array(xy, f32).reshape(-1, 2), np.array(xyz, f32).reshape(-1, 3)


def _case(name, cols, rows, W, H, positions):
    raw, z = _raw_map(cols, rows)
    xy, xyz = _points(camera(), z, positions)
    return dict(name=name, raw=raw, xy=xy, xyz=xyz, W=W, H=H)


def _case3_positions():
    cols, rows = 191, 143
    special = [
        (30.2, 25.3), (30.2, 25.3, (30.2, 25.3), 1.25),                  # one position twice, two 3-D points: the second rate wins
        (50.2, 60.3), (50.7, 60.6), (50.4, 60.8),                        # three points on one pixel: max_edge_length = 0
        (100.1, 40.2), (101.1, 40.8), (102.1, 40.3),                     # truncated corners (100, 40), (101, 40), (102, 40): collinear
        (195.2, 50.3, (120.2, 50.3)),                                    # a position outside the map (not inserted), a projection inside
        (70.2, 90.3, (0.2, 90.3)),                                       # projects onto column 0: rejected by ix > 0
        (84.2, 142.3), (190.4, 71.3),                                    # a corner on the last row, one on the last column
    ]
    rng = np.random.default_rng(20240)
    keep = [(30.2, 25.3), (50.5, 60.5), (101.1, 40.5), (84.2, 142.3), (190.4, 71.3)]
    out = list(special)
    while len(out) < 60:
        x, y = int(rng.integers(3, cols - 3)) + 0.2, int(rng.integers(3, rows - 3)) + 0.3
        if min((x - a) ** 2 + (y - b) ** 2 for a, b in keep) < 49:
            continue
        keep.append((x, y))
        out.append((x, y))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return (
        # 1: the five hand-placed points of test_host_oracles.py; the hull's edges are longer than 64 steps
        _case("hand_96x72", 96, 72, 96, 72, [(12, 10), (80, 14), (70, 60), (15, 55), (44, 33)]),
        # 2: other aspect ratio: the swapped ratios send target rows >= 48 outside the source
        _case("aspect_200x100_to_96x72", 200, 100, 96, 72, [(20, 12), (180, 15), (170, 88), (25, 84), (96, 47), (60, 30), (140, 66)]),
        # 3: inexact ratios, fractional positions, every special point
        _case("specials_191x143_to_96x72", 191, 143, 96, 72, _case3_positions()),
        # 4: triangles of more than 256 steps, a width that is no multiple of 64
        _case("long_400x300", 400, 300, 400, 300, [(10, 12), (390, 8), (385, 290), (14, 285), (200, 140), (120, 220), (300, 70), (250, 200)]),
    )


CASES = ("hand_96x72", "aspect_200x100_to_96x72", "specials_191x143_to_96x72", "long_400x300")


def case(k):
    return cases()[k]


def unusable_cases():
    """5: status 1 — no point lands in the map (behind the camera / far outside); an empty map"""
    raw, z = _raw_map(96, 72)
    cam = camera()
    xy, xyz = _points(cam, z, [(10, 10, (-40.0, 10.0)), (20, 20, (300.0, 20.0)), (30, 30, (30.0, -9.0))])
    return (dict(name="no_usable_point", raw=raw, xy=xy, xyz=xyz, W=96, H=72),
            dict(name="no_points", raw=raw, xy=np.zeros((0, 2), f32), xyz=np.zeros((0, 3), f32), W=96, H=72),
            dict(name="empty_map", raw=np.zeros((0, 0), f32), xy=xy, xyz=xyz, W=96, H=72))


# ---- the serial host build (tests/prior_host) -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def serial_lib():
    d = os.path.join(ROOT, "tests", "prior_host")
    subprocess.check_call(["make", "-s", "-C", d])
    L = ctypes.CDLL(os.path.join(d, "libdvp_prior_host.so"))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.dvp_prior_triangles_serial.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    L.dvp_prior_owner_serial.restype = ctypes.c_longlong
    L.dvp_prior_owner_serial.argtypes = [vp, ci, ci, ci, vp]
    L.dvp_prior_rate_serial.restype = None
    L.dvp_prior_rate_serial.argtypes = [vp, vp, ctypes.c_float, ci, ci, vp]
    L.dvp_prior_depth_serial.restype = None
    L.dvp_prior_depth_serial.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    L.dvp_prior_planes_serial.restype = None
    L.dvp_prior_planes_serial.argtypes = [vp, ci, ci, vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def serial_triangles(c, cam=None):
    """the host part: (status, middle_rate, triangle list, how often each skip rule fired)"""
    L = serial_lib()
    cam = camera() if cam is None else cam
    raw = np.ascontiguousarray(c["raw"], f32)
    rows, cols = raw.shape
    K, R, t = (np.ascontiguousarray(cam[n], f32).reshape(-1) for n in ("K", "R", "t"))
    cap = 4 * len(c["xy"]) + 16
    tris = np.zeros(cap, TRI_DTYPE)
    middle, count, skipped = np.zeros(1, f32), np.zeros(1, np.int32), np.zeros(3, np.int64)
    xy, xyz = np.ascontiguousarray(c["xy"], f32), np.ascontiguousarray(c["xyz"], f32)
    status = L.dvp_prior_triangles_serial(_p(raw), cols, rows, _p(xy), _p(xyz), len(xy), _p(K), _p(R), _p(t), _p(middle), _p(tris), cap, _p(count), _p(skipped))
    assert count[0] <= cap
    return status, middle[0], tris[:count[0]].copy(), skipped


def serial_stages(c, tris, middle, cam=None):
    """the device's decomposition, run serially: dict(owner, rate, depth, planes, rows)"""
    L = serial_lib()
    cam = camera() if cam is None else cam
    raw = np.ascontiguousarray(c["raw"], f32)
    rows, cols = raw.shape
    W, H = c["W"], c["H"]
    tris = np.ascontiguousarray(tris)
    owner = np.empty((rows, cols), np.int32)
    n_rows = L.dvp_prior_owner_serial(_p(tris), len(tris), cols, rows, _p(owner))
    rate = np.empty((rows, cols), f32)
    L.dvp_prior_rate_serial(_p(tris), _p(owner), ctypes.c_float(float(middle)), cols, rows, _p(rate))
    depth = np.empty((H, W), f32)
    L.dvp_prior_depth_serial(_p(raw), _p(rate), cols, rows, W, H, _p(depth))
    planes = np.empty((H, W, 4), f32)
    K, R = (np.ascontiguousarray(cam[n], f32).reshape(-1) for n in ("K", "R"))
    L.dvp_prior_planes_serial(_p(depth), W, H, _p(K), _p(R), _p(planes))
    return dict(owner=owner, rate=rate, depth=depth, planes=planes, rows=int(n_rows))


@functools.lru_cache(maxsize=None)
def expected(k):
    """(middle_rate, triangle list, skip counts, the model's stages) of case k, computed once and shared: leave it unchanged"""
    c = case(k)
    status, middle, tris, skipped = serial_triangles(c)
    assert status == 0
    m = model(c["raw"], tris, middle, c["W"], c["H"], camera())
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    tris.setflags(write=False)
    return middle, tris, skipped, m


# ---- a dense folder of a case, as the driver and test_host --prior read it -----------------------------------------------------------
def write_cam(path, cam):
    R, t, K = cam["R"].reshape(3, 3), cam["t"], cam["K"].reshape(3, 3)
    with open(path, "w") as f:
        f.write("extrinsic\n")
        for i in range(3):
            f.write("%.9g %.9g %.9g %.9g\n" % (R[i, 0], R[i, 1], R[i, 2], t[i]))
        f.write("0.0 0.0 0.0 1.0\n\nintrinsic\n")
        for i in range(3):
            f.write("%.9g %.9g %.9g\n" % tuple(K[i]))
        dmin, dmax = float(cam["depth_min"]), float(cam["depth_max"])
        f.write("\n%.9g %.9g %d %.9g\n" % (dmin, (dmax - dmin) / 192.0, 192, dmax))


def write_folder(d, c, view=0):
    """cams/, dep/ and sfm/ of one view; %.9g round-trips every float32"""
    for sub in ("cams", "dep", "sfm"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    write_cam(os.path.join(d, "cams", "%08d_cam.txt" % view), camera())
    raw = np.ascontiguousarray(c["raw"], f32)
    with open(os.path.join(d, "dep", "%08d.dmb" % view), "wb") as f:     # BinMat: version, rows, cols, CV_32FC1
        f.write(np.array([1, raw.shape[0], raw.shape[1], 5], np.int32).tobytes())
        f.write(raw.tobytes())
    with open(os.path.join(d, "sfm", "%08d.txt" % view), "w") as f:
        for (x, y), (X, Y, Z) in zip(c["xy"], c["xyz"]):
            f.write("%.9g %.9g %.9g %.9g %.9g 128 128 128\n" % (x, y, X, Y, Z))
