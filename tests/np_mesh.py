"""TEST INFRASTRUCTURE: numpy restatement of csrc/dvp_mesh.hpp (the TSDF volume over a hashed block grid and its surface nets), kept
apart from the C++ text on purpose; the case table of the mesh tests; the stand-alone program's driver; mesh checks (manifold, Euler
characteristic, signed volume).  model(views, s, tau, min_weight) works in binary32 with one rounding per operator, as the serial text
does; with ft=np.float64 every real number is a binary64 instead (the yardstick of the accuracy bounds)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "mesh_host", "mesh_host")
CAMERA_DTYPE = np.dtype([("K", np.float32, 9), ("R", np.float32, 9), ("t", np.float32, 3), ("c", np.float32, 3),
                         ("height", np.int32), ("width", np.int32), ("depth_min", np.float32), ("depth_max", np.float32)])
LIMIT = 1 << 20


class Refused(Exception):
    pass


# ---- the definition ---------------------------------------------------------------------------------------------------------------

def lattice(i, s, ft):
    return (np.asarray(i).astype(np.float64) * np.float64(s)).astype(ft)


def block_keys(b):
    """keys of integer block coordinates (..., 3)"""
    b = np.asarray(b, np.int64) + LIMIT
    return ((b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]).astype(np.uint64)


def key_blocks(keys):
    k = np.asarray(keys, np.uint64).astype(np.int64)
    return np.stack([(k >> 42) - LIMIT, ((k >> 21) & 0x1fffff) - LIMIT, (k & 0x1fffff) - LIMIT], -1)


def _camera(cam, ft):
    K, R, t = cam["K"].astype(ft), cam["R"].astype(ft), cam["t"].astype(ft)
    c = np.array([-((R[0 + k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]) for k in range(3)], ft)
    return K, R, t, c


def lift(cam, x, y, z, ft):
    K, R, t, c = _camera(cam, ft)
    cx = z * (x.astype(ft) - K[2]) / K[0]
    cy = z * (y.astype(ft) - K[5]) / K[4]
    return [((R[0 + k] * cx + R[3 + k] * cy) + R[6 + k] * z) + c[k] for k in range(3)]


def project(cam, X, ft):
    K, R, t, _ = _camera(cam, ft)
    T = [((R[3 * k] * X[0] + R[3 * k + 1] * X[1]) + R[3 * k + 2] * X[2]) + t[k] for k in range(3)]
    depth = (K[6] * T[0] + K[7] * T[1]) + K[8] * T[2]
    px = ((K[0] * T[0] + K[1] * T[1]) + K[2] * T[2]) / depth
    py = ((K[3] * T[0] + K[4] * T[1]) + K[5] * T[2]) / depth
    return px, py, depth


def round_pixel(v, ft):
    t = v + ft(0.5)
    ok = (t > -2147483648.0) & (t < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, t, 0)), -1).astype(np.int64)


def band(s, tau):
    return int(np.ceil(np.float64(np.float32(tau)) / np.float64(np.float32(s))))


def blocks(views, s, tau, ft=np.float32):
    """the ascending keys of the allocated blocks"""
    M, keys = band(s, tau), [np.zeros(0, np.uint64)]
    s32 = np.float32(s)
    with np.errstate(all="ignore"):
        for n, (cam, depth, mask, _) in enumerate(views):
            ys, xs = np.nonzero((mask != 0) & (depth > 0))
            z = depth[ys, xs].astype(ft)
            for m in range(-2 * M, 2 * M + 1):
                zm = z + ft(m) * (ft(s32) * ft(0.5))
                X = lift(cam, xs, ys, zm, ft)
                q = np.stack([np.floor(c.astype(np.float64) / np.float64(s32)) for c in X], -1)
                if not ((q >= -LIMIT) & (q < LIMIT)).all():
                    raise Refused("a lattice index beyond 21 bits (view %d)" % n)
                keys.append(np.unique(block_keys(q.astype(np.int64) >> 3)))
    return np.unique(np.concatenate(keys))


def integrate(views, keys, s, tau, ft=np.float32):
    """sf (B, 512), w (B, 512), colour sums (B, 512, 4) of the blocks `keys`"""
    B = len(keys)
    l = np.arange(512)
    idx = key_blocks(keys)[:, None, :] * 8 + np.stack([l >> 6, (l >> 3) & 7, l & 7], -1)[None]
    P = [lattice(idx[..., a], np.float32(s), ft) for a in range(3)]
    sf, w, col = np.zeros((B, 512), ft), np.zeros((B, 512), np.int32), np.zeros((B, 512, 4), np.uint32)
    tau = ft(np.float32(tau))
    with np.errstate(all="ignore"):
        for cam, depth, mask, bgr in views:
            H, W = depth.shape
            px, py, zc = project(cam, P, ft)
            x, y = round_pixel(px, ft), round_pixel(py, ft)
            ok = (zc > 0) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            xi, yi = np.where(ok, x, 0), np.where(ok, y, 0)
            d = depth[yi, xi].astype(ft)
            ok &= (mask[yi, xi] != 0) & (d > 0)
            sdf = d - zc
            ok &= sdf >= -tau
            r = sdf / tau
            sf = np.where(ok, sf + np.where(r < 1, r, ft(1)), sf)
            w = w + ok
            near = ok & (np.abs(sdf) <= tau)
            col[..., :3] += np.where(near[..., None], bgr[yi, xi], 0).astype(np.uint32)
            col[..., 3] += near
    return sf, w.astype(np.int32), col


def extract(keys, sf, w, col, s, min_weight, ft=np.float32):
    """vertices (V, 3), colours (V, 3) uint8, faces (F, 3) int32"""
    B = len(keys)
    if B == 0:
        return np.zeros((0, 3), ft), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32)
    s = np.float32(s)
    at = key_blocks(keys)
    where = {int(k): b for b, k in enumerate(keys)}
    forward = np.full((B, 2, 2, 2), -1, np.int64)
    for b in range(B):
        for n in range(8):
            d = np.array([n >> 2, (n >> 1) & 1, n & 1])
            forward[b, d[0], d[1], d[2]] = where.get(int(block_keys(at[b] + d)), -1)
    g = np.arange(9)
    lx, ly, lz = np.meshgrid(g, g, g, indexing="ij")
    nb = forward[:, lx >> 3, ly >> 3, lz >> 3]                                   # (B, 9, 9, 9)
    index = np.where(nb >= 0, nb * 512 + ((lx & 7) * 64 + (ly & 7) * 8 + (lz & 7))[None], -1)
    flat = np.where(index >= 0, index, 0)
    with np.errstate(all="ignore"):
        F_all = np.where(w.reshape(-1) >= min_weight, sf.reshape(-1) / w.reshape(-1).astype(ft), ft(np.nan))
    F = np.where(index >= 0, F_all[flat], ft(np.nan))
    csum = np.where((index >= 0)[..., None], col.reshape(-1, 4)[flat], 0).astype(np.int64)
    corner = lambda A, c: A[:, (c >> 2):(c >> 2) + 8, ((c >> 1) & 1):((c >> 1) & 1) + 8, (c & 1):(c & 1) + 8]
    F8 = [corner(F, c) for c in range(8)]
    valid = np.all([~np.isnan(f) for f in F8], 0)
    inside = np.sum([f < 0 for f in F8], 0)
    active = valid & (inside > 0) & (inside < 8)
    cell = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1)[None] + at[:, None, None, None, :] * 8   # (B, 8, 8, 8, 3)
    total, count = [np.zeros(active.shape, ft) for _ in range(3)], np.zeros(active.shape, np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            b_, c_ = (1 if a == 0 else 0), (1 if a == 2 else 2)
            for q in range(4):
                d = [0, 0, 0]
                d[b_], d[c_] = q >> 1, q & 1
                c0 = d[0] * 4 + d[1] * 2 + d[2]
                c1 = c0 + (4 >> a)
                F0, F1 = F8[c0], F8[c1]
                cross = active & ((F0 < 0) != (F1 < 0))
                X = [lattice(cell[..., e] + d[e], s, ft) for e in range(3)]
                P1 = lattice(cell[..., a] + 1, s, ft)
                X[a] = X[a] + F0 / (F0 - F1) * (P1 - X[a])
                for e in range(3):
                    total[e] = np.where(cross, total[e] + X[e], total[e])
                count += cross
        vert = np.stack([total[e] / count.astype(ft) for e in range(3)], -1)[active]
    sums = np.sum([corner(csum, c) for c in range(8)], 0)                         # (B, 8, 8, 8, 4)
    n = sums[..., 3:4]
    colours = np.where(n > 0, (sums[..., :3] + n // 2) // np.maximum(n, 1), 0).astype(np.uint8)[active]
    number = np.full(B * 512, -1, np.int64)
    number[np.nonzero(active.reshape(-1))[0]] = np.arange(int(active.sum()))
    cv = np.where(index >= 0, number[flat], -1)                                   # the cells' vertex numbers over the 9 x 9 x 9 region
    quads, keep = np.zeros(active.shape + (3, 6), np.int64), np.zeros(active.shape + (3,), bool)
    F1 = F[:, 1:, 1:, 1:]
    for a in range(3):
        lo = [slice(1, 9)] * 3
        lo[a] = slice(0, 8)
        F0 = F[(slice(None),) + tuple(lo)]
        change = ~np.isnan(F0) & ~np.isnan(F1) & ((F0 < 0) != (F1 < 0))
        rises = F0 < 0
        b_, c_ = (a + 1) % 3, (a + 2) % 3
        v = []
        for q in range(4):
            d = [0, 0, 0]
            d[b_], d[c_] = int(q in (1, 2)), int(q in (2, 3))
            v.append(cv[:, d[0]:d[0] + 8, d[1]:d[1] + 8, d[2]:d[2] + 8])
        keep[..., a] = change & np.all([x >= 0 for x in v], 0)
        up = np.stack([v[0], v[1], v[2], v[0], v[2], v[3]], -1)
        down = np.stack([v[0], v[2], v[1], v[0], v[3], v[2]], -1)
        quads[..., a, :] = np.where(rises[..., None], up, down)
    return vert, colours, quads[keep].reshape(-1, 3).astype(np.int32)


def model(views, s, tau, min_weight, ft=np.float32):
    """dict(keys, sf, w, colour_sums, vertices, colours, faces) of the definition"""
    s, tau = np.float32(s), np.float32(tau)
    keys = blocks(views, s, tau, ft)
    sf, w, col = integrate(views, keys, s, tau, ft)
    v, c, f = extract(keys, sf, w, col, s, min_weight, ft)
    return dict(keys=keys, sf=sf, w=w, colour_sums=col, vertices=v, colours=c, faces=f)


# ---- the stand-alone program ------------------------------------------------------------------------------------------------------

def build_program():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(PROGRAM)])


def run_program(*args):
    return subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def write_scene(views, path):
    with open(path, "wb") as f:
        f.write(np.int32(len(views)).tobytes())
        for cam, depth, mask, bgr in views:
            f.write(np.ascontiguousarray(cam).tobytes())
            f.write(np.array([depth.shape[1], depth.shape[0]], np.int32).tobytes())
            f.write(np.ascontiguousarray(depth, np.float32).tobytes())
            f.write(np.ascontiguousarray(mask, np.uint8).tobytes())
            f.write(np.ascontiguousarray(bgr, np.uint8).tobytes())


def serial(views, s, tau, min_weight, tmp):
    """(return code, stderr, model()'s dict or None) of mesh_host build"""
    scene, prefix = os.path.join(str(tmp), "scene.bin"), os.path.join(str(tmp), "out")
    write_scene(views, scene)
    out = run_program("build", scene, repr(float(np.float32(s))), repr(float(np.float32(tau))), min_weight, prefix)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    load = lambda name, dtype: np.fromfile(prefix + "." + name, dtype)
    return 0, out.stderr, dict(keys=load("keys", np.uint64), sf=load("sf", np.float32).reshape(-1, 512), w=load("w", np.int32).reshape(-1, 512),
                               colour_sums=load("colour", np.uint32).reshape(-1, 512, 4), vertices=load("vertices", np.float32).reshape(-1, 3),
                               colours=load("colours", np.uint8).reshape(-1, 3), faces=load("faces", np.int32).reshape(-1, 3))


def cull(views, s, tau, tmp):
    """(cullable per view, skipped (blocks, views) bool in key order) of mesh_host cull: the device's view cull, run on the host"""
    scene, out = os.path.join(str(tmp), "cull_scene.bin"), os.path.join(str(tmp), "cull.bin")
    write_scene(views, scene)
    got = run_program("cull", scene, repr(float(np.float32(s))), repr(float(np.float32(tau))), out)
    assert got.returncode == 0, got.stderr
    cullable = np.array([int(line.split()[3]) for line in got.stdout.splitlines() if line.startswith("view ")], bool)
    assert len(cullable) == len(views)
    return cullable, np.fromfile(out, np.uint8).reshape(-1, len(views)).astype(bool)


PAIR_DTYPE = np.dtype([("view", np.int32), ("s", np.float32), ("tau", np.float32), ("at", np.int32, 3)])


def cull_pairs(views, pairs, tmp):
    """skipped per record of `pairs` (PAIR_DTYPE) of mesh_host cull_pairs"""
    scene, file, out = os.path.join(str(tmp), "pairs_scene.bin"), os.path.join(str(tmp), "pairs.bin"), os.path.join(str(tmp), "pairs_out.bin")
    write_scene(views, scene)
    np.ascontiguousarray(pairs, PAIR_DTYPE).tofile(file)
    got = run_program("cull_pairs", scene, file, out)
    assert got.returncode == 0, got.stderr
    return np.fromfile(out, np.uint8).astype(bool)


STAGES = ("keys", "sf", "w", "colour_sums", "vertices", "colours", "faces")


def same(got, want):
    """"" or the first stage whose bytes differ"""
    for name in STAGES:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s: %s %s against %s %s" % (name, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            return "%s: %d of %d values differ" % (name, int((a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)).sum()), a.size)
    return ""


# ---- mesh checks ------------------------------------------------------------------------------------------------------------------

def edge_use(faces):
    """(directed edges used more than once, undirected edges not used exactly twice, Euler characteristic of the used vertices)"""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = np.unique(e[:, 0] * (1 << 32) + e[:, 1], return_counts=True)[1]
    u = np.sort(e, 1)
    undirected = np.unique(u[:, 0] * (1 << 32) + u[:, 1], return_counts=True)[1]
    V = len(np.unique(f))
    return int((directed != 1).sum()), int((undirected != 2).sum()), V - len(undirected) + len(f)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- the case table ---------------------------------------------------------------------------------------------------------------

def camera(eye, target, focal, size, up=(0.0, 0.0, 1.0)):
    """a pinhole camera record at `eye` looking at `target`: x_cam = R X + t, the optical axis is +z"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    u = np.asarray(up, np.float64)
    if abs(z @ u) > 0.9:
        u = np.array([0.0, 1.0, 0.0])
    x = np.cross(u, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    cam = np.zeros((), CAMERA_DTYPE)
    cam["K"] = [focal, 0, (size - 1) / 2.0, 0, focal, (size - 1) / 2.0, 0, 0, 1]
    cam["R"] = R.reshape(-1)
    cam["t"] = -R @ eye
    cam["c"] = eye
    cam["height"] = cam["width"] = size
    return cam


def rays(cam, size):
    """camera centre and the world directions (size, size, 3) of the pixel centres, scaled to unit depth"""
    K, R, t = cam["K"].astype(np.float64).reshape(3, 3), cam["R"].astype(np.float64).reshape(3, 3), cam["t"].astype(np.float64)
    y, x = np.mgrid[0:size, 0:size]
    d = np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.ones_like(x, np.float64)], -1)
    return -R.T @ t, d @ R


def general_camera(eye, target, cols, rows, fx, fy=None, cx=None, cy=None, roll=0.0, skew=0.0, k_scale=1.0, r_scale=1.0, up=(0.0, 0.0, 1.0)):
    """camera() without its symmetries: cols x rows pixels, fx, fy, cx, cy apart, rolled by `roll` radians about the optical axis, K[1] =
    skew, the whole of K times k_scale (K[8] == k_scale), R and t times r_scale (the eye stays the point that maps to 0)"""
    base = camera(eye, target, 1.0, 1, up)["R"].astype(np.float64).reshape(3, 3)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * base[0] + s * base[1], -s * base[0] + c * base[1], base[2]]) * r_scale
    cam = np.zeros((), CAMERA_DTYPE)
    fy = fx if fy is None else fy
    cx = (cols - 1) / 2.0 if cx is None else cx
    cy = (rows - 1) / 2.0 if cy is None else cy
    cam["K"] = np.array([fx, skew, cx, 0, fy, cy, 0, 0, 1], np.float64) * k_scale
    cam["R"] = R.reshape(-1)
    cam["t"] = -R @ np.asarray(eye, np.float64)
    cam["c"] = eye
    cam["height"], cam["width"] = rows, cols
    return cam


def general_rays(cam, cols, rows):
    """the point that maps to 0 and the world directions (rows, cols, 3) of the pixel centres from K^-1 and R^-1, scaled so that the
    parameter along a ray is the depth project() reports (K's last row times R X + t)"""
    K, R, t = cam["K"].astype(np.float64).reshape(3, 3), cam["R"].astype(np.float64).reshape(3, 3), cam["t"].astype(np.float64)
    y, x = np.mgrid[0:rows, 0:cols]
    pixel = np.stack([x, y, np.ones_like(x)], -1).astype(np.float64)
    Ri = np.linalg.inv(R)
    return -Ri @ t, pixel @ np.linalg.inv(K).T @ Ri.T


def _rays(cam, size):
    """size: an int (the square, symmetric cameras of camera()) or (cols, rows)"""
    return rays(cam, size) if np.isscalar(size) else general_rays(cam, *size)


def paint(depth):
    """a b g r picture that differs from pixel to pixel"""
    H, W = depth.shape
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 5) % 256, (y * 7 + 30) % 256, (x * 3 + y * 11) % 256], -1).astype(np.uint8)


def view_of_sphere(cam, size, centre, radius, max_incidence=90.0):
    """the sphere's depth map; the mask leaves out the pixels whose ray meets the surface at more than max_incidence degrees from its
    normal, as a consistency mask leaves out grazing pixels"""
    o, d = _rays(cam, size)
    oc = o - np.asarray(centre, np.float64)
    a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - radius * radius
    disc = b * b - 4 * a * c
    z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 0.0)   # d has unit depth: the parameter is the depth
    depth = np.where(z > 0, z, 0).astype(np.float32)
    normal = (oc + z[..., None] * d) / radius
    cos = -(normal * d).sum(-1) / np.sqrt(a)
    mask = (depth > 0) & (cos >= np.cos(np.radians(max_incidence)))
    return cam, depth, mask.astype(np.uint8), paint(depth)


def view_of_plane(cam, size, point, normal, within=None):
    """the plane's depth map; within = (lo, hi): only the pixels whose ray meets the plane inside that world box are masked"""
    o, d = _rays(cam, size)
    n = np.asarray(normal, np.float64)
    den = d @ n
    z = np.where(np.abs(den) > 1e-9, ((np.asarray(point, np.float64) - o) @ n) / np.where(np.abs(den) > 1e-9, den, 1), 0.0)
    depth = np.where(z > 0, z, 0).astype(np.float32)
    mask = depth > 0
    if within is not None:
        hit = o + z[..., None] * d
        mask &= np.all((hit >= np.asarray(within[0], np.float64) - 1e-9) & (hit <= np.asarray(within[1], np.float64) + 1e-9), -1)
    return cam, depth, mask.astype(np.uint8), paint(depth)


SIX = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def sphere_views(centre, s, size=48, distance=400.0, count=6, max_incidence=90.0):
    """`count` cameras on the axes, `distance` voxels away from a sphere of radius 6 s that fills three quarters of each picture"""
    centre = np.asarray(centre, np.float64)
    radius = 6.0 * s
    focal = 0.375 * size * distance / 6.0
    dirs = [SIX[k % 6] for k in range(count)]
    out = []
    for k, dr in enumerate(dirs):
        eye = centre + np.asarray(dr, np.float64) * s * (distance + 2.0 * (k // 6))
        out.append(view_of_sphere(camera(eye, centre, focal, size), size, centre, radius, max_incidence))
    return out


def plane_view(s, size, height, focal=None, eye=(0.0, 0.0, 0.0)):
    """one camera at `eye` looking along +z at the plane z = height"""
    eye = np.asarray(eye, np.float64)
    cam = camera(eye, eye + [0, 0, 1], focal or 1.2 * size, size, up=(0.0, 1.0, 0.0))
    return view_of_plane(cam, size, [0, 0, height], [0, 0, 1])


def block_count_views(n, s):
    """views whose band stays inside n blocks in a row along x: one pixel each, looking along +z from below the row's middle layer"""
    out = []
    for k in range(n):
        eye = np.array([(8 * k + 3.5) * s, 3.5 * s, -20.0 * s])
        cam = camera(eye, eye + [0, 0, 1], 10.0, 1, up=(0.0, 1.0, 0.0))
        depth = np.full((1, 1), np.float32(23.5 * s), np.float32)
        out.append((cam, depth, np.ones((1, 1), np.uint8), np.full((1, 1, 3), 200, np.uint8)))
    return out


OBLIQUE = (40, 28)


def oblique_views(centre, s, variants=()):
    """five 40 x 28 views of a sphere of 6 voxels along seeded random directions, 60 to 140 voxels away, rolled by 0.4 k, fy = 1.3 fx,
    the principal point at (0.37 W, 0.61 H), aimed up to 3 voxels off the centre so that the border cuts the sphere.  variants: view
    number -> "skew" (K[1] = 0.05 fx), "k2" (K times 2) or "r" (R times 1 + 5e-4): the cameras the cull must leave alone"""
    rng = np.random.default_rng(20240607)
    centre = np.asarray(centre, np.float64)
    cols, rows = OBLIQUE
    out = []
    for k in range(5):
        direction = rng.normal(size=3)
        direction /= np.linalg.norm(direction)
        distance = rng.uniform(60.0, 140.0)
        aim = rng.normal(size=3)
        aim *= rng.uniform(1.0, 3.0) / np.linalg.norm(aim)
        fx = 2.0 * distance                                                        # the sphere is 12 pixels wide and 15.6 high
        kind = dict(variants).get(k)
        cam = general_camera(centre + direction * distance * s, centre + aim * s, cols, rows, fx, 1.3 * fx, 0.37 * cols, 0.61 * rows, roll=0.4 * k,
                             skew=0.05 * fx if kind == "skew" else 0.0, k_scale=2.0 if kind == "k2" else 1.0, r_scale=1.0 + 5e-4 if kind == "r" else 1.0)
        out.append(view_of_sphere(cam, OBLIQUE, centre, 6.0 * s))
    return out


UNCULLABLE = {1: "skew", 2: "k2", 3: "r"}
WIDE = dict(height=160.3, eye=(0.0, 200.0, 0.0))      # (voxels) the wide plane z = 160.3 under a camera at `eye` looking along +z


def wide_plane(s, size, half):
    """a size x size view whose pixels spread over +-half voxels of the plane: (2 ceil(half * 1.025 / 8))^2 columns of two blocks each"""
    eye = np.asarray(WIDE["eye"]) * s
    return plane_view(s, size, WIDE["height"] * s, focal=WIDE["height"] * (size - 1) / (2.0 * half), eye=eye)


def cull_faces_views(s):
    """the 96 x 96 wide plane and three views whose frusta pass through its blocks (voxel coordinates below, relative to the plane's middle):
    1  20 x 12, rolled, off-centre, 40 voxels in front of the plane: it sees a middle part, blocks lie beyond all four sides;
    2  32 x 20 from inside the slab of blocks, looking along it at a grazing angle: blocks behind it, across z = 0 and in front;
    3  16 x 16 looking at a patch 30 voxels away that hides the plane: the plane's blocks lie beyond depth_max + tau in its frustum"""
    mid = np.array([WIDE["eye"][0], WIDE["eye"][1], WIDE["height"]])
    at = lambda *v: (mid + np.asarray(v, np.float64)) * s
    box = (at(-54, -54, -1), at(54, 54, 1))
    plane = ([0, 0, WIDE["height"] * s], [0, 0, 1])
    close = general_camera(at(5, -3, -40), at(8, 4, 0), 20, 12, 20.0, 26.0, 0.37 * 20, 0.61 * 12, roll=0.5, up=(0.0, 1.0, 0.0))
    along = general_camera(at(-20, 3, -4.3), at(30, 5, 0), 32, 20, 24.0, 24.0 * 1.3, 0.37 * 32, 0.61 * 20, roll=0.2)
    hidden = general_camera(at(10, -10, -60), at(10, -10, 0), 16, 16, 14.0, 14.0 * 1.3, 0.37 * 16, 0.61 * 16, roll=0.3, up=(0.0, 1.0, 0.0))
    return [wide_plane(s, 96, 54.0), view_of_plane(close, (20, 12), *plane, within=box), view_of_plane(along, (32, 20), *plane, within=box),
            view_of_plane(hidden, (16, 16), at(0, 0, -30), [0, 0, 1])]


def cases():
    """name -> dict(views, s, tau, min_weight, closed, table, centre).  The closed spheres are centred on lattice points: six views
    along the axes see the directions (+-1, +-1, +-1) at 54.7 degrees at best, and a cell there whose outer corner lies 1.7 voxels
    outside the surface has no masked pixel behind that corner unless the lattice is as symmetric as the cameras (an open mesh is
    then the definition's answer, not a fault: a corner without a view makes its cells inactive)."""
    s = 0.05
    C = {}
    add = lambda name, views, tau=4 * s, mw=1, closed=False, table=None, vs=s: C.__setitem__(name, dict(views=views, s=vs, tau=tau, min_weight=mw, closed=closed, table=table))
    off = (20 * s, -40 * s, 10 * s)
    add("sphere", sphere_views(off, s), closed=True)
    C["sphere"]["centre"] = off
    add("sphere_at_origin", sphere_views((0.0, 0.0, 0.0), s), closed=True)
    C["sphere_at_origin"]["centre"] = (0.0, 0.0, 0.0)
    add("plane_one_view", [plane_view(s, 24, 10.3 * s)])
    add("plane_on_layer", [plane_view(0.0625, 24, 0.625)], tau=0.25, vs=0.0625)          # depth 0.625 = layer 10 exactly: F == 0 there
    near, far = plane_view(s, 24, 10.3 * s), plane_view(s, 24, 20.3 * s)
    add("two_views_disagree", [near, far])
    behind = plane_view(s, 24, 10.3 * s)
    add("behind_a_camera", [behind, plane_view(s, 24, 16.0 * s, eye=(0.0, 0.0, 8.0 * s))])
    cam, depth, mask, bgr = plane_view(s, 24, 10.3 * s)
    depth, mask = depth.copy(), mask.copy()
    depth[::3, ::2] = 0
    depth[5, 5] = -1.0
    mask[:, 12:] = 0
    add("zero_depths_half_mask", [(cam, depth, mask, bgr)])
    for n in (1, 63, 64, 65):
        add("blocks_%d" % n, block_count_views(n, s), tau=s)
    add("nothing_masked", [(cam, depth, np.zeros_like(mask), bgr)])
    add("table_regrows", sphere_views(off, s), closed=True, table=4)
    C["table_regrows"]["centre"] = off
    add("min_weight_above_views", sphere_views(off, s), mw=7)
    add("views_33", sphere_views(off, s, size=24, count=33), mw=2)
    add("oblique_sphere", oblique_views(off, s))
    C["oblique_sphere"]["centre"] = off
    add("uncullable_views", oblique_views(off, s, UNCULLABLE))
    add("cull_faces", cull_faces_views(s))
    wide = wide_plane(s, 96, 54.0)                                                 # 14 x 14 x 2 = 392 blocks
    for n in (511, 512, 513):
        add("blocks_%d" % n, [wide] + block_count_views(n - 392, s), tau=s)
    add("blocks_968", [wide_plane(s, 128, 84.0)])                                  # 22 x 22 x 2
    return C
