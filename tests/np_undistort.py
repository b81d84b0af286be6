"""An independent numpy reading of what `apd --convert-from ... --undistort on` computes (csrc/dvp_undistort.hpp, host/colmap.cpp),
written from the stage's definition, not from the header: whole-picture array arithmetic with np.arctan, the
fixed-point bilinear rule on a zero-padded copy of the picture.  Also the cases the tests share, the pixels at which a last-bit
difference in a coordinate may move a byte ("fragile"), and the glue that runs tests/undistort_host/undistort_host (the project's
text, serially, on the host)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "undistort_host", "undistort_host")

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5, "FULL_OPENCV": 6, "FOV": 7,
             "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}
SINGLE_F = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
FISHEYE = ("SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "OPENCV_FISHEYE", "THIN_PRISM_FISHEYE")
OPENCV_EXTRA = [-0.2, 0.05, 0.004, -0.003]
# the distortion parameters of the ten accepted models (what follows cx, cy)
EXTRA = {
    "SIMPLE_PINHOLE": [], "PINHOLE": [],
    "SIMPLE_RADIAL": [-0.12], "RADIAL": [0.15, -0.03], "OPENCV": OPENCV_EXTRA, "FULL_OPENCV": OPENCV_EXTRA + [0.01, 0.02, -0.01, 0.005],
    "SIMPLE_RADIAL_FISHEYE": [0.05], "RADIAL_FISHEYE": [-0.04, 0.01], "OPENCV_FISHEYE": [-0.03, 0.01, -0.004, 0.001],
    "THIN_PRISM_FISHEYE": [-0.05, 0.02, 0.002, -0.001, -0.005, 0.001, 0.003, -0.002],
}
MODELS = list(EXTRA)
NOT_FISHEYE = [m for m in MODELS if m not in FISHEYE]
HOST_SIZES = [(1, 1), (3, 2), (67, 5), (300, 7), (129, 66)]
# one below, at and past a wave and a work-group of the device form
GPU_SIZES = [(1, 1), (3, 2), (63, 3), (64, 3), (65, 3), (67, 5), (257, 4), (129, 66)]


def intrinsics(w, h):
    f = 0.6 * max(w, h) + 0.3
    return f, 1.01 * f, w / 2 + 0.37, h / 2 - 0.21


def params(model, w, h, extra=None):
    """the camera's parameters in COLMAP's order"""
    fx, fy, cx, cy = intrinsics(w, h)
    head = [fx, cx, cy] if model in SINGLE_F else [fx, fy, cx, cy]
    return np.array(head + list(EXTRA[model] if extra is None else extra), np.float64)


def split(model, p):
    p = [float(v) for v in p]
    return (p[0], p[0], p[1], p[2], p[3:]) if model in SINGLE_F else (p[0], p[1], p[2], p[3], p[4:])


def distort(model, k, u, v):
    if model in FISHEYE:
        r = np.sqrt(u * u + v * v)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(r > 0, np.arctan(r) / r, 1.0)
        u, v = u * s, v * s
    r2 = u * u + v * v
    if model in ("SIMPLE_PINHOLE", "PINHOLE"):
        return u, v
    if model in ("SIMPLE_RADIAL", "SIMPLE_RADIAL_FISHEYE"):
        f = 1 + k[0] * r2
        return u * f, v * f
    if model in ("RADIAL", "RADIAL_FISHEYE"):
        f = 1 + k[0] * r2 + k[1] * r2 ** 2
        return u * f, v * f
    if model == "OPENCV_FISHEYE":
        f = 1 + k[0] * r2 + k[1] * r2 ** 2 + k[2] * r2 ** 3 + k[3] * r2 ** 4
        return u * f, v * f
    if model in ("OPENCV", "FULL_OPENCV"):
        k1, k2, p1, p2 = k[:4]
        rad = 1 + k1 * r2 + k2 * r2 ** 2
        if model == "FULL_OPENCV":
            k3, k4, k5, k6 = k[4:8]
            rad = (rad + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        return u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u), v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)
    if model == "THIN_PRISM_FISHEYE":
        k1, k2, p1, p2, k3, k4, sx1, sy1 = k[:8]
        rad = k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3 + k4 * r2 ** 4
        return (u + u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u) + sx1 * r2,
                v + v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v) + sy1 * r2)
    raise ValueError(model)


def source_coordinates(model, p, w, h):
    """(sx, sy), each (h, w) float64: where output pixel (x, y) looks in the picture as taken"""
    fx, fy, cx, cy, k = split(model, p)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u, v = (x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy
    du, dv = distort(model, k, u, v)
    return fx * du + cx - 0.5, fy * dv + cy - 0.5


def fragile(sx, sy, margin=1e-6):
    """pixels where 32 s + 0.5 of either axis lies within `margin` of an integer: a last-bit difference may move the 1/32-pixel step"""
    def near(s):
        t = 32 * s + 0.5
        return np.abs(t - np.rint(t)) <= margin
    return near(sx) | near(sy)


def undistort(bgr, model, p):
    """(the (h, w, 3) uint8 picture by the fixed-point rule, the fragile mask)"""
    h, w = bgr.shape[:2]
    sx, sy = source_coordinates(model, p, w, h)
    nan = np.isnan(sx) | np.isnan(sy)
    qx = np.clip(np.floor(32 * np.where(nan, 0, sx) + 0.5), -64, 32 * w + 64).astype(np.int64)
    qy = np.clip(np.floor(32 * np.where(nan, 0, sy) + 0.5), -64, 32 * h + 64).astype(np.int64)
    ix, a, iy, b = qx >> 5, qx & 31, qy >> 5, qy & 31
    pad = 4                                                     # ix, ix + 1 lie in -2 ... w + 3
    big = np.zeros((h + 2 * pad, w + 2 * pad, 3), np.int64)
    big[pad:pad + h, pad:pad + w] = bgr
    a, b = a[:, :, None], b[:, :, None]
    out = ((32 - a) * (32 - b) * big[iy + pad, ix + pad] + a * (32 - b) * big[iy + pad, ix + pad + 1] + (32 - a) * b * big[iy + pad + 1, ix + pad] +
           a * b * big[iy + pad + 1, ix + pad + 1] + 512) >> 10
    out[nan] = 0
    return out.astype(np.uint8), fragile(sx, sy)


def picture(w, h, seed=0):
    return np.random.default_rng(7000 * w + h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def padded(bgr, extra=9):
    """the same picture with `extra` more bytes in every row (a view: strides[0] = 3 w + extra)"""
    h, w = bgr.shape[:2]
    flat = np.zeros((h, 3 * w + extra), np.uint8)
    flat[:, :3 * w] = bgr.reshape(h, 3 * w)
    flat[:, 3 * w:] = 0xA5
    return np.lib.stride_tricks.as_strided(flat, (h, w, 3), (3 * w + extra, 3, 1))


def ramp(w, h, alpha, beta, c):
    """rint(alpha x + beta y + c) in all three channels"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    g = np.rint(alpha * x + beta * y + c)
    assert g.min() >= 0 and g.max() < 255
    return np.repeat(g.astype(np.uint8)[:, :, None], 3, 2)


def project(q, t, xyz, fx, fy, cx, cy, F):
    """sfm columns with --undistort on: ((fx Xc / Zc + cx) / F, (fy Yc / Zc + cy) / F, Zc) with (Xc, Yc, Zc) = R X + t, term by term"""
    import np_convert
    R = np_convert.rotation(q)
    X = [float(v) for v in xyz]
    xc, yc, zc = (R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r] for r in range(3))
    return (fx * xc / zc + cx) / F, (fy * yc / zc + cy) / F, zc


# ---- the project's text on the host -------------------------------------------------------------------------------------------
def run_program(*args):
    return subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def serial_atan(x, tmp):
    src, dst = os.path.join(str(tmp), "atan.in"), os.path.join(str(tmp), "atan.out")
    np.ascontiguousarray(x, np.float64).tofile(src)
    out = run_program("atan", src, dst)
    assert out.returncode == 0, out.stderr
    return np.fromfile(dst, np.float64)


def serial_image(bgr, model, p, tmp, num_params=None, size=None, pitch=None, null=()):
    """(return code, stderr, (h, w, 3) uint8 or None) of undistort_host image; model: a name or an id; `size`, `pitch`,
    `num_params` override what the arrays say, `null` names the pointers to withhold ("in", "params", "out")"""
    h, w = bgr.shape[:2]
    src, par, dst = (os.path.join(str(tmp), n) for n in ("und.in", "und.params", "und.out"))
    rows = np.zeros((h, bgr.strides[0]), np.uint8)
    rows[:, :3 * w] = np.asarray(bgr).reshape(h, 3 * w)
    rows.tofile(src)
    p = np.ascontiguousarray(p, np.float64)
    p.tofile(par)
    W, H = size if size else (w, h)
    out = run_program("image", W, H, bgr.strides[0] if pitch is None else pitch, MODEL_IDS.get(model, model), p.size if num_params is None else num_params,
                      "-" if "in" in null else src, "-" if "params" in null else par, "-" if "out" in null else dst)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    return 0, out.stderr, np.fromfile(dst, np.uint8).reshape(H, W, 3)


_SERIAL = {}


def serial_case(model, w, h, tmp_factory, pad=False, extra=None):
    """the serial program's picture for a shared case, made once"""
    key = (model, w, h, pad, None if extra is None else tuple(extra))
    if key not in _SERIAL:
        src = picture(w, h)
        rc, err, got = serial_image(padded(src) if pad else src, model, params(model, w, h, extra), tmp_factory.mktemp("serial"))
        assert rc == 0, err
        got.setflags(write=False)
        _SERIAL[key] = got
    return _SERIAL[key]
