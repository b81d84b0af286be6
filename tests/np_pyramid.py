"""Numpy model of a pyramid level's float image, written from host/APD.cpp load_image and host/io.cpp ResizeLinear: the decoded
bytes at the origin of a zero canvas of the reference's size (cropped beyond it), the canvas as float, cv::resize(INTER_LINEAR) to
the level size.  Vectorised; every binary32 operation of the C++ is one float32 numpy operation (one rounding, nothing fused), the
source coordinate is formed in float64.  Besides the model: the cases the CPU and GPU tests share, the serial host build of
csrc/dvp_pyramid.hpp (tests/pyramid_host) and the host mirror (tests/host/test_host --resize)."""
import ctypes
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = os.path.join(ROOT, "tests", "pyramid_host", "libdvp_pyramid_host.so")
f32 = np.float32

# (source (w, h), pad (w, h) or None = the image's own size, levels [(w, h), ...], pitch or None)
CASES = [
    ((67, 35), None, [(67, 35)], 80),                   # identity, rows wider than the image
    ((96, 64), None, [(48, 32), (24, 16)], None),       # exact halves / quarters
    ((838, 126), None, [(105, 16)], None),              # eighths
    ((123, 77), None, [(62, 39)], None),                # half-away rounding, inexact fractions
    ((40, 1082), None, [(10, 271)], None),
    ((129, 9), None, [(65, 5)], None),                  # one pixel past a wave
    ((40, 30), None, [(100, 70)], None),                # up-sampling: both clamps fire
    ((1, 1), None, [(3, 2)], None),
    ((72, 48), (96, 64), [(48, 32), (96, 64)], None),   # zero padding, a tap straddling the image's edge
    ((120, 80), (96, 64), [(48, 32)], None),            # crop
    ((120, 48), (96, 64), [(48, 32)], None),            # crop in x, padding in y
    ((71, 47), (96, 64), [(48, 32)], None),             # odd image in the canvas: taps 70 | 71 and 46 | 47 blend the last column / row with the padding
]
# one entry per level
LEVELS = [(k, lv) for k, c in enumerate(CASES) for lv in c[2]]


def level_id(item):
    k, (lw, lh) = item
    (sw, sh), pad, _, _ = CASES[k]
    return "%dx%d%s-%dx%d" % (sw, sh, "-pad%dx%d" % pad if pad else "", lw, lh)


@functools.lru_cache(None)
def image(k):
    """random bytes of case k, 255 and 0 both present (the 1 x 1 image is 255); read-only, with the case's pitch"""
    (sw, sh), _, _, pitch = CASES[k]
    rng = np.random.default_rng(1000 + k)
    wide = rng.integers(0, 256, (sh, pitch or sw), dtype=np.uint8)
    a = wide[:, :sw]
    a[0, 0] = 255
    if a.size > 1:
        a[-1, -1] = 0
    wide.setflags(write=False)
    a.setflags(write=False)
    return a


def pad_of(k):
    return CASES[k][1] or CASES[k][0]


def canvas(img, pad_w, pad_h):
    """load_image: Mat::zeros(pad_h, pad_w) with the image's rows and columns that fit, as float"""
    c = np.zeros((pad_h, pad_w), np.float32)
    h, w = min(pad_h, img.shape[0]), min(pad_w, img.shape[1])
    c[:h, :w] = img[:h, :w]
    return c


def taps(n_src, n_dst):
    """ResizeLinear's first tap, second tap and fraction of every destination index"""
    scale = float(n_src) / float(n_dst)                                   # (double)src / dst
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(np.float32)                                          # float - (float)int, in float
    low, high = i < 0, i >= n_src - 1
    i = np.where(low, 0, i)
    i = np.where(high, n_src - 1, i)
    f = np.where(low | high, f32(0), f).astype(np.float32)
    return i, np.minimum(i + 1, n_src - 1), f


def _blend(p, q, a):
    """p * (1.f - a) + q * a: four float32 operations"""
    assert p.dtype == q.dtype == a.dtype == np.float32
    return p * (f32(1) - a) + q * a


def resize_linear(src, new_cols, new_rows):
    src = np.ascontiguousarray(src, np.float32)
    x0, x1, ax = taps(src.shape[1], new_cols)
    y0, y1, ay = taps(src.shape[0], new_rows)
    h0 = _blend(src[y0][:, x0], src[y0][:, x1], ax[None, :])
    h1 = _blend(src[y1][:, x0], src[y1][:, x1], ax[None, :])
    out = _blend(h0, h1, ay[:, None])
    assert out.dtype == np.float32
    return out


def level(img, lw, lh, pad_w=0, pad_h=0):
    """the (lh, lw) float32 level of a uint8 image on a pad_w x pad_h canvas (0: the image's own size).  ResizeLinear runs at
    equal sizes too, where load_image skips it: the fractions are zero and the result is the canvas (the tests check that)."""
    if not pad_w:
        pad_h, pad_w = img.shape
    return resize_linear(canvas(img, pad_w, pad_h), lw, lh)


@functools.lru_cache(None)
def expected(item):
    k, (lw, lh) = item
    out = level(image(k), lw, lh, *pad_of(k))
    out.setflags(write=False)
    return out


def round_half_away(n, scale):
    """the driver's level size: (int)std::round(n * factor) with float factor = 1.f / scale"""
    return int(np.floor(float(f32(n) * (f32(1.0) / f32(scale))) + 0.5))


# ---- the serial host build of csrc/dvp_pyramid.hpp
@functools.lru_cache(None)
def host_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(_LIB)])
    L = ctypes.CDLL(_LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.dvp_pyramid_level_serial.argtypes = [vp, ctypes.c_longlong, ci, ci, ci, ci, ci, ci, vp]
    return L


def serial(img, lw, lh, pad_w=0, pad_h=0):
    """(rc, level) of the kernel's text run on the host, one texel after the other"""
    assert img.dtype == np.uint8 and img.strides[1] == 1
    if not pad_w:
        pad_h, pad_w = img.shape
    out = np.zeros((max(lh, 1), max(lw, 1)), np.float32)
    rc = host_lib().dvp_pyramid_level_serial(img.ctypes.data, img.strides[0], img.shape[1], img.shape[0], pad_w, pad_h, lw, lh, out.ctypes.data)
    return rc, out


# ---- the host mirror: host/io.cpp ResizeLinear through tests/host/test_host --resize
def mirror_resize(tmp_path, src_f32, new_cols, new_rows):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host")])
    src, out = os.path.join(str(tmp_path), "src.dmb"), os.path.join(str(tmp_path), "out.dmb")
    a = np.ascontiguousarray(src_f32, np.float32)
    with open(src, "wb") as f:
        f.write(np.array([1, a.shape[0], a.shape[1], 5], np.int32).tobytes())
        f.write(a.tobytes())
    r = subprocess.run([os.path.join(ROOT, "tests", "host", "test_host"), "--resize", src, str(new_cols), str(new_rows), out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    _, rows, cols, typ = np.frombuffer(raw[:16], np.int32)
    assert int(typ) == 5
    return np.frombuffer(raw[16:], np.float32).reshape(rows, cols)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and bool((a.view(np.uint32) == b.view(np.uint32)).all())
