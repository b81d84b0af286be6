"""Preview renderers and the JPEG encoder's arithmetic without a GPU: np_preview (numpy reading of APD.cpp:694-812) against
the renderers the device runs (csrc/dvp_jpeg.hpp, built for the host in tests/jpeg_host), on the cases that decide bits; and
the encoder's steps, run serially on the host, against libjpeg-turbo (Pillow) byte for byte."""
import ctypes
import os

import numpy as np
import pytest

import np_preview as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = os.path.join(ROOT, "tests", "jpeg_host", "libdvp_jpeg_host.so")


def host_lib():
    if not os.path.exists(_LIB):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(_LIB)])
    L = ctypes.CDLL(_LIB)
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    L.dvp_jpeg_encode_host.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ll, ctypes.c_int, ctypes.c_int, vp, ll, ctypes.POINTER(ll)]
    L.dvp_preview_render_host.argtypes = [vp, vp, ll, ctypes.c_float, ctypes.c_float, vp, vp, vp]
    return L


def render_host(planes, weak, dmin, dmax):
    L = host_lib()
    planes = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
    weak = np.ascontiguousarray(weak, np.uint8)
    n = len(planes)
    out = [np.zeros((n, 3), np.uint8) for _ in range(3)]
    L.dvp_preview_render_host(planes.ctypes.data, weak.ctypes.data, n, dmin, dmax, *[o.ctypes.data for o in out])
    return out


def encode_host(img, quality, restart):
    L = host_lib()
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else 3
    cap = 4096 + H * W * 8
    dst = np.empty(cap, np.uint8)
    n = ctypes.c_longlong(0)
    assert L.dvp_jpeg_encode_host(img.ctypes.data, W, H, C, img.strides[0], quality, restart, dst.ctypes.data, cap, ctypes.byref(n)) == 0
    return dst[:n.value].tobytes()


def band_depths(dmin, dmax):
    """depths whose pv = (dmax - d) / (dmax - dmin) * 255 lands on and around the band edges 51, 102, 153, 204, 255"""
    dmin, dmax = np.float32(dmin), np.float32(dmax)
    out = []
    for edge in (0, 51, 102, 153, 204, 255, 25.5, 76.5, 127.5, 178.5, 229.5):
        d = np.float32(dmax - np.float32(edge / 255.0) * (dmax - dmin))
        for k in range(-3, 4):
            out.append(np.nextafter(d, np.float32(np.inf) if k > 0 else np.float32(-np.inf)) if k else d)
            for _ in range(abs(k) - 1):
                out[-1] = np.nextafter(out[-1], np.float32(np.inf) if k > 0 else np.float32(-np.inf))
    out += [dmin, dmax, np.nextafter(dmin, np.float32(-1)), np.nextafter(dmax, np.float32(100)), np.float32(np.nan), np.float32(np.inf),
            np.float32(-np.inf), np.float32(0)]
    return np.array(out, np.float32)


def crafted_state(dmin, dmax, rs):
    """planes + weak map holding every case of the renderers: band edges, range ends, NaN / inf depths, zero / NaN /
    unnormalised normals, weak values 0..3"""
    d = band_depths(dmin, dmax)
    d = np.concatenate([d, rs.uniform(dmin - 1, dmax + 1, 400).astype(np.float32)])
    n = len(d)
    normal = rs.normal(size=(n, 3)).astype(np.float32) * rs.choice([1e-3, 1, 7, 1e4], size=(n, 1)).astype(np.float32)
    normal[:8] = [[0, 0, 0], [np.nan, 0, 0], [0, np.nan, 1], [1, 0, 0], [0, -1, 0], [3, 4, 0], [np.inf, 0, 0], [-0.0, 0, 0]]
    normal[8] = [0.6, 0.8, 0]                 # norm 1 in double, rounding at 127.5 multiples
    planes = np.concatenate([normal, d[:, None]], 1).astype(np.float32)
    weak = (np.arange(n) % 4).astype(np.uint8)
    return planes, weak


@pytest.mark.hostbox
@pytest.mark.parametrize("dmin,dmax", [(1.5, 7.8), (-2.0, 3.0), (0.0, 1.0), (2.0, 2.0)])
def test_renderers_match_numpy_reading(dmin, dmax):
    planes, weak = crafted_state(dmin, dmax, np.random.RandomState(int(dmax * 10)))
    ref = P.previews(planes, weak, dmin, dmax, 1, len(planes))
    got = render_host(planes, weak, dmin, dmax)
    for name, g in zip(("depth", "normal", "weak"), got):
        r = ref[name].reshape(-1, 3)
        bad = np.nonzero((g != r).any(1))[0]
        assert len(bad) == 0, (name, bad[:5], planes[bad[:5]], g[bad[:5]], r[bad[:5]])


@pytest.mark.hostbox
def test_renderer_literals():
    """values read off the reference's code by hand"""
    d = P.depth_preview(np.array([1.0, 2.0, 0.0, np.nan, np.inf, -np.inf, 3.0], np.float32), 1.0, 2.0)
    assert d[0].tolist() == [0, 0, 255]                  # pv = 255: band 5, 127 - (uchar)(51 * 127 / 51 + 0.5) = 0
    assert d[1].tolist() == [255, 0, 0]                  # pv = 0: band 1
    assert d[2:7].tolist() == [[0, 0, 0]] * 5            # out of range, NaN, +-inf
    z = P.depth_preview(np.array([0.0], np.float32), -1.0, 1.0)
    assert z[0].tolist() == [0, 255, 127]                # a kept 0 with dmin <= 0: pv = 127.5, band 3, (uchar)(25.5 * 5) = 127
    assert P.normal_preview(np.array([[0, 0, 0], [np.nan, 1, 1], [1, 0, 0]], np.float32)).tolist() == [[128, 128, 128], [0, 0, 0], [255, 128, 128]]
    assert P.weak_preview(np.array([0, 1, 2, 3], np.uint8)).tolist() == [[255, 255, 255], [0, 255, 0], [0, 0, 255], [0, 0, 0]]
    # unpack: out-of-range depths become 0 / UNKNOWN, NaN is kept
    dep, nor, st = P.unpack(np.array([[0, 0, 1, 5.0], [0, 0, 1, 9.0], [0, 0, 1, np.nan]], np.float32), [1, 0, 0], 1.0, 8.0)
    assert dep[:2].tolist() == [5.0, 0.0] and np.isnan(dep[2]) and st.tolist() == [1, 2, 0]


def images(rs, W, H, C):
    sh = (H, W) if C == 1 else (H, W, 3)
    g = np.add.outer(np.arange(H) * 3, np.arange(W) * 2) % 256
    grad = g if C == 1 else np.stack([g, 255 - g, (g * 7) % 256], -1)
    return dict(noise=rs.randint(0, 256, sh).astype(np.uint8), const=np.full(sh, 255, np.uint8), grad=grad.astype(np.uint8))


@pytest.mark.hostbox
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (16, 16), (17, 33), (1000, 3), (255, 129), (33, 18)])
@pytest.mark.parametrize("C", [1, 3])
def test_encoder_steps_match_libjpeg_turbo(W, H, C):
    rs = np.random.RandomState(W * 7 + H + C)
    for q in (50, 75, 95, 100, 1):
        for name, img in images(rs, W, H, C).items():
            for R in (1, 2, 32):
                assert encode_host(img, q, R) == P.pil_jpeg(img, q, R), (W, H, C, q, name, R)
