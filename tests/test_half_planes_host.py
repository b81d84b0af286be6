"""Format 2 of the image planes (binary16 tiles, Dev::images16) on the host: the device headers' addressing, decoding and upload
rule built with g++ (tests/half16), against the float row-pair planes.  Quarter-level images — multiples of 0.25 in [0, 255], what
a power-of-two down-sampling of 8-bit images gives — must sample to the float planes' texels bit for bit, with both samplers and
at coordinates on and beyond the border (clamp-to-edge) and NaN."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.hostbox

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "half16")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-s", "-C", _HERE])
        L = ctypes.CDLL(os.path.join(_HERE, "libhalf16.so"))
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
        L.h16_rule.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_uint32)]
        L.h16_rule.restype = ctypes.c_uint
        L.h16_decode.argtypes = [ctypes.c_uint32]
        L.h16_decode.restype = ctypes.c_float
        L.h16_footprints.argtypes = [fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, fp, fp, ctypes.c_int]
        L.h16_ref_texels.argtypes = [fp, ctypes.c_int, ctypes.c_int, ip, ip, ctypes.c_int]
        L.h16_offsets.argtypes = [ctypes.c_int, ctypes.c_int]
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _quarter_image(W, H, rng):
    return (rng.integers(0, 1021, (H, W)).astype(np.float32) * np.float32(0.25)).astype(np.float32)


def _coords(W, H, rng, n):
    xs = rng.uniform(-3.0, W + 2.0, n).astype(np.float32)
    ys = rng.uniform(-3.0, H + 2.0, n).astype(np.float32)
    # the clamp corners: -1, W, H exactly, just inside / outside them, and NaN in either coordinate
    edge_x = np.array([-1.0, W, W - 1.0, W - 0.5, -0.999, W + 0.25, np.nan, 0.0, np.nan], np.float32)
    edge_y = np.array([-1.0, H, H - 1.0, H - 0.5, H + 7.0, -0.25, 3.5, np.nan, np.nan], np.float32)
    gx, gy = np.meshgrid(edge_x, edge_y)
    return np.concatenate([xs, gx.ravel(), edge_x]), np.concatenate([ys, gy.ravel(), np.full(len(edge_x), H, np.float32)])


@pytest.mark.parametrize("sampler", [0, 1])
@pytest.mark.parametrize("W,H", [(37, 23), (64, 41), (131, 67)])
def test_footprints_equal_the_float_planes(W, H, sampler):
    rng = np.random.default_rng(W * 7 + H + sampler)
    img = _quarter_image(W, H, rng)
    assert set(np.unique(img % 1.0)) == {0.0, 0.25, 0.5, 0.75}
    xs, ys = _coords(W, H, rng, 20000)
    xs, ys = np.ascontiguousarray(xs, np.float32), np.ascontiguousarray(ys, np.float32)
    assert lib().h16_footprints(_p(img, ctypes.c_float), W, H, sampler, _p(xs, ctypes.c_float), _p(ys, ctypes.c_float), len(xs)) == 0


@pytest.mark.parametrize("W,H", [(37, 23), (131, 67)])
def test_reference_texels_equal_the_float_planes(W, H):
    rng = np.random.default_rng(W + H)
    img = _quarter_image(W, H, rng)
    yy, xx = np.mgrid[-3:H + 3, -3:W + 3]
    xs, ys = np.ascontiguousarray(xx.ravel(), np.int32), np.ascontiguousarray(yy.ravel(), np.int32)
    assert lib().h16_ref_texels(_p(img, ctypes.c_float), W, H, _p(xs, ctypes.c_int), _p(ys, ctypes.c_int), len(xs)) == 0


@pytest.mark.parametrize("W", [37, 38, 39, 40, 41, 42, 43])
@pytest.mark.parametrize("H", [23, 24, 25, 26, 27, 28, 29, 30])
def test_tile_addressing_on_distinct_texels(W, H):
    """img16_offset against the float planes' addressing at every footprint origin of the padded plane, on a plane whose texels all
    differ (the frame included, where a replicated border would hide a clamp one row or column off); widths cover every residue of
    (W + 4) mod 7, heights every residue of (H + 4) mod 8"""
    assert lib().h16_offsets(W, H) == 0


def _rule(a, b=0.0):
    h = ctypes.c_uint32(0)
    bits = lib().h16_rule(ctypes.c_float(a), ctypes.c_float(b), ctypes.byref(h))
    return bits, h.value


@pytest.mark.parametrize("v", [0.125, 254.75, 255.0, 0.25, 127.5, 2.0 ** -24, 3.0 * 2.0 ** -20, 1.0 / 1024, 0.0, -0.0, 100.125])
def test_rule_accepts_binary16_values_in_range(v):
    bits, h = _rule(v, 3.0)
    assert bits & 2 == 0
    assert bits & 1 == (0 if float(v) == np.floor(v) else 1)
    lo, hi = np.array([h & 0xFFFF, h >> 16], np.uint16).view(np.float16).astype(np.float32)
    assert np.float32(lo).tobytes() == np.float32(v).tobytes() and hi == 3.0
    assert np.float32(lib().h16_decode(h & 0xFFFF)).tobytes() == np.float32(v).tobytes()


@pytest.mark.parametrize("v", [255.25, 300.0, -0.25, float("nan"), 100.1, float("inf"), 2.0 ** -25, 1e-40, 255.5, 65504.0])
def test_rule_refuses_other_values(v):
    assert _rule(v)[0] & 3 == 3
    assert _rule(0.5, v)[0] & 3 == 3


def test_rule_integer_sets_stay_format_1():
    for v in (0.0, 1.0, 17.0, 128.0, 255.0):
        assert _rule(v, 255.0 - v)[0] == 0


def test_decoder_equals_numpy_on_every_binary16_value():
    h = np.arange(0x10000, dtype=np.uint32)
    ref = h.astype(np.uint16).view(np.float16).astype(np.float32)
    got = np.array([lib().h16_decode(int(x)) for x in h], np.float32)
    fin = ~np.isnan(ref)
    assert (got[fin].view(np.uint32) == ref[fin].view(np.uint32)).all()
    assert np.isnan(got[~fin]).all()
