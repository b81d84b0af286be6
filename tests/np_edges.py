"""Shared by the edge-prior tests (test_edges_host.py, test_gpu_edges.py): the input images and three-state maps, and the
references they are held against — the host mirror's EdgeSegment through `test_host --edges`, the numpy / scipy Canny of
test_host_oracles.py with the sequential frame fix-ups, scipy's connected components for the hysteresis.  Every reference is
computed once per case and handed out read-only."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT, synth

_LIB = os.path.join(ROOT, "tests", "edges_host", "libdvp_edges_host.so")


@functools.lru_cache(None)
def host_lib():
    """the serial host build of csrc/dvp_edges.hpp"""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(_LIB)])
    L = ctypes.CDLL(_LIB)
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.dvp_edge_thresholds_host.argtypes = [ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.dvp_edge_thresholds_host.restype = None
    L.dvp_edge_median_host.argtypes = [vp, ci, ci, ll]
    L.dvp_grey_bytes_host.argtypes = [vp, ll, vp]
    L.dvp_grey_bytes_host.restype = None
    L.dvp_edge_hysteresis_host.argtypes = [vp, ci, ci, vp]
    L.dvp_canny_edge_map_host.argtypes = [vp, ci, ci, ll, vp]
    return L


def serial_canny(u8):
    """the kernels' text run serially on the host: (rc, map)"""
    u8 = np.ascontiguousarray(u8, np.uint8)
    H, W = u8.shape
    out = np.zeros((H, W), np.uint8)
    rc = host_lib().dvp_canny_edge_map_host(u8.ctypes.data, W, H, u8.strides[0], out.ctypes.data)
    return rc, out


def serial_hysteresis(map3):
    map3 = np.ascontiguousarray(map3, np.uint8)
    H, W = map3.shape
    out = np.zeros((H, W), np.uint8)
    assert host_lib().dvp_edge_hysteresis_host(map3.ctypes.data, W, H, out.ctypes.data) == 0
    return out


@functools.lru_cache(None)
def _host_tool():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host")])
    return os.path.join(ROOT, "tests", "host", "test_host")


def host_tool_edges(u8):
    """EdgeSegment(scale 0, u8, 0, true) of the host mirror (host/edges.cpp), the function the driver calls: (H, W) uint8"""
    u8 = np.ascontiguousarray(u8, np.uint8)
    H, W = u8.shape
    with tempfile.TemporaryDirectory() as d:
        fn, out = os.path.join(d, "v.pgm"), os.path.join(d, "e.dmb")
        with open(fn, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (W, H))
            f.write(u8.tobytes())
        r = subprocess.run([_host_tool(), "--edges", fn, "0", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw = open(out, "rb").read()
    assert tuple(np.frombuffer(raw[:16], np.int32)) == (1, H, W, 0)
    return np.frombuffer(raw[16:], np.uint8).reshape(H, W)


def np_median(u8):
    """APD.cpp:420-427: the histogram median over grey levels 0..254, -1 if the running sum never passes half"""
    hist = np.bincount(u8.ravel(), minlength=256)
    cum = 0
    for i in range(255):
        cum += int(hist[i])
        if cum > u8.size // 2:
            return i
    return -1


def np_thresholds(median):
    """(low, high) as CannyL2 compares them: (int)((1 - 0.67f) * median) and median, squared only when positive"""
    t1, t2 = int(np.float32(1 - np.float32(0.67)) * np.float32(median)), int(median)
    sq = lambda t: int(np.floor(min(32767.0, float(t)) ** 2)) if t > 0 else int(np.floor(float(t)))
    return sq(t1), sq(t2)


def np_edges(u8):
    """the independent reading: _np_canny with the reference's thresholds, then the fix-ups statement by statement"""
    from test_host_oracles import _np_canny
    H, W = u8.shape
    med = np_median(u8)
    w2 = _np_canny(u8, int(np.float32(1 - np.float32(0.67)) * med), med).copy()
    for y in range(H):
        if not w2[y, 1]:
            w2[y, 0] = False
        if not w2[y, W - 2]:
            w2[y, W - 1] = False
    for x in range(W):
        if not w2[1, x]:
            w2[0, x] = False
        if not w2[H - 2, x]:
            w2[H - 1, x] = False
    return np.where(w2, 255, 0).astype(np.uint8)


def smooth_noisy(rs, W, H, noise=10.0):
    """a smooth field with a few steps plus noise: contours, chains and isolated responses at any size"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = 110 + 60 * np.sin(x / 7.0 + rs.uniform(0, 6)) * np.cos(y / 5.0 + rs.uniform(0, 6))
    f += 50 * ((x + 2 * y) % 37 < 15)
    f += rs.normal(0, noise, (H, W))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _steps(W, H, cols, rows, lo=30, hi=200, noise=0, seed=0):
    a = np.full((H, W), lo, np.float64)
    for c in cols:
        a[:, c:] = hi - a[:, c:] + lo
    for r in rows:
        a[r:, :] = hi - a[r:, :] + lo
    if noise:
        a += np.random.RandomState(seed).normal(0, noise, (H, W))
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


SIZES = [(3, 3), (3, 64), (64, 3), (4, 5), (63, 65), (64, 64), (65, 63), (257, 131)]   # (W, H)


@functools.lru_cache(None)
def images():
    """name -> (H, W) uint8 image, read-only"""
    out = {}
    W, H = 160, 120
    sc = synth.make_scene(W, H, 2)
    rng = np.random.default_rng(3)
    for k, img in enumerate([sc["images"][0], sc["images"][1], np.clip(sc["images"][2] + rng.normal(0, 6, (H, W)), 0, 255)]):
        out["view%d" % k] = np.rint(img).astype(np.uint8)
    rs = np.random.RandomState(11)
    out["noise_67x45"] = rs.randint(0, 256, (45, 67)).astype(np.uint8)
    a = rs.randint(0, 256, (48, 70)).astype(np.uint8)
    a[rs.uniform(size=a.shape) < 0.6] = 255
    out["median_minus_one"] = a                      # 60 % of the pixels at 255: no median below 255
    out["constant"] = np.full((31, 37), 93, np.uint8)
    out["zero"] = np.zeros((31, 37), np.uint8)
    W, H = 41, 29
    # steps whose responses fall on the frame and on the lines next to it: the fix-ups' ground
    for name, cols, rows in [("cols_1", [1], []), ("cols_2", [2], []), ("cols_w1", [W - 1], []), ("cols_w2", [W - 2], []), ("rows_1", [], [1]), ("rows_2", [], [2]),
                             ("rows_h1", [], [H - 1]), ("rows_h2", [], [H - 2]), ("frame_1", [1, W - 1], [1, H - 1]), ("frame_2", [2, W - 2], [2, H - 2]),
                             ("frame_12", [1, 2, W - 2, W - 1], [1, 2, H - 2, H - 1])]:
        out["step_" + name] = _steps(W, H, cols, rows)
        out["step_" + name + "_noisy"] = _steps(W, H, cols, rows, noise=25, seed=len(out))
    for (w, h) in SIZES:
        out["size_%dx%d" % (w, h)] = smooth_noisy(np.random.RandomState(w * 1000 + h), w, h)
        out["size_%dx%d_noise" % (w, h)] = np.random.RandomState(w * 7 + h).randint(0, 256, (h, w)).astype(np.uint8)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def expected_edges(name):
    """the host mirror's map of a case, checked once against the numpy reading"""
    u8 = images()[name]
    tool, model = host_tool_edges(u8), np_edges(u8)
    assert np.array_equal(tool, model), (name, int((tool != model).sum()))
    tool.setflags(write=False)
    return tool


# ---- three-state maps for the hysteresis alone: 0 = candidate, 1 = nothing, 2 = strong ---------------------------------------
def serpentine(W, H, strong=True):
    """a one-pixel-wide chain covering the map: every other row, joined at alternating ends; strong pixel at one end"""
    m = np.ones((H, W), np.uint8)
    m[0::2, :] = 0
    for k, r in enumerate(range(1, H - 1, 2)):
        m[r, W - 1 if k % 2 == 0 else 0] = 0
    if strong:
        m[0, 0] = 2
    return m


def spiral(n):
    m = np.ones((n, n), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 2
    for _ in range(n * n):
        moved = False
        for _turn in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and m[ny, nx] == 1 and not (0 <= fy < n and 0 <= fx < n and m[fy, fx] != 1):
                y, x, moved = ny, nx, True
                m[y, x] = 0
                break
            dy, dx = dx, -dy
        if not moved:
            break
    return m


@functools.lru_cache(None)
def maps():
    out = {}
    out["serpentine_129x67"] = serpentine(129, 67)
    out["serpentine_no_strong"] = serpentine(129, 67, strong=False)
    out["spiral_61"] = spiral(61)
    m = np.ones((70, 170), np.uint8)
    i = np.arange(60)
    m[i + 3, i + 5] = 0                       # down-right staircase: consecutive pixels touch by a corner only
    m[i + 3, 160 - i] = 0                     # down-left
    m[3, 5] = 2
    m[62, 101] = 2                            # the far end of the second one
    out["staircase"] = m
    m = np.ones((40, 150), np.uint8)
    m[5, 20:64] = 0                           # ends at column 63 ...
    m[5, 64:100] = 0                          # ... goes on at column 64
    m[5, 20] = 2
    m[8:16, 30] = 0                           # ends at row 15 ...
    m[16:24, 31] = 0                          # ... goes on at row 16, one column to the right
    m[23, 31] = 2
    m[8:16, 130] = 0
    m[16:24, 129] = 0                         # ... and one to the left
    m[8, 130] = 2
    m[30, 10:64] = 0                          # the same pieces without a strong pixel
    m[30, 64:90] = 0
    out["tile_boundaries"] = m
    m = np.zeros((67, 129), np.uint8)
    m[40, 77] = 2
    out["all_candidate"] = m
    out["all_strong"] = np.full((33, 65), 2, np.uint8)
    out["empty"] = np.ones((33, 65), np.uint8)
    for d in (0.1, 0.4, 0.6):
        rs = np.random.RandomState(int(d * 100))
        m = np.ones((131, 257), np.uint8)
        m[rs.uniform(size=m.shape) < d] = 0
        m[rs.uniform(size=m.shape) < 0.01] = 2
        out["random_%g" % d] = m
    for v in out.values():
        v.setflags(write=False)
    return out


def np_hysteresis(map3):
    """255 where a pixel is strong, or a candidate whose 8-connected component of non-empty pixels holds a strong one"""
    from scipy import ndimage
    lab, n = ndimage.label(map3 != 1, structure=np.ones((3, 3)))
    good = np.zeros(n + 1, bool)
    good[np.unique(lab[map3 == 2])] = True
    good[0] = False
    return np.where(good[lab], 255, 0).astype(np.uint8)


@functools.lru_cache(None)
def expected_hysteresis(name):
    e = np_hysteresis(maps()[name])
    e.setflags(write=False)
    return e
