"""Shared by the view clean-up tests (test_viewclean_host.py, test_gpu_viewclean.py): the selected-view word maps and the two
independent references they are held against — scipy.ndimage.label with the 4-connected structure + numpy.bincount, and the host
mirror (host/cc.cpp's Connect + the driver's fill rule) through tests/viewclean_host.  Every reference is computed once per
case, the two are asserted equal there, and the result is handed out read-only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import np_edges as E
from conftest import ROOT

_LIB = os.path.join(ROOT, "tests", "viewclean_host", "libdvp_viewclean_host.so")


@functools.lru_cache(None)
def host_lib():
    """the serial host build of csrc/dvp_viewclean.hpp + the host mirror's clean-up"""
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(_LIB)])
    L = ctypes.CDLL(_LIB)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.dvp_clean_selected_views_serial.argtypes = [vp, ci, ci, ci, ci, vp]
    L.dvp_clean_selected_views_mirror.argtypes = [vp, ci, ci, ci, ci, vp]
    return L


def tile():
    """(TILE_W, TILE_H) of the kernel"""
    L = host_lib()
    return L.dvp_viewclean_tile_w(), L.dvp_viewclean_tile_h()


def _call(fn, views, num_src, min_region):
    a = np.ascontiguousarray(views, np.uint32)
    H, W = a.shape
    out = np.full((H, W), 0xdeadbeef, np.uint32)
    rc = fn(a.ctypes.data, W, H, int(num_src), int(min_region), out.ctypes.data)
    return rc, out


def serial_clean(views, num_src, min_region):
    """the kernels' text run serially on the host, tile by tile: (rc, words)"""
    return _call(host_lib().dvp_clean_selected_views_serial, views, num_src, min_region)


def mirror_clean(views, num_src, min_region):
    """the host mirror: what `apd --cleanup-on host` computes"""
    rc, out = _call(host_lib().dvp_clean_selected_views_mirror, views, num_src, min_region)
    assert rc == 0
    return out


def low_mask(num_src):
    return np.uint32((1 << num_src) - 1)


def np_clean(views, num_src, min_region):
    """the independent reading: per bit, scipy's 4-connected components of the clear pixels and their sizes"""
    from scipy import ndimage
    views = np.asarray(views, np.uint32)
    out = views & low_mask(num_src)
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    for b in range(num_src):
        clear = ((views >> np.uint32(b)) & np.uint32(1)) == 0
        lab, n = ndimage.label(clear, structure=cross)
        cnt = np.bincount(lab.ravel(), minlength=n + 1).astype(np.int64)
        small = clear & (cnt[lab] < int(min_region))
        out = out | (small.astype(np.uint32) << np.uint32(b))
    return out.astype(np.uint32)


# ---- planes: (H, W) bool, True = the bit is CLEAR (the pixel does not select the view) ------------------------------------------
def checkerboard(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return (x + y) % 2 == 0


def random_plane(W, H, density, seed):
    return np.random.RandomState(seed).uniform(size=(H, W)) < density


def serpentine(W, H):
    return E.serpentine(W, H) != 1


def spiral(W, H):
    """a one-pixel-wide path winding inwards over the whole map, one pixel of wall between its turns"""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    inside = lambda yy, xx: 0 <= yy < H and 0 <= xx < W
    for _ in range(W * H):
        moved = False
        for _turn in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(fy, fx) and m[fy, fx]):
                y, x, moved = ny, nx, True
                m[y, x] = True
                break
            dy, dx = dx, -dy
        if not moved:
            break
    return m


def staircase_corners(W, H):
    """consecutive pixels touch by a corner only: every pixel is its own component"""
    p = np.zeros((H, W), bool)
    n = min(W // 2, H) - 2
    i = np.arange(n)
    p[i + 1, i + 1] = True            # down-right, in the left half
    p[i + 1, W - 2 - i] = True        # down-left, in the right half
    return p


def staircase_edges(W, H):
    """right, down, right, down ...: one 4-connected component across every tile it meets"""
    p = np.zeros((H, W), bool)
    x = y = 0
    while x < W and y < H:
        p[y, x] = True
        if x + 1 < W:
            p[y, x + 1] = True
        x, y = x + 1, y + 1
    return p


def seam_weave(W, H, seam, vertical=True):
    """one component that crosses the seam after column / row `seam` on every other line, joined at alternating ends"""
    if not vertical:
        return seam_weave(H, W, seam, True).T.copy()
    p = np.zeros((H, W), bool)
    a, b = seam - 1, seam + 2                     # columns a .. b straddle the seam
    ys = list(range(0, H, 2))
    for k, y in enumerate(ys):
        p[y, a:b + 1] = True
        if k + 1 < len(ys):
            p[y + 1, a if k % 2 == 0 else b] = True
    return p


def bars(W, H, m, seam_x, seam_y):
    """bars of m - 1, m, m + 1 pixels: inside a tile, across the vertical seam after column seam_x, and (upright) across the
    horizontal seam after row seam_y"""
    p = np.zeros((H, W), bool)
    for k, n in enumerate((m - 1, m, m + 1)):
        p[1 + 2 * k, 2:2 + n] = True                                   # inside the first tile
        p[1 + 2 * k, seam_x - n // 2 + 1:seam_x - n // 2 + 1 + n] = True   # across the vertical seam
        x = 30 + 2 * k
        p[seam_y - n // 2 + 1:seam_y - n // 2 + 1 + n, x] = True       # across the horizontal seam
    return p


def words_of(planes, garbage_seed=None, num_src=None):
    """bit b = NOT planes[b]; optional random bits above num_src"""
    H, W = planes[0].shape if planes else (0, 0)
    v = np.zeros((H, W), np.uint32)
    for b, p in enumerate(planes):
        v |= (~p).astype(np.uint32) << np.uint32(b)
    if garbage_seed is not None and num_src < 32:
        g = np.random.RandomState(garbage_seed).randint(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)
        v |= g & ~low_mask(num_src)
    return v


def pattern(k, W, H):
    """a different plane per bit"""
    kind = k % 8
    if kind == 0:
        return random_plane(W, H, 0.62, 100 + k)          # above the site-percolation threshold: one region larger than 1280 pixels
    if kind == 1:
        return random_plane(W, H, 0.1, 100 + k)
    if kind == 2:
        return random_plane(W, H, 0.9, 100 + k)
    if kind == 3:
        return serpentine(W, H)
    if kind == 4:
        return checkerboard(W, H)
    if kind == 5:
        return random_plane(W, H, 0.5, 100 + k)
    if kind == 6:
        y, x = np.mgrid[0:H, 0:W]
        return ((x // (7 + k)) + (y // (5 + k))) % 2 == 0          # blocks of (7 + k) x (5 + k) pixels: each one component
    return random_plane(W, H, 0.55, 100 + k) | (np.mgrid[0:H, 0:W][1] % 64 == 63)


@functools.lru_cache(None)
def sizes():
    TW, R = tile()
    assert TW == 64
    return [(1, 1), (1, 130), (130, 1), (63, 5), (64, R), (65, R + 1), (129, 2 * R + 1), (257, 131)]   # (W, H)


@functools.lru_cache(None)
def cases():
    """name -> (words (H, W) uint32 read-only, num_src, min_region)"""
    TW, R = tile()
    out = {}
    for (W, H) in sizes():
        tag = "%dx%d" % (W, H)
        full = np.ones((H, W), bool)
        out["all_clear_eq_" + tag] = (words_of([full]), 1, W * H)
        out["all_clear_gt_" + tag] = (words_of([full]), 1, W * H + 1)
        out["all_set_" + tag] = (words_of([~full]), 1, 20)
        out["checker_m1_" + tag] = (words_of([checkerboard(W, H)]), 1, 1)
        out["checker_m2_" + tag] = (words_of([checkerboard(W, H)]), 1, 2)
        out["random_" + tag] = (words_of([random_plane(W, H, d, W * 31 + H + k) for k, d in enumerate((0.1, 0.5, 0.9))]), 3, 6)
    for (W, H) in [(129, 2 * R + 1), (257, 131)]:
        tag = "%dx%d" % (W, H)
        # two clear pixels that touch only by a corner: across a tile corner, across a vertical and across a horizontal seam
        p = np.zeros((H, W), bool)
        p[R - 1, 63] = p[R, 64] = True
        p[3, 63] = p[4, 64] = True
        p[R - 1, 10] = p[R, 11] = True
        p[R - 1, 64] = p[R, 63] = False
        out["diagonal_" + tag] = (words_of([p]), 1, 2)
        for name, q in [("serpentine", serpentine(W, H)), ("spiral", spiral(W, H)),
                        ("stair_edges", staircase_edges(W, H)), ("weave_v", seam_weave(W, H, 63, True)), ("weave_h", seam_weave(W, H, R - 1, False))]:
            n = int(q.sum())
            out["%s_eq_%s" % (name, tag)] = (words_of([q]), 1, n)
            out["%s_gt_%s" % (name, tag)] = (words_of([q]), 1, n + 1)
        out["stair_corners_" + tag] = (words_of([staircase_corners(W, H)]), 1, 2)
        out["bars_" + tag] = (words_of([bars(W, H, 20, 63, R - 1)]), 1, 20)
    W, H = 257, 131
    for num_src in (0, 1, 9, 31, 32):
        planes = [pattern(k, W, H) for k in range(num_src)]
        if num_src == 0:
            base = np.zeros((H, W), np.uint32)
            base |= np.random.RandomState(1).randint(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)
        else:
            base = words_of(planes, garbage_seed=num_src, num_src=num_src)
        for m in (-5, 0, 20, 1280):
            out["words_s%d_m%d" % (num_src, m)] = (base, num_src, m)
    for v, _, _ in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def expected(name):
    """the host mirror's words of a case, checked once against scipy's"""
    views, num_src, min_region = cases()[name]
    want, model = mirror_clean(views, num_src, min_region), np_clean(views, num_src, min_region)
    assert np.array_equal(want, model), (name, int((want != model).sum()))
    want.setflags(write=False)
    return want


def smooth_words(W, H, num_src, seed=4, salt=0.02):
    """smooth-field thresholds per bit + salt noise: large regions with specks in them, as a pass leaves the words"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    v = np.zeros((H, W), np.uint32)
    for b in range(num_src):
        f = np.sin(x / np.float32(40 + 7 * b) + np.float32(rs.uniform(0, 6))) * np.cos(y / np.float32(33 + 5 * b) + np.float32(rs.uniform(0, 6)))
        bit = f > np.float32(rs.uniform(-0.4, 0.4))
        flip = rs.uniform(size=(H, W)) < salt
        v |= (bit ^ flip).astype(np.uint32) << np.uint32(b)
    return v
