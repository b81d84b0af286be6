"""Shared by the label-prior tests (test_labels_host.py, test_gpu_labels.py): the input images and the references they are held
against — the host mirror's LabelSegment with its intermediate maps and the serial host build of csrc/dvp_labels.hpp, both
through tests/labels_host, and scipy's connected components.  Every image and every reference is made once per case and handed
out read-only."""
import ctypes
import functools
import os
import subprocess

import numpy as np

from conftest import ROOT

_LIB = os.path.join(ROOT, "tests", "labels_host", "libdvp_labels_host.so")
STAGES = ("quarter", "texture", "lines", "resized", "cleaned")     # the host mirror's LabelStages, in order


@functools.lru_cache(None)
def host_lib():
    """the serial host build of csrc/dvp_labels.hpp next to host/labels.cpp's LabelSegment"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dvp-mvs_amd", "host")])
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(_LIB)])
    L = ctypes.CDLL(_LIB)
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    L.dvp_label_sizes_host.argtypes = [ci, ci, ci, vp]
    L.dvp_label_map_serial.argtypes = [vp, ci, ci, ll, ci] + [vp] * 7
    L.dvp_label_map_mirror.argtypes = [vp, ci, ci, ll, ci, ci] + [vp] * 6
    return L


def sizes(W, H, scale):
    """dict(quarter=(rows, cols), level=(rows, cols), weak_tex_num, unit), as labels.cpp derives them from the image size"""
    v = np.zeros(7, np.int32)
    assert host_lib().dvp_label_sizes_host(W, H, scale, v.ctypes.data) == 0
    weak = int(1.0 * H * W / (1024 << scale << scale))
    f = np.float32(1.0) / np.float32(1 << scale)
    rnd = lambda n: int(np.floor(float(np.float32(n) * f) + 0.5))          # std::round: halves away from zero
    assert (int(v[0]), int(v[1])) == (W // 2 // 2, H // 2 // 2) and (int(v[2]), int(v[3])) == (rnd(W), rnd(H)) and int(v[4]) == weak
    assert int(v[5]) == int(min(v[0], v[1]) / 30.0)
    return dict(quarter=(int(v[1]), int(v[0])), level=(int(v[3]), int(v[2])), weak_tex_num=weak, unit=int(v[5]))


def _rows(img):
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim == 2
    if a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a)
    return a


def serial(img, scale):
    """the kernels' text run serially on the host: (rc, dict of quarter, texture, region, lines, resized, cleaned, labels)"""
    a = _rows(img)
    H, W = a.shape
    try:
        s = sizes(W, H, scale)
    except AssertionError:
        return 1, {}
    q, l = s["quarter"], s["level"]
    if min(q) < 1 or min(l) < 1:
        return 1, {}
    out = dict(labels=np.zeros(l, np.int32), quarter=np.zeros(q, np.uint8), texture=np.zeros(q, np.uint8), region=np.zeros(q, np.int32), lines=np.zeros(q, np.uint8),
               resized=np.zeros(l, np.uint8), cleaned=np.zeros(l, np.uint8))
    rc = host_lib().dvp_label_map_serial(a.ctypes.data, W, H, a.strides[0], scale, *[out[n].ctypes.data for n in ("labels", "quarter", "texture", "region", "lines", "resized", "cleaned")])
    return rc, out


def mirror(img, scale, threads=0):
    """LabelSegment(scale, img, &stages) of the host mirror (host/labels.cpp), the function the driver calls"""
    a = _rows(img)
    H, W = a.shape
    s = sizes(W, H, scale)
    q, l = s["quarter"], s["level"]
    out = dict(labels=np.zeros(l, np.int32), quarter=np.zeros(q, np.uint8), texture=np.zeros(q, np.uint8), lines=np.zeros(q, np.uint8), resized=np.zeros(l, np.uint8),
               cleaned=np.zeros(l, np.uint8))
    assert host_lib().dvp_label_map_mirror(a.ctypes.data, W, H, a.strides[0], scale, threads, *[out[n].ctypes.data for n in ("labels",) + STAGES]) == 0
    for v in out.values():
        v.setflags(write=False)
    return out


def components(black):
    """scipy's 4-connected components of a boolean map: (labels, sizes)"""
    from scipy import ndimage
    lab, n = ndimage.label(black, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    return lab, np.bincount(lab.ravel(), minlength=n + 1)


def same_partition(a_ids, b_ids):
    """two id maps name the same sets: the pairs (a, b) that occur form a bijection"""
    pairs = np.unique(np.stack([np.asarray(a_ids).ravel(), np.asarray(b_ids).ravel()], 1), axis=0)
    return len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))


def check_against_mirror(got, want, weak_tex_num):
    """got: the device's or the serial build's maps (with region), want: the mirror's.  Every map exactly; the region map by its
    partition and its large regions, against scipy on the mirror's texture map; the labels also by scipy on the cleaned map."""
    for n in STAGES + ("labels",):
        assert got[n].shape == want[n].shape, (n, got[n].shape, want[n].shape)
        assert np.array_equal(got[n], want[n]), (n, int((got[n] != want[n]).sum()), got[n].size)
    lab, size = components(want["texture"] == 0)
    large = (lab > 0) & (size[lab] >= weak_tex_num)
    region = got["region"]
    assert np.array_equal(region >= 0, large), int(((region >= 0) != large).sum())
    if large.any():
        assert same_partition(region[large], lab[large])
        ids, first = np.unique(lab.ravel(), return_index=True)          # the smallest pixel index of every region
        lut = np.zeros(int(ids.max()) + 1, np.int64)
        lut[ids] = first
        assert np.array_equal(region[large], lut[lab[large]])
    lab, size = components(want["cleaned"] == 0)
    labels = got["labels"]
    assert np.array_equal(labels == 0, want["cleaned"] == 255)
    small = (lab > 0) & (size[lab] <= weak_tex_num)
    assert np.array_equal(labels == -1, small)
    big = (lab > 0) & ~small
    if big.any():
        assert same_partition(lab[big], labels[big]) and labels[big].min() > 0
        # Connect's numbers: 1, 2, ... in raster order of the first pixels, small regions counted, gaps kept
        ids, first = np.unique(lab.ravel(), return_index=True)
        ids, first = ids[ids > 0], first[ids > 0]
        lut = np.zeros(int(ids.max()) + 1, np.int64)
        lut[ids[np.argsort(first)]] = np.arange(1, len(ids) + 1)
        assert np.array_equal(labels[big], lut[lab[big]])


# ---- the images ---------------------------------------------------------------------------------------------------------------
SIZES = [(12, 12), (13, 15), (63, 65), (130, 70), (257, 131), (258, 130), (480, 360), (515, 259)]   # (W, H)
SCALES = (0, 1, 2)
CONTENTS = ("picture", "constant", "noise", "checker", "serpentine", "spiral", "threshold", "roberts", "frame")


def _noise(W, H, seed):
    return np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)


def picture(W, H):
    """test_host_oracles.py's walls / bars / islands / ramp picture (480 x 360 there), scaled to the size"""
    rng = np.random.default_rng(11)
    X = lambda v: int(round(v * W / 480.0))
    Y = lambda v: int(round(v * H / 360.0))
    img = np.full((H, W), 90, np.uint8)
    img[:, X(250):] = 170
    img[:, X(238):X(262)] = rng.integers(0, 255, (H, X(262) - X(238)))
    img[Y(120):Y(170), X(60):X(120)] = rng.integers(0, 255, (Y(170) - Y(120), X(120) - X(60)))
    img[Y(200):Y(206), X(300):X(420)] = rng.integers(0, 255, (Y(206) - Y(200), X(420) - X(300)))
    img[Y(128):Y(140), X(80):X(92)] = 128
    img[Y(148):Y(160), X(100):X(112)] = 40
    img += rng.integers(0, 2, (H, W)).astype(np.uint8)
    n = X(200) - X(20)
    img[Y(300):Y(340), X(20):X(200)] = (np.arange(n)[None, :] * 1.4 * 480.0 / W).astype(np.int64).clip(0, 230).astype(np.uint8) + 20
    return img


def _corridor(coarse, W, H, seed, cell=16):
    """coarse: 1 = wall, else corridor, in cells of 16 x 16 full-size pixels (4 x 4 at quarter size: the corridor keeps three
    black pixels of width there); the walls are noise, the corridor is flat"""
    cells = np.ones(((H + cell - 1) // cell, (W + cell - 1) // cell), np.uint8)
    h, w = min(cells.shape[0], coarse.shape[0]), min(cells.shape[1], coarse.shape[1])
    cells[:h, :w] = coarse[:h, :w]
    wall = np.kron(cells, np.ones((cell, cell), np.uint8))[:H, :W] == 1
    return np.where(wall, _noise(W, H, seed), 128).astype(np.uint8)


def serpentine(W, H):
    import np_edges as E
    ch, cw = (H + 15) // 16, (W + 15) // 16
    return _corridor(E.serpentine(cw, ch, strong=False) if cw > 1 and ch > 2 else np.zeros((ch, cw), np.uint8), W, H, 21)


def spiral(W, H):
    import np_edges as E
    return _corridor(E.spiral(max(1, min((H + 15) // 16, (W + 15) // 16))), W, H, 22)


def _stripes(W, H):
    """columns of one quarter-size pixel, 60 / 200: Roberts 197 everywhere, and against a flat 128 next to them at least 68"""
    return np.where((np.arange(W)[None, :] // 4) % 2 == 0, 60, 200).astype(np.uint8) * np.ones((H, 1), np.uint8)


def threshold(W, H, scale):
    """flat shapes on stripes whose black regions at quarter size hold weak_tex_num - 1, weak_tex_num and weak_tex_num + 1
    pixels (where the sizes are multiples of 4 the halvings are exact and so are the counts): full rows and one partial row.
    At scale 2 the level map is the quarter map, so the same regions meet the `<=` there; at scales 0 and 1 the up-sampling
    keeps a level pixel black only where all four of its sources are, which makes every inner region a multiple of 4 or 16."""
    weak = int(1.0 * H * W / (1024 << scale << scale))
    qw, qh = W // 4, H // 4
    img = _stripes(W, H)
    y = 3
    for n in (weak - 1, weak, weak + 1):
        if n < 1:
            continue
        w = max(1, min(qw - 8, int(np.ceil(np.sqrt(n * 2.0)))))
        rows, rest = n // w, n % w
        black = np.zeros((qh + 2, qw + 2), bool)
        if y + rows + 3 >= qh:
            break
        black[y:y + rows, 3:3 + w] = True
        black[y + rows, 3:3 + rest] = True
        flat = black.copy()                                              # a pixel is black when its 2 x 2 footprint is flat
        flat[1:, :] |= black[:-1, :]
        flat[:, 1:] |= black[:, :-1]
        flat[1:, 1:] |= black[:-1, :-1]
        full = np.kron(flat.astype(np.uint8), np.ones((4, 4), np.uint8))[:H, :W] == 1
        img[:full.shape[0], :full.shape[1]][full] = 128
        y += rows + 4
    return img


ROBERTS_ROOTS = (4, 5, 255, 256, 260, 261)


def roberts(W, H):
    """2 x 2 quarter-size patches (4 x 4 full-size pixels each) whose Roberts root is 4, 5, 255, 256, 260, 261: the byte cast
    makes 256 ... 260 black again"""
    img = np.full((H, W), 255, np.uint8)
    k = 0
    for (t1, t2) in ((4, 0), (5, 0), (255, 0), (182, 181), (184, 184), (185, 185)):
        assert int(np.floor(np.sqrt(t1 * t1 + t2 * t2))) == ROBERTS_ROOTS[k]
        y, x = 4 * (2 + 4 * (k // 3)), 4 * (2 + 4 * (k % 3))
        if y + 8 <= H and x + 8 <= W:
            img[y + 4:y + 8, x + 4:x + 8] = 255 - t1
            img[y:y + 4, x + 4:x + 8] = 255 - t2
        k += 1
    return img


def frame(W, H):
    """noise with flat blocks in the four corners and in the middle of every side: the frame clean-up has pixels to change"""
    img = _noise(W, H, 31)
    h, w = max(2, H // 3), max(2, W // 3)
    for ys in (slice(0, h), slice(H - h, H)):
        for xs in (slice(0, w), slice(W - w, W)):
            img[ys, xs] = 77
    img[:h // 2 + 1, W // 2 - w // 4:W // 2 + w // 4 + 1] = 150
    img[H // 2 - h // 4:H // 2 + h // 4 + 1, W - w // 2 - 1:] = 150
    return img


@functools.lru_cache(None)
def image(content, W, H, scale):
    if content == "picture":
        img = picture(W, H)
    elif content == "constant":
        img = np.full((H, W), 93, np.uint8)
    elif content == "noise":
        img = _noise(W, H, W * 7 + H)
    elif content == "checker":
        img = np.where(((np.arange(W)[None, :] // 4) + (np.arange(H)[:, None] // 4)) % 2 == 0, 60, 200).astype(np.uint8)
    elif content == "serpentine":
        img = serpentine(W, H)
    elif content == "spiral":
        img = spiral(W, H)
    elif content == "threshold":
        img = threshold(W, H, scale)
    elif content == "roberts":
        img = roberts(W, H)
    else:
        img = frame(W, H)
    img = np.ascontiguousarray(img, np.uint8)
    assert img.shape == (H, W)
    img.setflags(write=False)
    return img


CASES = [(c, W, H, s) for (W, H) in SIZES for s in SCALES for c in CONTENTS]


def case_id(case):
    return "%s-%dx%d-s%d" % case


@functools.lru_cache(None)
def expected(case):
    """the host mirror's maps of a case"""
    c, W, H, s = case
    return mirror(image(c, W, H, s), s)


def long_corridor(W=1023, H=515):
    """one serpentine corridor over the whole full-size image, in cells of 32 pixels: seven black pixels wide at quarter size,
    more than the gap the Hough lines bridge (unit = 4), so no line cuts it; at scale 0 one region of far more than 100 k level
    pixels whose union-find links run through every tile"""
    import np_edges as E
    coarse = E.serpentine((W + 31) // 32, (H + 31) // 32, strong=False)
    return _corridor(coarse, W, H, 41, cell=32)
