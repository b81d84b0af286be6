"""The JPEG files the input-decoder tests share (tests/test_jpeg_dec_host.py on the host, tests/test_gpu_jpeg_decode.py on the
device): written with PIL, none committed.  A case is (sampling, width, height, restart, quality, picture); CASES covers every
sampling at every size, every picture at every quality, and every restart interval with every sampling — each file decodes in
milliseconds."""
import io

import numpy as np
from PIL import Image

SAMPLINGS = ["444", "422", "420", "grey"]
# 1x1 and 8x8: one MCU (for 4:4:4 / grey); 7x9, 17x33, 250x130: partial blocks and partial MCUs on both edges; 515x259: 65 luma
# blocks across, a row of blocks crosses a wave of eight blocks with one left over
SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (64, 64), (250, 130), (515, 259)]
RESTARTS = [0, 1, 7]          # MCUs per interval; the sizes give 1, 2, 3, 4, 8, 16, 32, 33 or 65 MCUs per row: 7 divides none
QUALITIES = [30, 75, 95, 100]
PICTURES = ["constant", "ramp", "checker", "noise", "flat"]


def picture(name, W, H):
    """(H, W, 3) uint8, deterministic"""
    y, x = np.mgrid[0:H, 0:W]
    if name == "constant":
        a = np.empty((H, W, 3), np.uint8)
        a[:] = (200, 90, 40)
    elif name == "ramp":
        a = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(W + H - 2, 1)], -1).astype(np.uint8)
    elif name == "checker":     # 4 x 4 squares, saturated colours
        c = ((x // 4 + y // 4) & 1).astype(np.uint8)
        a = np.stack([c * 255, (1 - c) * 255, c * 255], -1).astype(np.uint8)
    elif name == "noise":       # uniform noise per channel, an eighth of the pixels black or white (luma then reaches both ends of
        rng = np.random.default_rng(W * 1000 + H)                      # the range, and at quality 100 the reconstruction overshoots them)
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ends = rng.integers(0, 16, (H, W))
        a[ends == 0] = 0
        a[ends == 1] = 255
    elif name == "flat":        # large flat areas (blocks with a DC record alone), one of them mid-grey (a DC prediction of 0), and a textured band
        a = np.empty((H, W, 3), np.uint8)
        a[:] = 128
        a[:, W // 2:] = (30, 220, 120)
        band = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
        a[H // 3:H // 3 + max(H // 6, 1)] = band[H // 3:H // 3 + max(H // 6, 1)]
    else:
        raise KeyError(name)
    return a


def jpeg_bytes(sampling, W, H, restart, quality, pic, **more):
    a = picture(pic, W, H)
    if sampling == "grey":
        im = Image.fromarray(a[:, :, 1].copy(), "L")
        kw = {}
    else:
        im = Image.fromarray(a, "RGB")
        kw = dict(subsampling={"444": 0, "422": 1, "420": 2}[sampling])
    if restart:
        kw["restart_marker_blocks"] = restart
    kw.update(more)
    b = io.BytesIO()
    im.save(b, "JPEG", quality=quality, **kw)
    return b.getvalue()


def _cases():
    out = []
    k = 0
    for (W, H) in SIZES:                       # every sampling at every size; the other three cycle
        for s in SAMPLINGS:
            out.append((s, W, H, RESTARTS[k % 3], QUALITIES[k % 4], PICTURES[k % 5]))
            k += 1
    for q in QUALITIES:                        # every picture at every quality
        for p in PICTURES:
            out.append(("420" if (len(out) & 1) else "444", 250, 130, 0, q, p))
    for r in RESTARTS:                         # every restart interval with every sampling
        for s in SAMPLINGS:
            out.append((s, 250, 130, r, 75, "noise"))
            out.append((s, 17, 33, r, 95, "flat"))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()
# where the records are compared coefficient by coefficient with a dense decode
RECORD_CASES = [("420", 250, 130, 7, 100, "noise"), ("422", 17, 33, 1, 75, "flat"), ("grey", 515, 259, 0, 30, "ramp")]


def case_id(c):
    return "%s-%dx%d-r%d-q%d-%s" % c


def libjpeg_luma(data):
    """the luma plane as this machine's libjpeg decodes it straight to greyscale"""
    im = Image.open(io.BytesIO(data))
    if im.mode != "L":
        im.draft("L", im.size)
    return np.asarray(im.convert("L") if im.mode != "L" else im)


def truncated_in_segment(data):
    """cut in the middle of the first DQT segment"""
    i = data.index(b"\xff\xdb")
    return data[:i + 20]


def truncated_in_scan(data):
    """cut a third into the entropy-coded data (a file with restart markers: the next marker is never found)"""
    i = data.index(b"\xff\xda")
    return data[:i + (len(data) - i) // 3]


def without_dht(data):
    """every DHT segment removed"""
    out, p = bytearray(data[:2]), 2
    while p + 4 <= len(data):
        assert data[p] == 0xFF
        marker, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        if marker == 0xDA:
            out += data[p:]
            break
        if marker != 0xC4:
            out += data[p:p + 2 + n]
        p += 2 + n
    return bytes(out)


def rejected_files():
    """name -> (bytes, the host path's message)"""
    good = jpeg_bytes("420", 64, 64, 1, 75, "noise")
    return {
        "cut_in_segment": (truncated_in_segment(good), "truncated segment"),
        "cut_in_scan": (truncated_in_scan(good), "missing restart marker"),
        "progressive": (jpeg_bytes("420", 64, 64, 0, 75, "noise", progressive=True), "progressive / lossless / arithmetic-coded JPEG is not supported (baseline only)"),
        "no_dht": (without_dht(good), "missing table"),
    }
