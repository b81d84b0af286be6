"""A numpy reading of the reference's preview renderers, written from the source text of the reference's APD.cpp:
ShowDepthMap (:694-758), ShowNormalMap (:760-783) and ShowWeakImage (:785-812), applied to the maps the driver stores
(main.cpp:300-309: depth = plane.w inside [depth_min, depth_max], else 0, and the state UNKNOWN).  BGR, as the reference
hands cv::Mat to cv::imwrite.

TEST INFRASTRUCTURE.  Every float32 step is one numpy float32 operation (one IEEE rounding, no contraction); the steps the
source writes in double (pow, the 128.0 / 127.0 bands) are float64 here."""
import numpy as np

WEAK, STRONG, UNKNOWN = 0, 1, 2
f32 = np.float32


def unpack(planes, weak, dmin, dmax):
    """main.cpp:300-309 (`!(w < min || w > max)`: NaN depths are kept)"""
    planes = np.asarray(planes, np.float32).reshape(-1, 4)
    w = planes[:, 3]
    with np.errstate(invalid="ignore"):
        usable = ~((w < f32(dmin)) | (w > f32(dmax)))
    depth = np.where(usable, w, f32(0)).astype(np.float32)
    state = np.where(usable, np.asarray(weak, np.uint8).reshape(-1), np.uint8(UNKNOWN)).astype(np.uint8)
    return depth, planes[:, :3].copy(), state


def depth_preview(depth, dmin, dmax):
    """ShowDepthMap, APD.cpp:694-758 -> (..., 3) uint8 BGR"""
    d = np.asarray(depth, np.float32)
    dmin, dmax = f32(dmin), f32(dmax)
    out = np.zeros(d.shape + (3,), np.uint8)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        skip = (d < dmin) | (d > dmax) | np.isnan(d)                        # :700-702
        pv = (dmax - d) / (dmax - dmin)                                     # :703 (float / float)
        pv = np.where(pv > 1, f32(1), pv)                                   # :704-709
        pv = np.where(pv < 0, f32(0), pv)
        pv = (pv * f32(255)).astype(np.float32)                             # :710
        pv = np.where(pv > 255, f32(255), np.where(pv < 0, f32(0), pv))     # :711-716
        b1 = ~skip & (pv <= 51)
        b2 = ~skip & ~b1 & (pv <= 102)
        b3 = ~skip & ~b1 & ~b2 & (pv <= 153)
        b4 = ~skip & ~b1 & ~b2 & ~b3 & (pv <= 204)
        b5 = ~skip & ~b1 & ~b2 & ~b3 & ~b4 & (pv <= 255)

        def u8(x):   # float -> unsigned char: truncation (the values are in [0, 255] where they are used)
            return np.where(np.isfinite(x), x, 0).astype(np.int64).astype(np.uint8)

        t = pv
        out[b1] = np.stack([np.full(b1.sum(), 255), u8(t[b1] * f32(5)), np.zeros(b1.sum())], -1)                  # :718-723
        t = (pv - f32(51)).astype(np.float32)
        out[b2] = np.stack([u8(f32(255) - t[b2] * f32(5)), np.full(b2.sum(), 255), np.zeros(b2.sum())], -1)      # :724-730
        t = (pv - f32(102)).astype(np.float32)
        out[b3] = np.stack([np.zeros(b3.sum()), np.full(b3.sum(), 255), u8(t[b3] * f32(5))], -1)                  # :731-737
        t = (pv - f32(153)).astype(np.float32)
        v = u8(t[b4].astype(np.float64) * 128.0 / 51 + 0.5).astype(np.int64)                                     # :738-744
        out[b4] = np.stack([np.zeros(b4.sum()), 255 - v, np.full(b4.sum(), 255)], -1)
        t = (pv - f32(204)).astype(np.float32)
        v = u8(t[b5].astype(np.float64) * 127.0 / 51 + 0.5).astype(np.int64)                                     # :745-751
        out[b5] = np.stack([np.zeros(b5.sum()), 127 - v, np.full(b5.sum(), 255)], -1)
    return out


def normal_preview(normal):
    """ShowNormalMap, APD.cpp:760-783 -> (..., 3) uint8 BGR (channel 0 = n.x)"""
    n = np.asarray(normal, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n64 = n.astype(np.float64)
        norm = np.sqrt((n64[..., 0] * n64[..., 0] + n64[..., 1] * n64[..., 1]) + n64[..., 2] * n64[..., 2]).astype(np.float32)   # :768 pow -> double
        inv = (f32(1) / norm).astype(np.float32)                             # Vec3f / float = v * (1.f / norm)
        nn = (n * inv[..., None]).astype(np.float32)
        nn = np.where((norm == 0)[..., None], f32(0), nn)                    # :769-771
        v = ((nn * f32(127.5)).astype(np.float32) + f32(127.5)).astype(np.float32)   # convertTo(.., 127.5, 127.5), unfused
        r = np.rint(v)                                                       # saturate_cast<uchar>: cvRound (half to even)
        r = np.where(np.isnan(r), 0, np.clip(r, 0, 255))
    return r.astype(np.uint8)


def weak_preview(state):
    """ShowWeakImage, APD.cpp:785-812 -> (..., 3) uint8 BGR; values other than the three states are black here"""
    s = np.asarray(state, np.uint8)
    out = np.zeros(s.shape + (3,), np.uint8)
    out[s == WEAK] = (255, 255, 255)
    out[s == STRONG] = (0, 255, 0)
    out[s == UNKNOWN] = (0, 0, 255)
    return out


def previews(planes, weak, dmin, dmax, H, W):
    """the three images the driver writes for a view: dict kind -> (H, W, 3) BGR"""
    depth, normal, state = unpack(planes, weak, dmin, dmax)
    return dict(depth=depth_preview(depth, dmin, dmax).reshape(H, W, 3), normal=normal_preview(normal).reshape(H, W, 3),
                weak=weak_preview(state).reshape(H, W, 3))


def pil_jpeg(img, quality=95, restart=None):
    """libjpeg-turbo's file (through Pillow) of a BGR (H, W, 3) or grey (H, W) image: 4:2:0, standard tables, restart interval
    `restart` MCUs (None: no markers).  Grey is saved with subsampling 0, which gives the 1x1 sampling factor OpenCV's
    imwrite writes (with 2, Pillow marks the single component 2x2; the coded data are the same)."""
    import io
    from PIL import Image
    img = np.asarray(img, np.uint8)
    im = Image.fromarray(img, "L") if img.ndim == 2 else Image.fromarray(np.ascontiguousarray(img[..., ::-1]))
    kw = dict(quality=quality, subsampling=2 if img.ndim == 3 else 0, optimize=False)
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def dri(jpeg_bytes):
    """restart interval of a JPEG file's DRI segment (0 if it has none)"""
    i = 2
    while i + 4 <= len(jpeg_bytes):
        m = jpeg_bytes[i + 1]
        n = int.from_bytes(jpeg_bytes[i + 2:i + 4], "big")
        if m == 0xDD:
            return int.from_bytes(jpeg_bytes[i + 4:i + 6], "big")
        if m == 0xDA:
            return 0
        i += 2 + n
    return 0


def decode(jpeg_bytes):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpeg_bytes)).convert("RGB" if jpeg_bytes[jpeg_bytes.find(b"\xff\xc0") + 9] == 3 else "L"))
