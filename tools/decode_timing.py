#!/usr/bin/env python3
"""Where the input JPEG decode spends its time, and what `apd --decode-on gpu` can move: writes profiles/decode_timing.txt.

Host part (needs no GPU): a 6208 x 4128 4:2:0 file is made here with PIL from a deterministic picture with texture, and
tools/decode_timing.cpp — the three parts of host/jpeg.cpp's DecodeJpeg from the shared headers — is built and run on it,
single-threaded, median of five: (a) marker parse + entropy decode, (b) inverse DCT + plane stores, (c) the colour loop; with
the bytes of coefficient records per pixel.

Device part (only where a GPU is present; else the file says "not measured on the device"): dvp_jpeg_decode and
dvp_jpeg_decode_into_store on the same file, their host part (parse + entropy decode) and device part (upload, launches, read-back, wait),
median of five after one warm-up call.  Per-kernel times want a run of their own:
    rocprofv3 --kernel-trace --stats -d /tmp/jd -- python tools/decode_timing.py --device-only
usage: decode_timing.py [--quality Q] [--size WxH] [--device-only] [--out FILE]"""
import io
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def textured_picture(W, H):
    """(H, W, 3) uint8: smooth colour gradients, a few octaves of value noise and fine grain — deterministic"""
    rng = np.random.default_rng(20240)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    a = np.stack([120 + 90 * np.sin(x / 700.0) * np.cos(y / 500.0), 110 + 80 * np.cos(x / 900.0 + y / 400.0), 100 + 70 * np.sin(y / 650.0)], -1)
    for cell, gain in ((256, 40.0), (64, 24.0), (16, 14.0), (4, 8.0)):
        g = rng.standard_normal((H // cell + 2, W // cell + 2, 3)).astype(np.float32)
        a += gain * np.repeat(np.repeat(g, cell, 0), cell, 1)[:H, :W]
    a += 3.0 * rng.standard_normal((H, W, 3)).astype(np.float32)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def main():
    args = sys.argv[1:]
    quality = int(args[args.index("--quality") + 1]) if "--quality" in args else 95
    W, H = (int(v) for v in args[args.index("--size") + 1].split("x")) if "--size" in args else (6208, 4128)
    out_file = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "decode_timing.txt")
    device_only = "--device-only" in args
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(textured_picture(W, H), "RGB").save(b, "JPEG", quality=quality, subsampling=2)
    data = b.getvalue()
    lines = ["input decode timing (tools/decode_timing.py)",
             "file: %d x %d, 4:2:0, PIL quality %d, %d bytes (%.2f bytes per pixel), deterministic textured picture" % (W, H, quality, len(data), len(data) / (W * H)), ""]
    if not device_only:
        with tempfile.TemporaryDirectory() as tmp:
            exe, jpg = os.path.join(tmp, "decode_timing"), os.path.join(tmp, "a.jpg")
            open(jpg, "wb").write(data)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "decode_timing.cpp")])
            text = subprocess.run([exe, jpg, "5"], capture_output=True, text=True, check=True).stdout
        lines.append("host, one thread, median of 5 (ms):")
        for row in text.strip().splitlines():
            w = row.split()
            v = dict(zip(w[0::2], w[1::2]))
            ch, a, bb, c = int(v["channels"]), float(v["entropy_ms"]), float(v["blocks_ms"]), float(v["colour_ms"])
            total = a + bb + c
            lines.append("  %s: (a) parse + entropy decode %.1f   (b) inverse DCT + plane stores %.1f   (c) colour loop %.1f   total %.1f" % ("grey  " if ch == 1 else "colour", a, bb, c, total))
            lines.append("          share that can move to the device, (b) + (c): %.0f %%;  what stays, (a): %.0f %%" % (100 * (bb + c) / total, 100 * a / total))
            lines.append("          coefficient records + offsets: %d bytes = %.2f bytes per pixel, against %d byte(s) per pixel of the plane; %d blocks, %.2f records per block"
                         % (int(v["record_bytes"]), int(v["record_bytes"]) / int(v["pixels"]), ch, int(v["blocks"]), (int(v["record_bytes"]) / 4 - int(v["blocks"])) / int(v["blocks"])))
        lines.append("")
    if os.path.exists("/dev/kfd"):
        import importlib
        capi = importlib.import_module("dvp-mvs_amd").get_capi()
        lines.append("device (MI355X), one thread, median of 5 after a warm-up call (ms):")
        for what in ("dvp_jpeg_decode 1 channel", "dvp_jpeg_decode 3 channels", "dvp_jpeg_decode_into_store + host copy", "dvp_jpeg_decode_into_store"):
            host, dev = [], []
            for k in range(6):
                if what.startswith("dvp_jpeg_decode"):
                    capi.jpeg_decode(data, 1 if "1 channel" in what else 3)
                else:
                    store = capi.ImageStore()
                    store.put_jpeg(0, data, want_plane="copy" in what)
                    store.close()
                t = capi.jpeg_decode_timings()
                if k:
                    host.append(t["host_ms"])
                    dev.append(t["device_ms"])
            lines.append("  %-32s host part (parse + entropy decode) %.1f   device part (upload, launches, read-back, wait) %.1f   records %.1f MB"
                         % (what + ":", statistics.median(host), statistics.median(dev), t["record_bytes"] / 1e6))
        lines.append("  per-kernel times: not split here (rocprofv3 --kernel-trace --stats in a run of its own)")
    else:
        lines.append("device: not measured on the device (no GPU where this file was written)")
    text = "\n".join(lines) + "\n"
    if not device_only:
        open(out_file, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
