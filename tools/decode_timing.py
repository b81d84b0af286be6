#!/usr/bin/env python3
"""Where the input JPEG decode spends its time, and what `apd --decode-on gpu` can move: writes profiles/decode_timing.txt.

Host part (needs no GPU): a 6208 x 4128 4:2:0 file is made here with PIL from a deterministic picture with texture, and
tools/decode_timing.cpp — the three parts of host/jpeg.cpp's DecodeJpeg from the shared headers — is built and run on it,
single-threaded, median of five: (a) marker parse + entropy decode, (b) inverse DCT + plane stores, (c) the colour loop; with
the bytes of coefficient records per pixel.

Device part (only where a GPU is present; else the file says "not measured on the device"): dvp_jpeg_decode and
dvp_jpeg_decode_into_store on the same file, their host part (parse + entropy decode) and device part (upload, launches, read-back, wait),
median of five after one warm-up call; then the same calls with the Huffman scan on the device as well (`apd --entropy-on gpu`,
dvp_jpeg_set_entropy(1)): wall time of each call with the switch off and on (unserialised), the path's statistics, and the split
over its phases from a serialised run (DVP_JPEG_ENTROPY_SERIAL=1: a wait after every phase), at subsequences of 128 and 256 bytes.
wall_lines(capi, data, why) with another checkout's package as `capi` measures that build's calls the same way (the parent
commit's, for the comparison in profiles/decode_timing.txt).
Per-kernel times want a run of their own:
    rocprofv3 --kernel-trace --stats -d /tmp/jd -- python tools/decode_timing.py --device-only
usage: decode_timing.py [--quality Q] [--size WxH] [--device-only] [--out FILE]"""
import io
import os
import statistics
import subprocess
import sys
import tempfile
import time
import ctypes

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


CALLS = ("dvp_jpeg_decode 1 channel", "dvp_jpeg_decode 3 channels", "dvp_jpeg_decode_into_store + host copy", "dvp_jpeg_decode_into_store")


def one_call(capi, data, what):
    """wall milliseconds of one call"""
    t0 = time.perf_counter()
    if what.startswith("dvp_jpeg_decode_into_store"):
        store = capi.ImageStore()
        t0 = time.perf_counter()
        store.put_jpeg(0, data, want_plane="copy" in what)
        t = time.perf_counter() - t0
        store.close()
        return t * 1e3
    L, f = capi.lib(), np.frombuffer(data, np.uint8)     # (straight through the C ABI, into a buffer made before the clock starts)
    ch = 1 if "1 channel" in what else 3
    W, H = capi.jpeg_size(data, ch)
    out = np.empty((H, W * ch), np.uint8)
    t0 = time.perf_counter()
    rc = L.dvp_jpeg_decode(0, f.ctypes.data_as(ctypes.c_void_p), f.size, ch, out.ctypes.data_as(ctypes.c_void_p), out.strides[0], None, None)
    t = time.perf_counter() - t0
    assert rc == 0, L.dvp_jpeg_decode_last_error()
    return t * 1e3


def wall(capi, data, what):
    """median of five after a warm-up call"""
    return statistics.median([one_call(capi, data, what) for _ in range(6)][1:])


def wall_lines(capi, data, why):
    out = ["", "wall time per call, median of 5 after a warm-up call (ms; %s):" % why]
    for what in CALLS:
        out.append("  %-40s %.1f" % (what + ":", wall(capi, data, what)))
    return out


def entropy_lines(capi, data):
    out = ["", "--entropy-on gpu (dvp_jpeg_set_entropy(1)): the Huffman scan on the device as well, same file, same session",
           "wall time per call, median of 5 after a warm-up call, unserialised (ms):",
           "  %-40s %10s %16s %16s" % ("", "switch off", "on, 128 bytes", "on, 256 bytes")]
    os.environ.pop("DVP_JPEG_ENTROPY_SERIAL", None)
    for what in CALLS:
        row = []
        for on, subseq in ((False, "128"), (True, "128"), (True, "256")):
            os.environ["DVP_JPEG_SUBSEQ_BYTES"] = subseq
            capi.jpeg_set_entropy(on)
            row.append(wall(capi, data, what))
            if on:
                assert capi.jpeg_entropy_stats()["path"] == "device", capi.jpeg_entropy_stats()
        out.append("  %-40s %10.1f %16.1f %16.1f" % ((what + ":",) + tuple(row)))
    out.append("statistics and the split over the phases (serialised: a wait after every phase; median of 5 after a warm-up call, ms):")
    os.environ["DVP_JPEG_ENTROPY_SERIAL"] = "1"
    capi.jpeg_set_entropy(True)
    for subseq in ("128", "256"):
        os.environ["DVP_JPEG_SUBSEQ_BYTES"] = subseq
        for what in ("dvp_jpeg_decode 1 channel", "dvp_jpeg_decode 3 channels"):
            runs = []
            for k in range(6):
                total = one_call(capi, data, what)
                runs.append(dict(capi.jpeg_entropy_phases(), total=total))
            st = capi.jpeg_entropy_stats()
            med = {k: statistics.median(r[k] for r in runs[1:]) for k in runs[0]}
            out.append("  %s, subsequences of %s bytes: %d subsequences in %d chunk(s), %d segment(s); longest chain %d, inter-chunk rounds %d, mean re-decodes per subsequence %.2f; uploaded %.1f MB"
                       % (what, subseq, st["subsequences"], st["chunks"], st["segments"], st["longest_chain"], st["rounds"], st["decodes"] / max(st["subsequences"], 1), st["uploaded_bytes"] / 1e6))
            out.append("      pre-scan %.2f   upload %.2f   synchronisation %.2f   census + count %.2f   scans %.2f   write %.2f   reconstruction %.2f   whole call %.1f"
                       % tuple(med[k] for k in capi.ENTROPY_PHASES + ("total",)))
    os.environ.pop("DVP_JPEG_ENTROPY_SERIAL", None)
    os.environ.pop("DVP_JPEG_SUBSEQ_BYTES", None)
    capi.jpeg_set_entropy(False)
    return out


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
            lines.append("          with --entropy-on gpu the host keeps: parse to the scan + pre-scan %.2f ms; uploads %d bytes (%d subsequences of 128 bytes in %d segment(s)) instead of the records"
                         % (float(v["prescan_ms"]), int(v["upload_bytes"]), int(v["subsequences"]), int(v["segments"])))
        lines.append("")
    if os.path.exists("/dev/kfd"):
        import importlib
        capi = importlib.import_module("dvp-mvs_amd").get_capi()
        lines.append("device (MI355X), one thread, median of 5 after a warm-up call (ms):")
        for what in ("dvp_jpeg_decode 1 channel", "dvp_jpeg_decode 3 channels", "dvp_jpeg_decode_into_store + host copy", "dvp_jpeg_decode_into_store"):
            host, dev = [], []
            for k in range(6):
                if what.startswith("dvp_jpeg_decode "):
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
        if hasattr(capi.lib(), "dvp_jpeg_set_entropy"):
            lines += entropy_lines(capi, data)
        else:
            lines += wall_lines(capi, data, "this build has no --entropy-on")
    else:
        lines.append("device: not measured on the device (no GPU where this file was written)")
    text = "\n".join(lines) + "\n"
    if not device_only:
        open(out_file, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
