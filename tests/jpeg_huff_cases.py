"""The files the parallel-Huffman-scan tests share beyond jpeg_dec_cases.CASES (tests/test_jpeg_huff_host.py on the host,
tests/test_gpu_jpeg_entropy.py on the device): written with PIL or cut out of such files, none committed.  SUBSEQ is the
subsequence size the device path runs with (csrc/dvp_jpeg_huff.hpp kSubseqBytes), CHUNK the subsequences per chunk."""
import jpeg_dec_cases as JC

SUBSEQ = 128
CHUNK = 256

# name -> (case, extra keywords of PIL's save)
ADDITIONAL = {
    "multi_chunk": (("420", 250, 130, 0, 100, "noise"), {}),          # one segment of about 70 KB: more than two chunks
    "tiny_segments_420": (("420", 64, 64, 1, 75, "ramp"), {}),         # every segment shorter than a subsequence
    "tiny_segments_grey": (("grey", 64, 64, 1, 75, "noise"), {}),
    "partial_last_segment": (("420", 250, 130, 7, 75, "noise"), {}),   # 144 MCUs in intervals of 7: the last holds 4
    "single_mcu_1x1": (("444", 1, 1, 0, 75, "noise"), {}),
    "single_mcu_8x8": (("grey", 8, 8, 0, 95, "noise"), {}),
    "flat_blocks": (("420", 250, 130, 0, 75, "flat"), {}),             # blocks of one record: dozens of blocks per subsequence
    "constant_blocks": (("444", 250, 130, 0, 75, "constant"), {}),
    "sampling_422": (("422", 250, 130, 0, 95, "noise"), {}),
    "grey_one_block_per_mcu": (("grey", 250, 130, 0, 95, "noise"), {}),
    "optimised_tables": (("420", 250, 130, 0, 75, "noise"), dict(optimize=True)),   # the tables are the file's own, not the standard ones
    "optimised_tables_restarts": (("444", 64, 64, 7, 95, "checker"), dict(optimize=True)),
}
LARGE = ("420", 1552, 1032, 0, 95, "noise")    # the only larger shape

_MADE = {}


def additional(name):
    if name not in _MADE:
        case, more = ADDITIONAL[name]
        _MADE[name] = JC.jpeg_bytes(*case, **more)
    return _MADE[name]


def scan_span(data):
    """(first, end) of the entropy-coded bytes: behind the SOS segment, up to the marker that ends the scan"""
    i = data.index(b"\xff\xda")
    first = i + 2 + ((data[i + 2] << 8) | data[i + 3])
    p = first
    while p + 1 < len(data):
        if data[p] == 0xFF and data[p + 1] != 0 and not 0xD0 <= data[p + 1] <= 0xD7:
            return first, p
        p += 1
    return first, len(data)


def segments(data):
    """[(first, end)] of the stretches between RSTn markers"""
    first, end = scan_span(data)
    out, p, start = [], first, first
    while p + 1 < end:
        if data[p] == 0xFF and 0xD0 <= data[p + 1] <= 0xD7:
            out.append((start, p))
            start = p = p + 2
        else:
            p += 1
    out.append((start, end))
    return out


def stuffing_straddles(data, subseq=SUBSEQ):
    """0xFF 0x00 pairs whose zero is the first byte of a subsequence"""
    n = 0
    for a, b in segments(data):
        for o in range(a + subseq, b, subseq):
            n += data[o] == 0 and data[o - 1] == 0xFF
    return n


def straddling_file():
    """(name, bytes) of the first file of a fixed search whose scan has a stuffed pair across a subsequence boundary"""
    if "straddle" not in _MADE:
        for q in (100, 95):
            for W, H in ((250, 130), (130, 250), (64, 64), (200, 100)):
                for s in ("420", "444", "grey"):
                    data = JC.jpeg_bytes(s, W, H, 0, q, "noise")
                    if stuffing_straddles(data):
                        _MADE["straddle"] = ("%s-%dx%d-q%d" % (s, W, H, q), data)
                        return _MADE["straddle"]
        raise AssertionError("no file of the search has a stuffed pair across a subsequence boundary")
    return _MADE["straddle"]


# ---- damaged files: a well-formed file with ... -----------------------------------------------------------------------------------
def flipped_byte(data):
    """one entropy byte flipped mid-scan"""
    first, end = scan_span(data)
    p = (first + end) // 2
    while data[p] in (0x00, 0xFF) or data[p - 1] == 0xFF:     # (not a stuffed pair, not a marker)
        p += 1
    return data[:p] + bytes([data[p] ^ 0x5A]) + data[p + 1:]


def without_one_restart(data):
    """an RSTn removed"""
    seg = segments(data)
    assert len(seg) > 2
    a = seg[len(seg) // 2][1]          # the marker behind the middle segment
    assert data[a] == 0xFF and 0xD0 <= data[a + 1] <= 0xD7
    return data[:a] + data[a + 2:]


def doubled_segment(data):
    """a segment's bytes, with the marker behind them, twice"""
    seg = segments(data)
    assert len(seg) > 2
    a, b = seg[len(seg) // 2]
    return data[:b + 2] + data[a:b + 2] + data[b + 2:]


def cut_short(data):
    """the last 40 % cut off"""
    return data[:len(data) * 6 // 10]


def damaged_files():
    """name -> bytes"""
    plain = JC.jpeg_bytes("420", 250, 130, 0, 75, "noise")
    restarts = JC.jpeg_bytes("420", 250, 130, 7, 75, "noise")
    return {
        "flipped_byte": flipped_byte(plain),
        "flipped_byte_restarts": flipped_byte(restarts),
        "restart_removed": without_one_restart(restarts),
        "segment_doubled": doubled_segment(restarts),
        "cut_short": cut_short(plain),
        "cut_short_restarts": cut_short(restarts),
    }
