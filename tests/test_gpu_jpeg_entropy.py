"""The input JPEGs' Huffman scan on the device (csrc/dvp_jpeg_huff.hip behind dvp_jpeg_set_entropy(1), `apd --entropy-on gpu`) against
the host's serial scan: the coefficient records of dvp_jpeg_scan_records word for word, and dvp_jpeg_decode with 1 and 3 channels and
dvp_jpeg_decode_into_store byte for byte against the same calls with the switch off — on every file of jpeg_dec_cases.CASES and on
the additional files of jpeg_huff_cases (more than two chunks, a stuffed pair across a subsequence boundary, segments shorter than
a subsequence, a partial last segment, one MCU, blocks of one record, 4:2:2 and grey, optimised tables), each of which takes the
device path without falling back.  Rejected files carry the host's message; damaged files (a flipped byte, a restart marker
removed, a segment doubled, the tail cut off) end as on the host, message or bytes; a round cap of 0 makes a multi-chunk file fall
back to the host's bytes; refused allocations leave `out of device memory` or the host's bytes; two threads decode at once; one
1552 x 1032 file is the only larger shape."""
import contextlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import jpeg_dec_cases as JC
import jpeg_huff_cases as HC
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

VAR = "DVP_TEST_SIDE_ALLOC_FAIL"
REFUSED = "out of device memory"
_FILES = {("case",) + c: None for c in JC.CASES}
_FILES.update({("more", n): None for n in HC.ADDITIONAL})
_FILES[("straddle",)] = None
_HOST = {}


def capi():
    return pkg().get_capi()


def file_id(key):
    return JC.case_id(key[1:]) if key[0] == "case" else "-".join(key)


def data_of(key):
    if _FILES.get(key) is None:
        _FILES[key] = JC.jpeg_bytes(*key[1:]) if key[0] == "case" else HC.additional(key[1]) if key[0] == "more" else HC.straddling_file()[1]
    return _FILES[key]


@contextlib.contextmanager
def entropy_on_device():
    """the switch is process-wide: it is off again when the block is left, however it is left"""
    capi().jpeg_set_entropy(True)
    try:
        yield
    finally:
        capi().jpeg_set_entropy(False)


def outcome(call):
    """("bytes", the result's bytes and shape) or ("error", the message)"""
    try:
        a = call()
        return ("bytes", None if a is None else (a.shape, a.tobytes()))
    except capi().DvpError as e:
        return ("error", str(e))


def decode_outcomes(data):
    """what the three decode calls leave for a file: the two images, and the plane and the level of a put into a fresh store"""
    out = [outcome(lambda: capi().jpeg_decode(data, 1)), outcome(lambda: capi().jpeg_decode(data, 3))]
    store = capi().ImageStore()
    try:
        out.append(outcome(lambda: store.put_jpeg(2, data, want_plane=True)))
        if out[-1][0] == "bytes":
            w, h = store.size(2)
            out.append(("level", store.level(2, w, h).tobytes()))
            out.append(outcome(lambda: store.put_jpeg(3, data)))       # without the host copy
            out.append(("level", store.level(3, w, h).tobytes()))
        out.append(("held", store.bytes()))
    finally:
        store.close()
    return out


def host_outcomes(key, data=None):
    """... with the switch off: made once per file and left unchanged"""
    if key not in _HOST:
        capi().jpeg_set_entropy(False)
        _HOST[key] = decode_outcomes(data_of(key) if data is None else data)
    return _HOST[key]


def same_records(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])) for x, y in zip(a, b))


@pytest.mark.parametrize("key", list(_FILES), ids=file_id)
def test_records_and_images_equal_the_hosts(key):
    data = data_of(key)
    if key[0] == "straddle":
        assert HC.stuffing_straddles(data) > 0
    for luma_only in (False, True):
        want = capi().jpeg_scan_records(data, luma_only, on_device=False)
        assert capi().jpeg_entropy_stats()["path"] == "host"
        got = capi().jpeg_scan_records(data, luma_only, on_device=True)
        stats = capi().jpeg_entropy_stats()
        assert stats["path"] == "device", stats
        assert same_records(got, want), (luma_only, stats)
        assert all(w is not None for w in want) if not luma_only else all(w is None for w in want[1:])
        segs = HC.segments(data)
        assert stats["segments"] == len(segs) and stats["subsequences"] == sum(-(-(b - a) // HC.SUBSEQ) for a, b in segs), stats
        assert stats["chunks"] == -(-stats["subsequences"] // HC.CHUNK) and stats["uploaded_bytes"] < len(data) + 20 * stats["subsequences"] + 4096, stats
    want = host_outcomes(key)
    with entropy_on_device():
        got = decode_outcomes(data)
        assert capi().jpeg_entropy_stats()["path"] == "device"
    assert got == want and all(kind != "error" for kind, _ in want)
    if key == ("more", "multi_chunk"):
        assert stats["segments"] == 1 and stats["chunks"] > 2 and stats["rounds"] >= 1, stats
    if key[0] == "more" and (key[1].startswith("tiny_segments") or key[1].startswith("single_mcu")):
        assert stats["segments"] == stats["subsequences"], stats      # one subsequence per segment


def test_the_larger_file():
    data = JC.jpeg_bytes(*HC.LARGE)
    want = capi().jpeg_scan_records(data, False, on_device=False)
    got = capi().jpeg_scan_records(data, False, on_device=True)
    stats = capi().jpeg_entropy_stats()
    assert stats["path"] == "device" and stats["chunks"] > 32 and stats["rounds"] < 8 and stats["longest_chain"] <= HC.CHUNK, stats
    assert same_records(got, want)
    want = host_outcomes(("large",), data)
    with entropy_on_device():
        assert decode_outcomes(data) == want
        assert capi().jpeg_entropy_stats()["path"] == "device"


@pytest.mark.parametrize("name", sorted(JC.rejected_files()))
def test_a_rejected_file_carries_the_hosts_message(name):
    data, message = JC.rejected_files()[name]
    want = host_outcomes(("rejected", name), data)
    with entropy_on_device():
        got = decode_outcomes(data)
        for ch in (1, 3):
            with pytest.raises(capi().DvpError, match="dvp_jpeg_decode: ") as e:
                capi().jpeg_decode(data, ch)
            assert message in str(e.value)
        assert capi().jpeg_entropy_stats()["path"] != "device"
    assert got == want and got[0][0] == got[1][0] == got[2][0] == "error" and got[-1] == ("held", 0)
    with pytest.raises(capi().DvpError) as e:
        capi().jpeg_scan_records(data, False, on_device=True)
    assert message in str(e.value)


@pytest.mark.parametrize("name", sorted(HC.damaged_files()))
def test_a_damaged_file_ends_as_on_the_host(name):
    data = HC.damaged_files()[name]
    want = host_outcomes(("damaged", name), data)
    with entropy_on_device():
        got = decode_outcomes(data)
    assert got == want
    for luma_only in (False, True):
        a = outcome_of_records(data, luma_only, False)
        b = outcome_of_records(data, luma_only, True)
        assert a[0] == b[0] and (a[1] == b[1] if a[0] == "error" else same_records(a[1], b[1]))
        if a[0] == "error":
            assert capi().jpeg_entropy_stats()["path"] != "device"


def outcome_of_records(data, luma_only, on_device):
    try:
        return ("records", capi().jpeg_scan_records(data, luma_only, on_device=on_device))
    except capi().DvpError as e:
        return ("error", str(e))


_CHILD = """
import importlib, sys
sys.path[:0] = [%r, %r]
import numpy as np
import jpeg_huff_cases as HC
capi = importlib.import_module("dvp-mvs_amd").get_capi()
data = HC.additional("multi_chunk")
host = [capi.jpeg_decode(data, ch) for ch in (1, 3)]
capi.jpeg_set_entropy(True)
for ch in (1, 3):
    got = capi.jpeg_decode(data, ch)
    stats = capi.jpeg_entropy_stats()
    print("channels", ch, "path", stats["path"].replace(" ", "_"), "chunks", stats["chunks"], "rounds", stats["rounds"], "equal", int(np.array_equal(got, host[ch // 2])))
"""


def test_a_round_cap_of_zero_falls_back_to_the_hosts_bytes():
    """DVP_TEST_JPEG_SYNC_CAP=0 in a child process: the multi-chunk file needs a round, gets none, and is decoded on the host"""
    env = dict(os.environ, DVP_TEST_JPEG_SYNC_CAP="0")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("channels")]
    assert len(lines) == 2, r.stdout + r.stderr
    for words in lines:
        said = dict(zip(words[0::2], words[1::2]))
        assert said["path"] == "fell_back" and int(said["chunks"]) > 2 and said["rounds"] == "0" and said["equal"] == "1", said


def test_refused_allocations(monkeypatch):
    """every threshold leaves `out of device memory` or the host's bytes, never anything else; afterwards all is as before"""
    key = ("case", "420", 250, 130, 7, 75, "noise")
    data = data_of(key)
    monkeypatch.delenv(VAR, raising=False)
    want = host_outcomes(key)
    paths = set()
    with entropy_on_device():
        try:
            refused, t = 0, 1
            while t <= 4 << 20:
                monkeypatch.setenv(VAR, str(t))
                got = decode_outcomes(data)
                paths.add(capi().jpeg_entropy_stats()["path"])
                monkeypatch.delenv(VAR)
                for g, w in zip(got[:3], want[:3]):
                    if g[0] == "error":
                        assert REFUSED in g[1] and t < 4 << 20, (t, g)
                        refused += 1
                    else:
                        assert g == w, t
                t *= 2
            assert refused >= 3 and "fell back" in paths and "device" in paths, (refused, paths)
        finally:
            monkeypatch.delenv(VAR, raising=False)
        assert decode_outcomes(data) == want and capi().jpeg_entropy_stats()["path"] == "device"


def test_two_threads_decode_different_files_at_once():
    keys = [("case", "420", 515, 259, 7, 75, "noise"), ("more", "multi_chunk")]
    want = [host_outcomes(k)[:2] for k in keys]
    bad = []

    def work(k):
        try:
            for _ in range(4):
                got = [outcome(lambda: capi().jpeg_decode(data_of(keys[k]), ch)) for ch in (1, 3)]
                if got != want[k] or capi().jpeg_entropy_stats()["path"] != "device":
                    bad.append((k, capi().jpeg_entropy_stats()))
        except Exception as e:     # noqa: BLE001 (reported below)
            bad.append((k, repr(e)))

    for k in keys:
        data_of(k)
    with entropy_on_device():
        threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not bad, bad


def test_the_switch_off_is_the_host_path():
    data = data_of(("case", "420", 250, 130, 0, 75, "noise"))
    capi().jpeg_set_entropy(False)
    capi().jpeg_decode(data, 3)
    stats = capi().jpeg_entropy_stats()
    assert stats["path"] == "host" and stats["subsequences"] == 0 and stats["uploaded_bytes"] == 0, stats
