"""The parallel Huffman scan's shared text without a GPU: tests/jpeg_huff_host builds csrc/dvp_jpeg_huff.hpp beside
csrc/dvp_jpeg_dec_mid.hpp for the host into a stand-alone program under the address and undefined-behaviour sanitizers and runs the
passes of the device path (guesses, synchronisation inside the chunks, rounds across them, census, count, scans, write) with serial
loops over the lanes, in forward and in reverse lane order within a step.  On every file of jpeg_dec_cases.CASES and on the
additional files of jpeg_huff_cases — more than two chunks, a stuffed pair across a subsequence boundary, segments shorter than a
subsequence, a partial last segment, one MCU, blocks of one record, 4:2:2 and grey, optimised tables — the offsets and records
equal Decoder::scan's word for word, with all components and with the luma alone, and the path taken is the parallel one; a
damaged file is left to the serial scan or gives its words; a round cap of 0 makes a multi-chunk file fall back."""
import os
import subprocess

import pytest

import jpeg_dec_cases as JC
import jpeg_huff_cases as HC

pytestmark = pytest.mark.hostbox

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_huff_host")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", _HERE])
    return os.path.join(_HERE, "jpeg_huff_host")


def check(exe, tmp_path, data, luma_only=False, subseq=HC.SUBSEQ, cap=8):
    """(return code, the words of the program's line as a dict)"""
    f = str(tmp_path / "a.jpg")
    open(f, "wb").write(data)
    r = subprocess.run([exe, "check", f, str(subseq), "1" if luma_only else "0", str(cap)], capture_output=True, text=True)
    words = r.stdout.split()
    assert r.returncode in (0, 3) and len(words) == 20, r.stdout + r.stderr
    return r.returncode, dict(zip(words[0::2], words[1::2])), r.stderr


@pytest.mark.parametrize("case", JC.CASES, ids=JC.case_id)
def test_parallel_scan_equals_the_serial_scan(exe, tmp_path, case):
    for luma_only in (False, True):
        rc, said, err = check(exe, tmp_path, JC.jpeg_bytes(*case), luma_only)
        assert rc == 0 and said["path"] == "device" and said["serial"] == "ok", (said, err)


@pytest.mark.parametrize("name", sorted(HC.ADDITIONAL))
def test_additional_files(exe, tmp_path, name):
    data = HC.additional(name)
    for luma_only in (False, True):
        rc, said, err = check(exe, tmp_path, data, luma_only)
        assert rc == 0 and said["path"] == "device" and said["serial"] == "ok", (said, err)
    lanes, segs = int(said["subsequences"]), int(said["segments"])
    if name == "multi_chunk":
        assert segs == 1 and int(said["chunks"]) > 2 and int(said["rounds"]) >= 1 and lanes > 2 * HC.CHUNK, said
    if name.startswith("tiny_segments"):
        assert segs == lanes == 64 if name.endswith("grey") else segs == lanes == 16, said      # one subsequence per segment
        assert all(b - a < HC.SUBSEQ for a, b in HC.segments(data))
    if name == "partial_last_segment":
        assert segs == 21 and (16 * 9) % 7 == 4, said      # 144 MCUs in intervals of 7: the last holds 4
    if name.startswith("single_mcu"):
        assert segs == lanes == 1, said
    if name in ("flat_blocks", "constant_blocks"):
        blocks = {"flat_blocks": 32 * 17 * 6 // 2, "constant_blocks": 32 * 17 * 3}[name]
        assert blocks > 12 * lanes, (said, blocks)       # a dozen blocks and more per subsequence on average


def test_a_stuffed_pair_across_a_subsequence_boundary(exe, tmp_path):
    name, data = HC.straddling_file()
    assert HC.stuffing_straddles(data) > 0, name
    for luma_only in (False, True):
        rc, said, err = check(exe, tmp_path, data, luma_only)
        assert rc == 0 and said["path"] == "device" and int(said["straddles"]) == HC.stuffing_straddles(data) > 0, (name, said, err)


@pytest.mark.parametrize("subseq", [64, 256])
def test_other_subsequence_sizes(exe, tmp_path, subseq):
    for case in JC.RECORD_CASES + [HC.ADDITIONAL["multi_chunk"][0]]:
        rc, said, err = check(exe, tmp_path, JC.jpeg_bytes(*case), subseq=subseq)
        assert rc == 0 and said["path"] == "device", (case, said, err)


def test_the_larger_file(exe, tmp_path):
    rc, said, err = check(exe, tmp_path, JC.jpeg_bytes(*HC.LARGE))
    assert rc == 0 and said["path"] == "device" and int(said["chunks"]) > 32 and int(said["rounds"]) < 8, (said, err)


def test_a_round_cap_of_zero_falls_back(exe, tmp_path):
    rc, said, err = check(exe, tmp_path, HC.additional("multi_chunk"), cap=0)
    assert rc == 0 and said["path"] == "fellback" and said["why"] == "round_cap", (said, err)


@pytest.mark.parametrize("name", sorted(JC.rejected_files()))
def test_a_rejected_file_is_left_to_the_serial_scan(exe, tmp_path, name):
    data, message = JC.rejected_files()[name]
    rc, said, err = check(exe, tmp_path, data)
    assert rc == 0 and said["path"] in ("host", "fellback") and said["serial"] == message.replace(" ", "_"), (said, err)


@pytest.mark.parametrize("name", sorted(HC.damaged_files()))
def test_a_damaged_file_never_gives_other_words(exe, tmp_path, name):
    """exit 0 is the whole claim: the emulation left the file to the serial scan, or gave exactly its words"""
    for luma_only in (False, True):
        rc, said, err = check(exe, tmp_path, HC.damaged_files()[name], luma_only)
        assert rc == 0, (said, err)
        if said["serial"] != "ok":
            assert said["path"] != "device", said
