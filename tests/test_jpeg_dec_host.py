"""The input JPEG decoder's shared text without a GPU: tests/jpeg_dec_host builds csrc/dvp_jpeg_dec_mid.hpp (parse + entropy decode
-> coefficient records) and csrc/dvp_jpeg_dec.hpp (block and pixel arithmetic) for the host into a stand-alone program under the
address and undefined-behaviour sanitizers and runs them block after block and pixel after pixel.  On the files of
jpeg_dec_cases.CASES its output equals the host mirror's DecodeJpeg (grey and B, G, R, every pixel) and its grey output equals
libjpeg's luma; the records, densified and dequantised, are the coefficients of a dense decode of the same scan; the pictures hold
what they were built for; and a damaged file is refused with the host mirror's message and leaves no output."""
import os
import subprocess

import numpy as np
import pytest

import jpeg_dec_cases as JC
from conftest import ROOT

pytestmark = pytest.mark.hostbox

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_dec_host")
_MIRROR = os.path.join(ROOT, "tests", "host", "test_host")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", _HERE])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "host")])
    return os.path.join(_HERE, "jpeg_dec_host")


def _image(f):
    raw = open(f, "rb").read()
    rows, cols, ch = np.frombuffer(raw[:12], np.int32)
    return np.frombuffer(raw[12:], np.uint8).reshape(rows, cols, ch)


@pytest.mark.parametrize("case", JC.CASES, ids=JC.case_id)
def test_serial_text_equals_the_host_mirror_and_libjpeg(exe, tmp_path, case):
    data = JC.jpeg_bytes(*case)
    f = str(tmp_path / "a.jpg")
    open(f, "wb").write(data)
    for ch in (1, 3):
        mine, mirror = str(tmp_path / ("mine%d.bin" % ch)), str(tmp_path / ("mirror%d.bin" % ch))
        r = subprocess.run([exe, "decode", f, mine, str(ch)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([_MIRROR, "--jpeg", f, mirror, str(ch)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        a, b = _image(mine), _image(mirror)
        assert a.shape == (case[2], case[1], ch) and a.shape == b.shape and np.array_equal(a, b)
        if ch == 1:
            assert np.array_equal(a[:, :, 0], JC.libjpeg_luma(data))


def _records(exe, tmp_path, case):
    f, out = str(tmp_path / "a.jpg"), str(tmp_path / "records.bin")
    open(f, "wb").write(JC.jpeg_bytes(*case))
    r = subprocess.run([exe, "records", f, out], capture_output=True, text=True)
    words = r.stdout.split()
    return r, dict(zip(words[0::2], (int(w) for w in words[1::2]))), out


@pytest.mark.parametrize("case", JC.RECORD_CASES, ids=JC.case_id)
def test_records_give_the_dense_decoders_coefficients(exe, tmp_path, case):
    r, stats, out = _records(exe, tmp_path, case)
    assert r.returncode == 0 and stats["differ"] == 0, r.stdout + r.stderr
    raw = np.frombuffer(open(out, "rb").read(), np.int32)
    n = int(raw[0])
    assert n == (1 if case[0] == "grey" else 3)
    blocks = sum(int(raw[1 + 2 * i]) * int(raw[2 + 2 * i]) for i in range(n))
    assert blocks == stats["blocks"] and raw.size == 1 + 2 * n + blocks * 64
    coef = raw[1 + 2 * n:].reshape(blocks, 64)
    assert (coef != 0).any(axis=1).sum() > blocks // 2     # (the comparison was not of zeros with zeros)
    # at least one record per block, at most 64, and the offsets cost 4 bytes per block
    assert stats["min_records"] >= 1 and stats["max_records"] <= 64 and stats["record_bytes"] >= 8 * blocks


def test_the_pictures_hold_what_they_were_built_for(exe, tmp_path):
    """both clamps fire; some block has one record and some block more than 32; some DC prediction is 0"""
    r, noise, _ = _records(exe, tmp_path, ("444", 250, 130, 0, 100, "noise"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert noise["clamp_low"] > 0 and noise["clamp_high"] > 0 and noise["max_records"] > 32, noise
    r, flat, _ = _records(exe, tmp_path, ("420", 250, 130, 0, 75, "flat"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert flat["min_records"] == 1 and flat["max_records"] > 32 and flat["zero_dc"] > 0, flat
    # ... and every sampling, size, restart interval, quality and picture is in the shared list
    for k, values in enumerate((JC.SAMPLINGS, None, None, JC.RESTARTS, JC.QUALITIES, JC.PICTURES)):
        if values:
            assert {c[k] for c in JC.CASES} == set(values)
    assert {(c[1], c[2]) for c in JC.CASES} == set(JC.SIZES)
    for s in JC.SAMPLINGS:
        assert {(c[1], c[2]) for c in JC.CASES if c[0] == s} == set(JC.SIZES)


@pytest.mark.parametrize("name", sorted(JC.rejected_files()))
def test_a_damaged_file_is_refused_with_the_host_mirrors_message(exe, tmp_path, name):
    data, message = JC.rejected_files()[name]
    f = str(tmp_path / "bad.jpg")
    open(f, "wb").write(data)
    for ch in (1, 3):
        out = str(tmp_path / ("out%d.bin" % ch))
        r = subprocess.run([exe, "decode", f, out, str(ch)], capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.strip().endswith(": " + message), r.stdout + r.stderr
        assert not os.path.exists(out)
        m = subprocess.run([_MIRROR, "--jpeg", f, str(tmp_path / "m.bin"), str(ch)], capture_output=True, text=True)
        assert m.returncode == 2 and message in m.stderr, m.stdout + m.stderr
