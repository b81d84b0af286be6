"""The input JPEGs reconstructed on the device (csrc/dvp_jpeg_dec.hip: dvp_jpeg_decode, dvp_jpeg_decode_into_store) against the host
mirror's DecodeJpeg, byte for byte: the files of jpeg_dec_cases.CASES with one and three channels; the luma plane put straight
into an image store against dvp_images_put of the host-decoded plane (the level at the image's own size, bitwise, and the plane
that comes back); one store across sizes that grow and shrink; two threads at once; the argument checks; rejected files, which
leave the store as it was and carry the host path's message; one 1552 x 1032 file; and DVP_TEST_SIDE_ALLOC_FAIL over the powers
of two."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import jpeg_dec_cases as JC
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

_MIRROR = os.path.join(ROOT, "tests", "host", "test_host")
VAR = "DVP_TEST_SIDE_ALLOC_FAIL"
REFUSED = "out of device memory"
_FILES, _HOST = {}, {}


def capi():
    return pkg().get_capi()


def data_of(case):
    if case not in _FILES:
        _FILES[case] = JC.jpeg_bytes(*case)
    return _FILES[case]


def host_decode(case, channels, tmp_path_factory):
    """the host mirror's DecodeJpeg of the case's file, made once per (case, channels) and left unchanged"""
    key = (case, channels)
    if key not in _HOST:
        d = tmp_path_factory.mktemp("mirror")
        f, out = str(d / "a.jpg"), str(d / "a.bin")
        open(f, "wb").write(data_of(case))
        r = subprocess.run([_MIRROR, "--jpeg", f, out, str(channels)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(out, "rb").read()
        rows, cols, ch = np.frombuffer(raw[:12], np.int32)
        a = np.frombuffer(raw[12:], np.uint8).reshape((rows, cols) if ch == 1 else (rows, cols, 3))
        a.flags.writeable = False
        _HOST[key] = a
    return _HOST[key]


@pytest.mark.parametrize("case", JC.CASES, ids=JC.case_id)
def test_decode_equals_the_host_mirror(case, tmp_path_factory):
    for ch in (1, 3):
        want = host_decode(case, ch, tmp_path_factory)
        assert capi().jpeg_size(data_of(case), ch) == (case[1], case[2])
        got = capi().jpeg_decode(data_of(case), ch)
        assert got.shape == want.shape and np.array_equal(got, want), (ch, int((got != want).sum()))


def own_level(store, image_id):
    w, h = store.size(image_id)
    return store.level(image_id, w, h)


@pytest.mark.parametrize("case", JC.CASES, ids=JC.case_id)
def test_put_jpeg_equals_put_of_the_host_plane(case, tmp_path_factory):
    want = host_decode(case, 1, tmp_path_factory)
    a, b = capi().ImageStore(), capi().ImageStore()
    try:
        plane = a.put_jpeg(3, data_of(case), want_plane=True)
        b.put(3, want)
        assert np.array_equal(plane, want)
        assert a.size(3) == b.size(3) == (case[1], case[2]) and a.bytes() == b.bytes() == case[1] * case[2]
        la, lb = own_level(a, 3), own_level(b, 3)
        assert la.tobytes() == lb.tobytes() and np.array_equal(la, want.astype(np.float32))
        assert a.put_jpeg(4, data_of(case)) is None and own_level(a, 4).tobytes() == lb.tobytes()     # without the host copy
    finally:
        a.close()
        b.close()


def test_one_store_across_sizes_that_grow_and_shrink(tmp_path_factory):
    cases = [("420", 64, 64, 0, 75, "noise"), ("420", 250, 130, 7, 75, "noise"), ("grey", 515, 259, 0, 30, "ramp"), ("422", 17, 33, 1, 95, "flat"), ("444", 8, 8, 0, 75, "noise")]
    store = capi().ImageStore()
    try:
        held = 0
        for k, case in enumerate(cases):           # one id replaced again and again, and an id of its own per size
            if k:
                store.drop(0)
                held -= cases[k - 1][1] * cases[k - 1][2]
            store.put_jpeg(0, data_of(case))
            store.put_jpeg(10 + k, data_of(case))
            held += 2 * case[1] * case[2]
            assert store.bytes() == held
        for k, case in enumerate(cases):
            fresh = capi().ImageStore()
            fresh.put(0, host_decode(case, 1, tmp_path_factory))
            want = own_level(fresh, 0)
            fresh.close()
            assert own_level(store, 10 + k).tobytes() == want.tobytes()
            if k == len(cases) - 1:
                assert own_level(store, 0).tobytes() == want.tobytes()
    finally:
        store.close()


def test_two_threads_decode_different_files_at_once(tmp_path_factory):
    cases = [("420", 515, 259, 7, 75, "noise"), ("444", 250, 130, 0, 100, "noise")]
    want = [[host_decode(c, ch, tmp_path_factory) for ch in (1, 3)] for c in cases]
    bad = []

    def work(k):
        try:
            for _ in range(4):
                for i, ch in enumerate((1, 3)):
                    if not np.array_equal(capi().jpeg_decode(data_of(cases[k]), ch), want[k][i]):
                        bad.append((k, ch))
        except Exception as e:     # noqa: BLE001 (reported below)
            bad.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad


def test_argument_checks():
    L = capi().lib()
    data = np.frombuffer(data_of(("420", 64, 64, 0, 75, "noise")), np.uint8)
    out = np.zeros((64, 64 * 3), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    err = lambda: L.dvp_jpeg_decode_last_error().decode()
    assert L.dvp_jpeg_decode(0, None, data.size, 1, p(out), 64, None, None) != 0 and "required" in err()
    assert L.dvp_jpeg_decode(0, p(data), 0, 1, p(out), 64, None, None) != 0 and "required" in err()
    assert L.dvp_jpeg_decode(0, p(data), -5, 1, p(out), 64, None, None) != 0 and "required" in err()
    assert L.dvp_jpeg_decode(0, p(data), data.size, 2, p(out), 192, None, None) != 0 and "channels" in err()
    assert L.dvp_jpeg_decode(0, p(data), data.size, 1, p(out), 63, None, None) != 0 and "pitch" in err()
    assert L.dvp_jpeg_decode(0, p(data), data.size, 3, p(out), 191, None, None) != 0 and "pitch" in err()
    assert not out.any()
    # no output: the size alone, and the device is not touched — a device that does not exist is no error
    assert L.dvp_jpeg_decode(12345, p(data), data.size, 3, None, 0, ctypes.byref(w), ctypes.byref(h)) == 0 and (w.value, h.value) == (64, 64) and err() == ""
    assert L.dvp_jpeg_decode(12345, p(data), data.size, 1, p(out), 64, None, None) != 0 and "hipSetDevice" in err()
    # a wider pitch leaves the bytes between the rows alone
    out[:] = 7
    assert L.dvp_jpeg_decode(0, p(data), data.size, 1, p(out), 192, ctypes.byref(w), ctypes.byref(h)) == 0, err()
    assert np.array_equal(out[:, :64], capi().jpeg_decode(data.tobytes(), 1)) and (out[:, 64:] == 7).all()
    store = capi().ImageStore()
    try:
        assert L.dvp_jpeg_decode_into_store(None, 0, p(data), data.size, None, 0) != 0 and "store" in err()
        assert L.dvp_jpeg_decode_into_store(store.h, 0, None, data.size, None, 0) != 0 and "required" in err()
        assert L.dvp_jpeg_decode_into_store(store.h, 0, p(data), 0, None, 0) != 0 and "required" in err()
        assert L.dvp_jpeg_decode_into_store(store.h, 0, p(data), data.size, p(out), 63) != 0 and "pitch" in err()
        assert store.bytes() == 0
    finally:
        store.close()


@pytest.mark.parametrize("name", sorted(JC.rejected_files()))
def test_a_rejected_file_leaves_the_store_as_it_was(name, tmp_path_factory):
    data, message = JC.rejected_files()[name]
    good = ("444", 16, 16, 0, 75, "noise")
    for ch in (1, 3):
        with pytest.raises(capi().DvpError, match="dvp_jpeg_decode: ") as e:
            capi().jpeg_decode(data, ch)
        assert message in str(e.value)
    store = capi().ImageStore()
    try:
        store.put_jpeg(5, JC.jpeg_bytes(*good))
        before = (store.bytes(), own_level(store, 5).tobytes())
        with pytest.raises(capi().DvpError) as e:
            store.put_jpeg(6, data)
        assert message in str(e.value)
        with pytest.raises(capi().DvpError, match="already in the store"):
            store.put_jpeg(5, JC.jpeg_bytes(*good))
        with pytest.raises(capi().DvpError, match="not in the store"):
            store.size(6)
        assert (store.bytes(), own_level(store, 5).tobytes()) == before
    finally:
        store.close()


def test_a_1552_x_1032_file(tmp_path_factory):
    case = ("420", 1552, 1032, 0, 90, "noise")
    for ch in (1, 3):
        assert np.array_equal(capi().jpeg_decode(data_of(case), ch), host_decode(case, ch, tmp_path_factory))
    store = capi().ImageStore()
    try:
        assert np.array_equal(store.put_jpeg(1, data_of(case), want_plane=True), host_decode(case, 1, tmp_path_factory))
    finally:
        store.close()


def test_refused_allocations(monkeypatch, tmp_path_factory):
    """every threshold either refuses with `out of device memory` or changes nothing; afterwards the same store works"""
    case = ("420", 250, 130, 7, 75, "noise")
    monkeypatch.delenv(VAR, raising=False)
    want = {ch: host_decode(case, ch, tmp_path_factory) for ch in (1, 3)}
    store = capi().ImageStore()
    try:
        refused, t, next_id = 0, 1, 0
        while t <= 4 << 20:      # (the colour call's pool is below 1 MB: the last thresholds refuse nothing)
            for call in ("decode1", "decode3", "put"):
                monkeypatch.setenv(VAR, str(t))
                held = store.bytes()
                try:
                    if call == "put":
                        got, error = store.put_jpeg(next_id, data_of(case), want_plane=True), None
                    else:
                        got, error = capi().jpeg_decode(data_of(case), int(call[-1])), None
                except capi().DvpError as e:
                    got, error = None, str(e)
                monkeypatch.delenv(VAR)
                if error is None:
                    assert t > 1 and np.array_equal(got, want[3 if call == "decode3" else 1]), (t, call)
                else:
                    assert REFUSED in error and t < 4 << 20, (t, call, error)
                    refused += 1
                    assert store.bytes() == held
                if call == "put":
                    if error is not None:      # the same store, the same id: works once the variable is gone
                        assert np.array_equal(store.put_jpeg(next_id, data_of(case), want_plane=True), want[1])
                    assert own_level(store, next_id).tobytes() == want[1].astype(np.float32).tobytes()
                    store.drop(next_id)
                    next_id += 1
            t *= 2
        assert refused >= 3
    finally:
        monkeypatch.delenv(VAR, raising=False)
        store.close()
