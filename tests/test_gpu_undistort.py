"""`apd --convert-from ... --undistort on` on the device (csrc/dvp_undistort.hip): dvp_undistort_image leaves the bytes of the same
text run serially on the host (tests/undistort_host), no pixel skipped, for all ten accepted camera models at the widths one below,
at and past a wave and a work-group - where the tail of the repack through LDS can go wrong - and with padded input rows; zero
distortion is the identity; sources outside the picture read zero; the argument checks; two threads at once."""
import threading

import numpy as np
import pytest

import np_undistort as U
from conftest import pkg

pytestmark = pytest.mark.gpu


def capi():
    return pkg().get_capi()


@pytest.mark.parametrize("w,h", U.GPU_SIZES)
@pytest.mark.parametrize("model", U.MODELS)
def test_device_bytes_equal_the_serial_text(tmp_path_factory, model, w, h):
    want = U.serial_case(model, w, h, tmp_path_factory)
    got = capi().undistort_image(U.picture(w, h), model, U.params(model, w, h))
    assert got.dtype == np.uint8 and np.array_equal(got, want), np.argwhere((got != want).any(2))[:5]


@pytest.mark.parametrize("model,w,h", [("OPENCV", 67, 5), ("THIN_PRISM_FISHEYE", 257, 4), ("RADIAL", 129, 66)])
def test_padded_rows(tmp_path_factory, model, w, h):
    src = U.padded(U.picture(w, h))
    assert src.strides[0] == 3 * w + 9
    assert np.array_equal(capi().undistort_image(src, model, U.params(model, w, h)), U.serial_case(model, w, h, tmp_path_factory))


@pytest.mark.parametrize("model", U.NOT_FISHEYE)
def test_zero_distortion_is_the_identity(model):
    for w, h in ((65, 3), (257, 4)):
        src = U.picture(w, h)
        assert np.array_equal(capi().undistort_image(src, model, U.params(model, w, h, [0.0] * len(U.EXTRA[model]))), src)


def test_sources_outside_the_picture_read_zero():
    w, h = 129, 66
    p = U.params("RADIAL", w, h)
    sx, sy = U.source_coordinates("RADIAL", p, w, h)
    got = capi().undistort_image(U.picture(w, h), "RADIAL", p)
    outside = (sx < -1.1) | (sx > w + 0.1) | (sy < -1.1) | (sy > h + 0.1)
    assert outside.mean() >= 0.05 and not got[outside].any() and got[~outside].any()
    # a NaN coordinate: a zero pixel
    assert not capi().undistort_image(U.picture(65, 3), "SIMPLE_RADIAL", [float("nan"), 32.0, 1.5, 0.0]).any()


def test_argument_checks():
    C = capi()
    L = C.lib()
    src = U.picture(9, 5)
    good = U.params("OPENCV", 9, 5)
    out = np.zeros(135, np.uint8)
    with pytest.raises(C.DvpError, match="dvp_undistort_image: the FOV camera model is not supported"):
        C.undistort_image(src, "FOV", [5.0, 5.0, 4.5, 2.5, 0.9])
    with pytest.raises(C.DvpError, match="dvp_undistort_image: unknown camera model 11"):
        C.undistort_image(src, 11, good)
    with pytest.raises(C.DvpError, match="dvp_undistort_image: OPENCV takes 8 parameters, not 7"):
        C.undistort_image(src, "OPENCV", good[:7])
    for args, message in (((0, 5, 27), b"bad image geometry (sizes of 1 ... 65535)"), ((9, 65536, 27), b"bad image geometry"), ((9, 5, 26), b"the pitch is below 3 * width bytes")):
        w, h, pitch = args
        assert L.dvp_undistort_image(0, C._p(src), w, h, pitch, 4, C._p(good), 8, C._p(out)) != 0 and message in L.dvp_undistort_last_error()
    for a, p, o in ((None, C._p(good), C._p(out)), (C._p(src), None, C._p(out)), (C._p(src), C._p(good), None)):
        assert L.dvp_undistort_image(0, a, 9, 5, 27, 4, p, 8, o) != 0 and b"the picture, the parameters and the output are required" in L.dvp_undistort_last_error()
    # an error leaves the next call alone
    want, skip = U.undistort(src, "OPENCV", good)
    got = C.undistort_image(src, "OPENCV", good)
    assert not ((got != want).any(2) & ~skip).any() and L.dvp_undistort_last_error() == b""


def test_two_threads_undistort_at_once(tmp_path_factory):
    cases = [("THIN_PRISM_FISHEYE", 257, 4), ("RADIAL", 129, 66)]
    want = [U.serial_case(m, w, h, tmp_path_factory) for m, w, h in cases]
    bad = []

    def work(k):
        try:
            for _ in range(3):
                for (m, w, h), expected in zip(cases, want):
                    if not np.array_equal(capi().undistort_image(U.picture(w, h), m, U.params(m, w, h)), expected):
                        bad.append((k, m))
        except Exception as e:      # noqa: BLE001
            bad.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad
