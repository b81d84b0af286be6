"""`apd --convert-from` on the device (csrc/dvp_pairs.hip): dvp_view_scores is bit-identical to the same text run serially on the
host (tests/convert_host) on every shape at which the kernel can go wrong - two and three images, tracks one below, at and past a
wave and past two, multiplicities, S = 0, the count of small angles at and one above (3 * S) >> 2, a list that is all -1, a
cosine that rounds above 1 - and on 40 images x 2 000 points, where 40 x 39 / 2 items per point contend for the matrix entries;
dvp_convert_image equals the numpy reading of OpenCV's nearest-neighbour rule; the argument checks; two threads at once."""
import threading

import numpy as np
import pytest

import np_convert as N
from conftest import pkg

pytestmark = pytest.mark.gpu

SCORE_CASES = N.score_cases()


def capi():
    return pkg().get_capi()


def device_scores(m):
    return capi().view_scores(m["offsets"], m["ids"], m["centres"], m["point_ids"], m["xyz"])


@pytest.mark.parametrize("case", list(SCORE_CASES))
def test_view_scores_equal_the_serial_text(tmp_path, case):
    m = SCORE_CASES[case]
    rc, err, want = N.serial_scores(m, tmp_path)
    assert rc == 0, err
    got = device_scores(m)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (got, want)


def test_view_scores_under_contention(tmp_path):
    m = N.big_model()
    rc, err, want = N.serial_scores(m, tmp_path)
    assert rc == 0, err
    upper = want[np.triu_indices(40, 1)]
    assert want[0, 39] == 2001 and want[5, 39] == 2001 and (upper == 0).sum() >= 10 and (upper >= 2000).sum() >= 600      # (some close pairs are zeroed)
    for _ in range(2):      # integer sums: the same matrix whatever the order
        assert np.array_equal(device_scores(m), want)


@pytest.mark.parametrize("w,h,pad_w,pad_h,F", N.IMAGE_CASES)
def test_convert_image_equals_the_numpy_reading(w, h, pad_w, pad_h, F):
    out_w, out_h = N.out_size(pad_w, pad_h, F)
    src = N.picture(w, h)
    assert np.array_equal(capi().convert_image(src, pad_w, pad_h, out_w, out_h), N.convert_image(src, pad_w, pad_h, out_w, out_h))


def test_convert_image_honours_the_pitch():
    wide = N.picture(40, 9)
    src = wide[:, :17]
    assert src.strides[0] == 120
    assert np.array_equal(capi().convert_image(src, 17, 9, 11, 6), N.convert_image(np.ascontiguousarray(src), 17, 9, 11, 6))


def test_argument_checks():
    C = capi()
    m = SCORE_CASES["n3"]
    with pytest.raises(C.DvpError, match="dvp_view_scores: image \\d+, observation \\d+ names point \\d+, which is not among the points"):
        C.view_scores(m["offsets"], m["ids"], m["centres"], m["point_ids"][1:], m["xyz"][1:])
    twice = m["point_ids"].copy()
    twice[1] = twice[0]
    with pytest.raises(C.DvpError, match="dvp_view_scores: point id \\d+ occurs twice"):
        C.view_scores(m["offsets"], m["ids"], m["centres"], twice, m["xyz"])
    off = m["offsets"].copy()
    off[1], off[2] = off[2], off[1]
    with pytest.raises(C.DvpError, match="obs_offsets must not decrease"):
        C.view_scores(off, m["ids"], m["centres"], m["point_ids"], m["xyz"])
    L = C.lib()
    assert L.dvp_view_scores(0, 3, None, None, None, 0, None, None, None) != 0 and b"are required" in L.dvp_pairs_last_error()
    out = np.zeros(4, np.uint32)
    zero = np.zeros(20000, np.int64)
    assert L.dvp_view_scores(0, 16385, C._p(zero), None, C._p(np.zeros(3 * 16385)), 0, None, None, C._p(out)) != 0 and b"num_images must be 1 ... 16384" in L.dvp_pairs_last_error()
    # no observations and no points at all: zeros
    assert not C.view_scores(np.zeros(3, np.int64), np.zeros(0, np.int64), np.zeros((2, 3)), np.zeros(0, np.int64), np.zeros((0, 3))).any()
    src = N.picture(9, 5)
    for args, message in (((8, 7, 9, 5), "the padded size"), ((13, 4, 9, 5), "the padded size"), ((13, 7, 0, 5), "bad output size"), ((13, 7, 9, 70000), "bad output size")):
        with pytest.raises(C.DvpError, match="dvp_convert_image: .*" + message):
            C.convert_image(src, *args)
    assert L.dvp_convert_image(0, None, 9, 5, 27, 9, 5, 9, 5, C._p(out)) != 0 and b"are required" in L.dvp_pairs_last_error()
    assert L.dvp_convert_image(0, C._p(src), 9, 5, 26, 9, 5, 9, 5, C._p(np.zeros(135, np.uint8))) != 0 and b"pitch" in L.dvp_pairs_last_error()
    # an error leaves the next call alone
    assert np.array_equal(C.convert_image(src, 13, 7, 6, 3), N.convert_image(src, 13, 7, 6, 3))


def test_two_threads_convert_at_once(tmp_path):
    m, src = SCORE_CASES["track130"], N.picture(300, 5)
    _, _, want_scores = N.serial_scores(m, tmp_path)
    want_image = N.convert_image(src, 301, 6, 301, 6)
    bad = []

    def work(k):
        try:
            for _ in range(3):
                if not np.array_equal(device_scores(m), want_scores):
                    bad.append((k, "scores"))
                if not np.array_equal(capi().convert_image(src, 301, 6, 301, 6), want_image):
                    bad.append((k, "image"))
        except Exception as e:      # noqa: BLE001
            bad.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad
