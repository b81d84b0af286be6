"""The device view clean-up's arithmetic without a GPU: csrc/dvp_viewclean.hpp, built for the host in tests/viewclean_host and
run tile by tile, one lane after the other, against the host mirror's clean-up (host/cc.cpp's Connect + the driver's fill rule)
and scipy's 4-connected components + numpy.bincount.  The two references are asserted equal on every case first
(np_viewclean.expected); every comparison is exact on every word."""
import numpy as np
import pytest

import np_viewclean as V

pytestmark = pytest.mark.hostbox


@pytest.mark.parametrize("name", sorted(V.cases()))
def test_serial_device_text_equals_host_mirror_and_scipy(name):
    views, num_src, min_region = V.cases()[name]
    want = V.expected(name)                      # host mirror, asserted equal to scipy's
    rc, got = V.serial_clean(views, num_src, min_region)
    assert rc == 0
    assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_tile_is_the_wave_wide():
    TW, R = V.tile()
    assert TW == 64 and R >= 2 and (R & (R - 1)) == 0


def _components(plane):
    from scipy import ndimage
    return ndimage.label(plane, structure=np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]))[1]


def test_cases_say_what_they_claim():
    TW, R = V.tile()
    c, e = V.cases(), V.expected
    low = lambda name: c[name][0] & np.uint32(1)
    for tag, (W, H) in (("129x%d" % (2 * R + 1), (129, 2 * R + 1)), ("257x131", (257, 131))):
        for name in ("serpentine", "spiral", "stair_edges", "weave_v", "weave_h"):
            clear = low("%s_eq_%s" % (name, tag)) == 0
            assert _components(clear) == 1 and clear.sum() == c["%s_eq_%s" % (name, tag)][2], name
            assert np.array_equal(e("%s_eq_%s" % (name, tag)), low("%s_eq_%s" % (name, tag)))      # a size equal to min_region stays clear
            assert (e("%s_gt_%s" % (name, tag)) == 1).all()                                          # one pixel short: filled
            # the path is in every tile column and tile row it can reach
            cols, rows = np.nonzero(clear.any(axis=0))[0] // TW, np.nonzero(clear.any(axis=1))[0] // R
            if name in ("serpentine", "spiral"):
                assert set(cols) == set(range((W + TW - 1) // TW)) and set(rows) == set(range((H + R - 1) // R))
        clear = low("weave_v_eq_" + tag) == 0
        assert (clear[:, 63] & clear[:, 64]).sum() >= H // 2            # crosses the seam on every other row
        clear = low("weave_h_eq_" + tag) == 0
        assert (clear[R - 1, :] & clear[R, :]).sum() >= W // 2
        clear = low("stair_corners_" + tag) == 0
        assert _components(clear) == clear.sum() > 20 and (e("stair_corners_" + tag) == 1).all()
        clear = low("diagonal_" + tag) == 0
        assert clear.sum() == 6 and _components(clear) == 6 and clear[R - 1, 63] and clear[R, 64] and (e("diagonal_" + tag) == 1).all()
        clear = low("bars_" + tag) == 0
        left = e("bars_" + tag) == 0
        assert _components(clear) == 9 and _components(left) == 6 and left.sum() == 3 * (20 + 21) and clear.sum() == 3 * (19 + 20 + 21)
        assert left[3, 63] and left[3, 64] and left[R - 1, 32] and left[R, 32] and not left[1, 63] and not left[R, 30]
    for (W, H) in V.sizes():
        tag = "%dx%d" % (W, H)
        assert (e("all_clear_eq_" + tag) == 0).all() and (e("all_clear_gt_" + tag) == 1).all() and (e("all_set_" + tag) == 1).all()
        assert np.array_equal(e("checker_m1_" + tag), low("checker_m1_" + tag)) and (e("checker_m2_" + tag) == 1).all()
    for num_src in (0, 1, 9, 31, 32):
        raw = c["words_s%d_m0" % num_src][0]
        mask = V.low_mask(num_src)
        if num_src < 32:
            assert (raw & ~mask).any()                                   # garbage above num_src ...
        for m in (-5, 0):
            assert np.array_equal(e("words_s%d_m%d" % (num_src, m)), raw & mask)   # ... is all that min_region <= 0 takes away
        if num_src:
            a, b = e("words_s%d_m20" % num_src), e("words_s%d_m1280" % num_src)
            assert (a != (raw & mask)).any() and (b != a).any() and (b != mask).any()
    assert not e("words_s0_m1280").any()


def test_bad_source_count_fails():
    views, num_src, min_region = V.cases()["words_s9_m20"]
    assert V.serial_clean(views, 33, 20)[0] != 0 and V.serial_clean(views, -1, 20)[0] != 0
