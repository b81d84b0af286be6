"""The device edge prior's arithmetic without a GPU: csrc/dvp_edges.hpp, built for the host in tests/edges_host and run one
pixel after the other, against the host mirror's EdgeSegment (`test_host --edges`), the independent numpy / scipy Canny of
test_host_oracles.py with the sequential frame fix-ups, and scipy's connected components for the hysteresis alone.  Every
comparison is exact: the arithmetic is integer, and the two sector tests (fixed-point TG22, float tan) agree for every Sobel
gradient an 8-bit image can give."""
import ctypes

import numpy as np
import pytest

import np_edges as E

pytestmark = pytest.mark.hostbox


def test_thresholds_for_every_median():
    L = E.host_lib()
    for med in range(-1, 255):
        lo, hi = ctypes.c_int(0), ctypes.c_int(0)
        L.dvp_edge_thresholds_host(med, ctypes.byref(lo), ctypes.byref(hi))
        assert (lo.value, hi.value) == E.np_thresholds(med), med
    assert E.np_thresholds(-1) == (0, -1) and E.np_thresholds(0) == (0, 0) and E.np_thresholds(100) == (33 * 33, 100 * 100)


@pytest.mark.parametrize("name", sorted(E.images()))
def test_median_matches_numpy(name):
    u8 = E.images()[name]
    assert E.host_lib().dvp_edge_median_host(u8.ctypes.data, u8.shape[1], u8.shape[0], u8.strides[0]) == E.np_median(u8)


def test_median_minus_one_case_is_one():
    assert E.np_median(E.images()["median_minus_one"]) == -1
    assert E.expected_edges("median_minus_one").any()


@pytest.mark.parametrize("name", sorted(E.images()))
def test_whole_map_equals_host_mirror_and_numpy(name):
    u8 = E.images()[name]
    want = E.expected_edges(name)               # test_host --edges, asserted equal to _np_canny + sequential fix-ups
    rc, got = E.serial_canny(u8)
    assert rc == 0
    assert set(np.unique(got)) <= {0, 255}
    assert np.array_equal(got, want), (name, int((got != want).sum()), int((want > 0).sum()))


def test_cases_reach_the_fix_ups():
    """the step images do put edges on the frame and take some of them away again"""
    hit = 0
    for name, u8 in E.images().items():
        if not name.startswith("step_"):
            continue
        e = E.expected_edges(name)
        frame = np.ones(e.shape, bool)
        frame[1:-1, 1:-1] = False
        hit += int((e[frame] > 0).sum())
    assert hit > 0


def test_pitch_is_honoured():
    u8 = E.images()["size_63x65"]
    wide = np.zeros((65, 80), np.uint8)
    wide[:, :63] = u8
    out = np.zeros((65, 63), np.uint8)
    assert E.host_lib().dvp_canny_edge_map_host(wide.ctypes.data, 63, 65, 80, out.ctypes.data) == 0
    assert np.array_equal(out, E.expected_edges("size_63x65"))


@pytest.mark.parametrize("W,H", [(2, 9), (9, 2), (1, 1), (2, 2)])
def test_small_sizes_are_an_error(W, H):
    rc, _ = E.serial_canny(np.zeros((H, W), np.uint8))
    assert rc != 0


def test_grey_conversion_rounds_half_to_even_and_saturates():
    k = np.arange(0, 256, dtype=np.float32)
    t = np.concatenate([k + np.float32(0.5), k + np.float32(0.25), k + np.float32(0.75), k, np.array([-3.0, 300.0, -0.5, -0.25, 254.5, 255.5, 255.25], np.float32)])
    out = np.zeros(len(t), np.uint8)
    E.host_lib().dvp_grey_bytes_host(t.ctypes.data, len(t), out.ctypes.data)
    want = np.clip(np.rint(t), 0, 255).astype(np.uint8)
    assert np.array_equal(out, want), np.nonzero(out != want)[0][:5]
    assert out[0] == 0 and out[1] == 2 and out[2] == 2 and out[3] == 4          # 0.5, 1.5, 2.5, 3.5: ties go to the even byte


@pytest.mark.parametrize("name", sorted(E.maps()))
def test_hysteresis_equals_connected_components(name):
    m = E.maps()[name]
    want = E.expected_hysteresis(name)
    got = E.serial_hysteresis(m)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_hysteresis_cases_say_what_they_claim():
    assert (E.expected_hysteresis("serpentine_129x67") > 0).sum() == (E.maps()["serpentine_129x67"] != 1).sum() > 129 * 33
    assert not E.expected_hysteresis("serpentine_no_strong").any()
    assert (E.expected_hysteresis("spiral_61") > 0).sum() == (E.maps()["spiral_61"] != 1).sum() > 61 * 20
    st = E.expected_hysteresis("staircase")
    assert (st > 0).sum() == 120                        # both staircases, corner contacts only
    from scipy import ndimage
    lab4, n4 = ndimage.label(E.maps()["staircase"] != 1)
    assert n4 == 120                                    # 4-connectivity would leave every pixel alone
    tb = E.expected_hysteresis("tile_boundaries")
    assert tb[5, 99] and tb[8, 30] and tb[23, 129] and not tb[30].any()
    assert E.expected_hysteresis("all_candidate").all() and E.expected_hysteresis("all_strong").all() and not E.expected_hysteresis("empty").any()
