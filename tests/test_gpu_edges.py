"""The edge prior on the device (csrc/dvp_edges.hip) through the C ABI: dvp_canny_edge_map and dvp_edge_hysteresis on the cases
of test_edges_host.py, a 260 k-pixel chain, the context path (dvp_edge_map_begin / _finish from the resident image 0, ties in
the grey conversion included) and one full-size image.  References: the host mirror's EdgeSegment (`test_host --edges`), the
numpy Canny, scipy's connected components — exact, every pixel."""
import numpy as np
import pytest

import np_edges as E
from conftest import pkg, synth, make_params

pytestmark = pytest.mark.gpu


def capi():
    return pkg().get_capi()


@pytest.mark.parametrize("name", sorted(E.images()))
def test_whole_map_equals_host_mirror_and_numpy(name):
    want = E.expected_edges(name)
    got = capi().canny_edge_map(E.images()[name])
    assert np.array_equal(got, want), (name, int((got != want).sum()), int((want > 0).sum()))


def test_pitch_is_honoured():
    wide = np.zeros((65, 80), np.uint8)
    wide[:, :63] = E.images()["size_63x65"]
    assert np.array_equal(capi().canny_edge_map(wide[:, :63]), E.expected_edges("size_63x65"))


@pytest.mark.parametrize("W,H", [(2, 9), (9, 2)])
def test_small_sizes_are_an_error(W, H):
    with pytest.raises(capi().DvpError, match="at least 3"):
        capi().canny_edge_map(np.zeros((H, W), np.uint8))


@pytest.mark.parametrize("name", sorted(E.maps()))
def test_hysteresis_equals_connected_components(name):
    want = E.expected_hysteresis(name)
    got = capi().edge_hysteresis(E.maps()[name])
    assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_hysteresis_long_chain():
    """one chain of about 260 k pixels whose only strong pixel sits at one end: every launch of the stage runs once"""
    m = E.serpentine(1023, 515)
    assert (m != 1).sum() > 260000
    got = capi().edge_hysteresis(m)
    assert np.array_equal(got > 0, m != 1)
    assert not capi().edge_hysteresis(E.serpentine(1023, 515, strong=False)).any()


W, H = 127, 93


def _scene():
    sc = synth.make_scene(W, H, 1)
    big = E.smooth_noisy(np.random.RandomState(5), 2 * W, 2 * H).astype(np.float32)
    img = (big[0::2, 0::2] + big[0::2, 1::2] + big[1::2, 0::2] + big[1::2, 1::2]) * np.float32(0.25)   # exact: multiples of 0.25
    frac = img - np.floor(img)
    assert (frac == 0.5).sum() > 50 and (frac == 0.25).sum() > 50 and (frac == 0.75).sum() > 50
    ties = np.floor(img[frac == 0.5]).astype(int)
    assert (ties % 2 == 0).any() and (ties % 2 == 1).any()
    images = [img] + [np.asarray(a, np.float32) for a in sc["images"][1:]]
    return sc, images, np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _context(sc, images):
    c = capi().from_scene(sc, make_params(2))
    c.set_images(images)
    return c


def test_context_edge_map():
    sc, images, u8 = _scene()
    want = E.host_tool_edges(u8)
    assert 0.01 < (want > 0).mean() < 0.5
    c = _context(sc, images)
    c.edge_map_begin(True)
    assert np.array_equal(c.edge_map_finish(), want)
    assert np.array_equal(c.get("edge").reshape(H, W), want)
    c.run_stage("gen_edge_inform")
    c.synchronize()
    o = _context(sc, images)
    o.upload_state(edge=want)
    o.run_stage("gen_edge_inform")
    o.synchronize()
    a, b = c.get("edge_neigh"), o.get("edge_neigh")
    assert (b >= 0).any() and np.array_equal(a, b)
    # install = 0: the map is computed and fetched, the context's edge buffer keeps what it held
    mine = (np.random.RandomState(2).uniform(size=(H, W)) < 0.1).astype(np.uint8) * 255
    o.upload_state(edge=mine)
    o.edge_map_begin(False)
    assert np.array_equal(o.edge_map_finish(), want)
    assert np.array_equal(o.get("edge").reshape(H, W), mine)
    # two maps begun, then fetched: oldest first
    o.set_images([images[1], images[0]])
    o.edge_map_begin(False)
    o.set_images(images)
    o.edge_map_begin(False)
    first, second = o.edge_map_finish(), o.edge_map_finish()
    assert np.array_equal(first, E.host_tool_edges(np.clip(np.rint(images[1]), 0, 255).astype(np.uint8))) and np.array_equal(second, want)
    with pytest.raises(capi().DvpError, match="no edge map was begun"):
        o.edge_map_finish()
    c.close()
    o.close()


def test_context_edge_map_reserved_ahead():
    sc, images, u8 = _scene()
    c = _context(sc, images)
    c.reserve(0, 8)
    c.edge_map_begin(True)
    assert np.array_equal(c.edge_map_finish(), E.host_tool_edges(u8))
    c.close()


def test_begin_before_any_image_is_an_error():
    c = capi().Context(W, H, 2)
    with pytest.raises(capi().DvpError, match="no images"):
        c.edge_map_begin(True)
    c.close()


def test_full_size_image_equals_host_mirror():
    """6208 x 4128: a smooth random field plus steps and noise.  The numpy model is left out at this size for time; the host
    tool is the function the driver calls."""
    FW, FH = 6208, 4128
    rs = np.random.RandomState(9)
    coarse = rs.uniform(40, 200, (FH // 64 + 2, FW // 64 + 2)).astype(np.float32)
    ys, xs = (np.arange(FH, dtype=np.float32) / 64)[:, None], (np.arange(FW, dtype=np.float32) / 64)[None, :]
    y0, x0 = ys.astype(np.int32), xs.astype(np.int32)
    fy, fx = ys - y0, xs - x0
    f = (coarse[y0, x0] * (1 - fy) * (1 - fx) + coarse[y0, x0 + 1] * (1 - fy) * fx + coarse[y0 + 1, x0] * fy * (1 - fx) + coarse[y0 + 1, x0 + 1] * fy * fx)
    f += np.float32(40) * (((np.arange(FW)[None, :] // 300) + (np.arange(FH)[:, None] // 220)) % 2).astype(np.float32)   # steps
    f += rs.randint(-25, 26, (FH, FW)).astype(np.float32)
    u8 = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    want = E.host_tool_edges(u8)
    assert 0.005 < (want > 0).mean() < 0.5
    got = capi().canny_edge_map(u8)
    assert np.array_equal(got, want), int((got != want).sum())
