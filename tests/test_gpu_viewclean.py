"""The visibility-mask clean-up on the device (csrc/dvp_viewclean.hip) through the C ABI: dvp_clean_selected_views on the cases
of test_viewclean_host.py, one 260 k-pixel component, a 1552 x 1032 map of nine planes, and the context path
(dvp_set_view_cleanup + dvp_download_maps / _begin / _finish after a run).  References: the host mirror's clean-up and scipy's
4-connected components — exact, every word."""
import threading

import numpy as np
import pytest

import np_viewclean as V
from conftest import pkg, synth, make_params, first_pass_state

pytestmark = pytest.mark.gpu


def capi():
    return pkg().get_capi()


@pytest.mark.parametrize("name", sorted(V.cases()))
def test_words_equal_host_mirror_and_scipy(name):
    views, num_src, min_region = V.cases()[name]
    want = V.expected(name)
    got = capi().clean_selected_views(views, num_src, min_region)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_one_long_component():
    """a serpentine of about 260 k pixels through every tile of a 1023 x 515 map: filled or kept as a whole"""
    clear = V.serpentine(1023, 515)
    n = int(clear.sum())
    assert n > 260000
    views = V.words_of([clear])
    assert np.array_equal(capi().clean_selected_views(views, 1, n), views)            # size == min_region: stays clear
    assert (capi().clean_selected_views(views, 1, n + 1) == 1).all()
    assert np.array_equal(capi().clean_selected_views(views, 1, n - 1), views)


def test_level_sized_map_of_nine_planes():
    W, H, S = 1552, 1032, 9
    views = V.smooth_words(W, H, S)
    want = V.np_clean(views, S, 1280)
    changed = want != views
    assert 0.01 < changed.mean() < 0.5 and (want != V.low_mask(S)).any()
    got = capi().clean_selected_views(views, S, 1280)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("num_src", [33, -1])
def test_bad_source_count_is_an_error(num_src):
    with pytest.raises(capi().DvpError, match="num_src"):
        capi().clean_selected_views(np.zeros((5, 7), np.uint32), num_src, 20)


W, H, S = 127, 93, 3
MIN_REGION = 20


@pytest.fixture(scope="module")
def ran():
    """a context after one run, its raw selected-view words and the reference applied to them"""
    sc = synth.make_scene(W, H, S)
    c = capi().from_scene(sc, make_params(S + 1, max_iterations=2))
    c.upload_state(**first_pass_state(sc))
    c.run_patchmatch()
    raw = c.get("selected_views").copy()
    want = V.mirror_clean(raw.reshape(H, W), S, MIN_REGION).ravel()
    assert np.array_equal(want, V.np_clean(raw.reshape(H, W), S, MIN_REGION).ravel())
    assert (want != raw).any()                       # the clean-up has something to do on this scene
    yield c, raw, want
    c.close()


def test_context_download_maps_cleans_the_staged_words_only(ran):
    c, raw, want = ran
    plain = c.download_maps()
    assert np.array_equal(plain[2], raw)                                  # off by default: the raw words
    c.set_view_cleanup(True, S, MIN_REGION)
    cleaned = c.download_maps()
    assert np.array_equal(cleaned[2], want)
    assert np.array_equal(c.get("selected_views"), raw)                   # the device state keeps the raw words
    for k in (0, 1, 3, 4):                                                # depth, normal, states, radius: as without
        assert np.array_equal(cleaned[k].view(np.uint8), plain[k].view(np.uint8)), k
    c.set_view_cleanup(False)
    assert np.array_equal(c.download_maps()[2], raw)
    c.set_view_cleanup(True, S, MIN_REGION)
    assert np.array_equal(c.download_maps()[2], want)
    c.set_view_cleanup(True, 2, 5)                                        # other arguments: fewer planes, the third bit dropped
    assert np.array_equal(c.download_maps()[2], V.mirror_clean(raw.reshape(H, W), 2, 5).ravel())
    c.set_view_cleanup(False)
    with pytest.raises(capi().DvpError, match="num_src"):
        c.set_view_cleanup(True, 33, MIN_REGION)
    assert np.array_equal(c.download_maps()[2], raw)


def test_context_begin_and_finish_from_two_threads(ran):
    c, raw, want = ran
    c.set_view_cleanup(True, S, MIN_REGION)
    got = []
    for _ in range(2):
        c.download_maps_begin()
        t = threading.Thread(target=lambda: got.append(c.download_maps_finish()))
        t.start()
        t.join()
    c.set_view_cleanup(False)
    assert len(got) == 2 and all(np.array_equal(g[2], want) for g in got)
    assert np.array_equal(c.get("selected_views"), raw)


def test_context_scratch_reserved_ahead(ran):
    _, raw, want = ran
    sc = synth.make_scene(W, H, S)
    c = capi().from_scene(sc, make_params(S + 1, max_iterations=2))
    c.reserve(0, 16)
    c.upload_state(**first_pass_state(sc))
    c.run_patchmatch()
    assert np.array_equal(c.get("selected_views"), raw)                   # the same run ...
    c.set_view_cleanup(True, S, MIN_REGION)
    assert np.array_equal(c.download_maps()[2], want)                     # ... the same words
    c.close()
