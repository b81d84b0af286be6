"""The sweep passes' evaluation launches from per-view (pixel, view) lists (DVP_SWEEP_LIST, dvp_sweep_list.hpp) on the GPU:
dvp_run_patchmatch with the evaluations from lists and tile by tile (DVP_SWEEP_LIST=0) leaves the oracle's bits and the same number
of evaluations — every (pixel, view) lane computes what it computed, only the wave and the round it sits in differ.  The scene, the
state and the switches are test_gpu_sweep_dead_slots': 96 x 64 (second tile column 32 wide, last tile row 8 high), S = 9,
DVP_SWEEP_SPLIT=2 forces the passes on the small view."""
import numpy as np
import pytest

from conftest import pkg, synth, count_diff
from oracle import oracle as O
from test_sweep_dead_slots_host import scene, params
from test_gpu_sweep_dead_slots import OUT, S, MODE, oracle_pass

pytestmark = pytest.mark.gpu
_oracles = {}


def without_view_3(st, vw):
    st = dict(st, views=st["views"] & ~np.uint32(1 << 3))   # no pixel selects view 3: its lists are empty
    vw = vw.copy()
    vw[:, 5] = 0                                            # view 5 weighs 0 everywhere: its lists are empty too
    return st, vw


def pass_params(wpr, iterations=1):
    p = params(S, MODE, wpr)
    p["max_iterations"] = iterations   # 0: no strong / weak update rewrites the selections and weights before the sweep site
    return p


def start(cls_from_scene, p, change=None, **kw):
    sc, st, vw = scene(S)
    if change:
        st, vw = change(st, vw)
    e = cls_from_scene(sc, p, depths=sc["depth_gt"], **kw)
    e.upload_state(**st)
    e.set("view_weight", vw)
    return e


def oracle_of(wpr, sampler=0, change=None, iterations=1):
    if sampler == 0 and change is None and iterations == 1:
        return oracle_pass(wpr)
    key = (wpr, sampler, change, iterations)
    if key not in _oracles:
        o = start(O.from_scene, pass_params(wpr, iterations), change, sampler=sampler)
        o.run_patchmatch()
        _oracles[key] = {n: o.get(n).copy() for n in OUT}
    return _oracles[key]


NO_ROOM = "no room for the sweep passes' (pixel, view) lists"   # dvp_engine.hip: ensure_sweep_list_buffers' message on stderr


def gpu_pass(wpr, lists, monkeypatch, all_slots=False, band_gb=None, sampler=0, no_room=False, change=None, iterations=1):
    monkeypatch.setenv("DVP_SWEEP_LIST", "1" if lists else "0")
    monkeypatch.setenv("DVP_SWEEP_ALL_SLOTS", "1" if all_slots else "0")
    monkeypatch.setenv("DVP_SWEEP_SPLIT", "2")
    if band_gb is not None:
        monkeypatch.setenv("DVP_SWEEP_BAND_GB", band_gb)
    if no_room:
        monkeypatch.setenv("DVP_TEST_SWEEP_LIST_ALLOC_FAIL", "1")
    g = start(pkg("capi").from_scene, pass_params(wpr, iterations), change, sampler=sampler)   # (the DVP_* switches are read here)
    g.set_profiling(True)
    g.run_patchmatch()
    return {n: g.get(n).copy() for n in OUT}, g.timings()["ncc_evals"]["depth_to_weak"]


@pytest.mark.parametrize("all_slots", [False, True])
@pytest.mark.parametrize("wpr", [4, 29])   # 29: the whole line is the first stage, no second evaluation launch
def test_lists_and_tiles_leave_the_oracles_bits(wpr, all_slots, monkeypatch):
    want = oracle_of(wpr)
    lst, n_lst = gpu_pass(wpr, True, monkeypatch, all_slots)
    til, n_til = gpu_pass(wpr, False, monkeypatch, all_slots)
    for n in OUT:
        assert count_diff(lst[n], want[n]) == 0, n
        assert count_diff(til[n], want[n]) == 0, n
    assert n_lst == n_til and n_lst > 0
    w = want["weak_info"]
    assert (w == synth.STRONG).sum() > 0 and (w == synth.WEAK).sum() > 0


def test_the_exact_sampler(monkeypatch):
    want = oracle_of(4, sampler=1)
    lst, n_lst = gpu_pass(4, True, monkeypatch, sampler=1)
    til, n_til = gpu_pass(4, False, monkeypatch, sampler=1)
    for n in OUT:
        assert count_diff(lst[n], want[n]) == 0, n
    assert n_lst == n_til


def test_two_bands_of_rows(monkeypatch):
    """96 x 64, S = 9: 16.1 MB of cost records, 0.009 GB -> two bands (42 and 22 rows), each with lists of its own"""
    want = oracle_of(4)
    lst, n_lst = gpu_pass(4, True, monkeypatch, band_gb="0.009")
    til, n_til = gpu_pass(4, False, monkeypatch, band_gb="0.009")
    for n in OUT:
        assert count_diff(lst[n], want[n]) == 0, n
    assert n_lst == n_til


def test_lists_that_do_not_fit_fall_back_to_tiles(monkeypatch, capfd):
    """the hook refuses the lists' allocation group: the engine says so and evaluates tile by tile; without the hook it does not say
    so — the one sign, beside the time, of which evaluation kernels ran (bits and counts are equal by design)"""
    want = oracle_of(4)
    capfd.readouterr()
    got, n_got = gpu_pass(4, True, monkeypatch, no_room=True)
    assert NO_ROOM in capfd.readouterr().err
    monkeypatch.delenv("DVP_TEST_SWEEP_LIST_ALLOC_FAIL")
    lst, n_lst = gpu_pass(4, True, monkeypatch)
    assert NO_ROOM not in capfd.readouterr().err
    til, n_til = gpu_pass(4, False, monkeypatch)
    assert NO_ROOM not in capfd.readouterr().err   # (the switch is off: nothing was asked for)
    for n in OUT:
        assert count_diff(got[n], want[n]) == 0, n
        assert count_diff(got[n], til[n]) == 0, n
        assert count_diff(lst[n], til[n]) == 0, n
    assert n_got == n_til == n_lst


def test_views_with_empty_lists(monkeypatch, capfd):
    """Views 3 and 5 have no entry in either stage: dvp_scan3's total is 0, every workgroup of the two views leaves after the scalar
    load, dvp_sweep_list_fill writes nothing for them.  A pass with max_iterations = 0 hands the uploaded selections' view 3 and the
    uploaded weights to the sweep site as they are (an iteration's strong update rewrites both); the outputs say so."""
    want = oracle_of(4, change=without_view_3, iterations=0)
    assert ((want["selected_views"].reshape(-1) >> 3) & 1).sum() == 0
    assert (want["view_weight"].reshape(-1, 32)[:, 5] != 0).sum() == 0
    w = want["weak_info"]
    assert (w == synth.STRONG).sum() > 0 and (w == synth.WEAK).sum() > 0   # (both stages ran)
    capfd.readouterr()
    lst, n_lst = gpu_pass(4, True, monkeypatch, change=without_view_3, iterations=0)
    assert NO_ROOM not in capfd.readouterr().err
    til, n_til = gpu_pass(4, False, monkeypatch, change=without_view_3, iterations=0)
    for n in OUT:
        assert count_diff(lst[n], want[n]) == 0, n
        assert count_diff(til[n], want[n]) == 0, n
    assert n_lst == n_til and n_lst > 0
