"""The sweep passes' evaluation launches from per-view (pixel, view) lists (DVP_SWEEP_LIST, dvp_sweep_list.hpp) on the host
emulation (tests/sweep_list_host/sweep_list_emul.cpp: tests/emul's emulation plus the engine's sequence of the passes with the
evaluation launches in the form dvp_forms.hpp chooses): a whole sweep site with the lists — built by the functions the kernels share
with the host, consumed workgroup by workgroup in list order — and without them (DVP_SWEEP_LIST=0) leaves the oracle's bits and the
same number of evaluations, at weak_peak_radius 4 and 29 (the whole line in the first stage: no second evaluation launch), with and
without the end slots (DVP_SWEEP_ALL_SLOTS).  Then the switch and the decision on their own (sweep_eval_form), through a test hook
that leaves the lists tests/test_forms.py pins as they are.  The scene and the state are test_sweep_dead_slots_host's."""
import numpy as np
import pytest

from conftest import synth, count_diff
from tests.sweep_list_host import sweep_list_emul as E
from test_sweep_dead_slots_host import OUT, W, H, params, engine, oracle_result, run_site
from test_sweep_list_host import VALID, PEAK, go, expected

S, MODE = 9, "refine_geom"
TILES, LISTS = 0, 1       # dvp_forms.hpp: SweepEval


def site(wpr, lists, all_slots, monkeypatch, no_room=False):
    monkeypatch.setenv("DVP_SWEEP_LIST", "1" if lists else "0")
    monkeypatch.setenv("DVP_SWEEP_ALL_SLOTS", "1" if all_slots else "0")
    monkeypatch.setenv("DVP_SWEEP_SPLIT", "2")   # the passes also on this small view
    if no_room:
        monkeypatch.setenv("DVP_TEST_SWEEP_LIST_ALLOC_FAIL", "1")
    e = engine(E.SweepListEmul, S, params(S, MODE, wpr))
    e.read_switches()
    e.count_evals(True)
    assert e.run_passes() == (LISTS if lists and not no_room else TILES)
    return e


@pytest.mark.parametrize("all_slots", [False, True])
@pytest.mark.parametrize("wpr", [4, 29])
def test_lists_and_tiles_leave_the_oracles_bits(wpr, all_slots, monkeypatch):
    want = oracle_result(S, MODE, wpr)
    lst = site(wpr, True, all_slots, monkeypatch)
    til = site(wpr, False, all_slots, monkeypatch)
    ref = run_site(S, MODE, wpr, "passes", all_slots, monkeypatch)   # tests/sweep_host's own sequence of the passes, pixel by pixel
    for n in OUT:
        assert count_diff(lst.get(n), want[n]) == 0, n
        assert count_diff(til.get(n), want[n]) == 0, n
    assert lst.evals() == til.evals() == ref.evals() > 0
    w = want["weak_info"]
    assert (w == synth.STRONG).sum() > 0 and (w == synth.WEAK).sum() > 0


def test_the_cost_records_are_the_same(monkeypatch):
    """field by field: the lists change which wave evaluates a (pixel, view), not what it writes"""
    lst = site(4, True, False, monkeypatch)
    til = site(4, False, False, monkeypatch)
    for v in range(S):
        for f in (0, 1, 24, 25, 30, 35, 36, 59, 60, 61, 71, 72):
            assert count_diff(lst.sweep_field(v, f), til.sweep_field(v, f)) == 0, (v, f)


def test_stage_1_lists_after_a_real_decide1(monkeypatch):
    """the lists of the second stage as the pass built them, from the flags its own dvp_sweep_decide1 left — some valid pixels
    without a central peak — against the numpy enumeration of sweep_go in the order rule (test_sweep_list_host)"""
    e = site(4, True, False, monkeypatch)
    flags, lists = E.stage1_lists(S, W * H)
    valid, peak = (flags & VALID) != 0, (flags & PEAK) != 0
    assert (peak <= valid).all() and 0 < peak.sum() < valid.sum()
    sel = e.get("selected_views").reshape(-1)[:W * H]      # (the site leaves selections and weights as they are)
    vw = e.get("view_weight").reshape(W * H, 32)
    want = expected(W, H, S, go(W, H, S, 1, flags, sel, vw))
    for v in range(S):
        assert lists[v].size == want[v].size > 0, v
        assert (lists[v] == want[v]).all(), v
    # ... and the pixels with a central peak are the ones the second decision pass classified: all the others are WEAK or UNKNOWN
    assert (e.get("weak_info").reshape(-1)[~peak] != synth.STRONG).all()


def test_lists_that_do_not_fit(monkeypatch):
    want = oracle_result(S, MODE, 4)
    e = site(4, True, False, monkeypatch, no_room=True)
    for n in OUT:
        assert count_diff(e.get(n), want[n]) == 0, n


# ---- the switch and the decision ----
def decide(fused=1, geom=1, wpr=4, sweep_fits=1, W=96, H=64, list_fits=1):
    return E.sweep_eval_form(fused, geom, wpr, sweep_fits, W, H, list_fits)


@pytest.fixture
def env(monkeypatch):
    for v in ("DVP_SWEEP_LIST", "DVP_SWEEP_SPLIT", "DVP_SWEEP_ALL_SLOTS", "DVP_SWEEP_BAND_GB"):
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


def test_the_lists_are_the_default_of_the_passes(env):
    assert decide() == (1, LISTS)
    assert decide(wpr=29) == (1, LISTS)
    for v, on in (("1", 1), ("0", 0), ("2", 1), ("", 0), ("x", 0)):   # atoi(e) != 0, as every =0 / =1 switch
        env.setenv("DVP_SWEEP_LIST", v)
        assert decide() == (on, LISTS if on else TILES), v


def test_no_lists_without_the_passes_or_without_room(env):
    assert decide(list_fits=0) == (1, TILES)
    assert decide(sweep_fits=0) == (1, TILES)      # the fused kernel
    assert decide(fused=0) == (1, TILES)           # the separate kernels of dvp_run_stage
    assert decide(geom=0) == (1, TILES)            # without the geometric term the fused kernel is the default ...
    env.setenv("DVP_SWEEP_SPLIT", "2")
    assert decide(geom=0) == (1, LISTS)            # ... unless the passes are forced
    env.setenv("DVP_SWEEP_SPLIT", "0")
    assert decide() == (1, TILES)
