"""The sweep site without the two end slots no decision reads (dvp_forms.hpp: sweep_slot_read), on the GPU: dvp_run_patchmatch with
the site as view-compacted passes and as the fused kernel leaves the oracle's bits and those of DVP_SWEEP_ALL_SLOTS=1 (all 61 slots,
as before; at weak_peak_radius 29 the whole line is the first stage and the end slots stay, so the switch changes nothing there).  The scene and the state are test_sweep_dead_slots_host's: a wide baseline and depth range, so that both end slots are
inside the depth range and the switch changes what is evaluated."""
import pytest

from conftest import pkg, synth, count_diff
from oracle import oracle as O
from test_sweep_dead_slots_host import scene, params, engine, run_site

pytestmark = pytest.mark.gpu
S, MODE = 9, "refine_geom"
OUT = ("planes", "weak_info", "radius", "costs", "selected_views", "view_weight")
_oracles = {}


def gpu_engine(p):
    sc, st, vw = scene(S)
    g = pkg("capi").from_scene(sc, p, depths=sc["depth_gt"])   # (the DVP_* switches are read here)
    g.upload_state(**st)
    g.set("view_weight", vw)
    return g


def oracle_pass(wpr):
    if wpr not in _oracles:
        o = engine(O.Oracle, S, params(S, MODE, wpr))
        o.run_patchmatch()
        _oracles[wpr] = {n: o.get(n).copy() for n in OUT}
    return _oracles[wpr]


def gpu_pass(wpr, form, all_slots, monkeypatch, band_gb=None):
    monkeypatch.setenv("DVP_SWEEP_ALL_SLOTS", "1" if all_slots else "0")
    monkeypatch.setenv("DVP_SWEEP_SPLIT", "2" if form == "passes" else "0")
    if band_gb is not None:
        monkeypatch.setenv("DVP_SWEEP_BAND_GB", band_gb)
    g = gpu_engine(params(S, MODE, wpr))
    g.run_patchmatch()
    return {n: g.get(n).copy() for n in OUT}


@pytest.mark.parametrize("form", ["passes", "fused"])
@pytest.mark.parametrize("wpr", [4, 29])
def test_a_pass_leaves_the_oracles_bits(wpr, form, monkeypatch):
    want = oracle_pass(wpr)
    skip = gpu_pass(wpr, form, False, monkeypatch)
    full = gpu_pass(wpr, form, True, monkeypatch)
    for n in OUT:
        assert count_diff(skip[n], want[n]) == 0, n
        assert count_diff(skip[n], full[n]) == 0, n
    w = want["weak_info"]
    assert (w == synth.STRONG).sum() > 0 and (w == synth.WEAK).sum() > 0


def test_two_bands_of_rows(monkeypatch):
    """96 x 64, S = 9: 16.1 MB of cost records, 0.009 GB -> two bands (42 and 22 rows)"""
    want = oracle_pass(4)
    skip = gpu_pass(4, "passes", False, monkeypatch, band_gb="0.009")
    for n in OUT:
        assert count_diff(skip[n], want[n]) == 0, n


@pytest.mark.parametrize("all_slots", [False, True])
def test_the_separate_kernels_and_their_evaluation_counts(all_slots, monkeypatch):
    """dvp_run_stage's DepthToWeak and LocalRefine on the built state: the bits and the number of evaluations of the host emulation of
    the same source, with and without the end slots (the host test derives the difference of the two counts from the state)"""
    host = run_site(S, MODE, 4, "separate", all_slots, monkeypatch)
    g = gpu_engine(params(S, MODE, 4))
    g.set_profiling(True)
    g.run_stage("depth_to_weak")
    g.run_stage("local_refine")
    for n in ("planes", "weak_info", "radius", "selected_views"):
        assert count_diff(g.get(n), host.get(n)) == 0, n
    ev = g.timings()["ncc_evals"]
    assert ev["depth_to_weak"] + ev["local_refine"] == host.evals()
