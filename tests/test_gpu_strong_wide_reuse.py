"""The plane cache under the split strong update at 17 and 20 source views (DVP_STRONG_WIDE=1): dvp_strong_decide_wide reads the
vectors from the pixel's full-size record (cache on) or from the launch's half-size one (cache off) through the same place words.
dvp_run_patchmatch and the stage sequence give the same bits either way and equal the CPU oracle over three iterations of a
FIRST_INIT and a REFINE_ITER pass on one context (the helpers and the passes of tests/test_gpu_strong_reuse.py; one scene of odd
width)."""
import pytest

from conftest import count_diff, CHECKED
from test_gpu_strong_reuse import reference, _two_passes, _by_stages, _equal, _Snap, capi

pytestmark = pytest.mark.gpu

CASES = [(71, 50, 17), (96, 64, 20)]


def _forms_checked(run):
    def go(g):
        assert g.strong_update_form() == 32
        run(g)
        assert g.strong_update_form() == 32
    return go


def _both_modes(W, H, S, run, monkeypatch, whole_candidates, what):
    monkeypatch.setenv("DVP_STRONG_WIDE", "1")
    ref = reference(W, H, S)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DVP_STRONG_REUSE", mode)
        res[mode] = _two_passes(ref, S, _forms_checked(run))
    for k, out in ((0, ref["out1"]), (1, ref["out2"])):
        for n in CHECKED:
            nd = count_diff(res["1"][k][n], res["0"][k][n])
            assert nd == 0, "pass %d: %s differs in %d entries between DVP_STRONG_REUSE=0 and the default" % (k + 1, n, nd)
        _equal(out, _Snap(res["1"][k]), "pass %d %s against the oracle" % (k + 1, what), W, whole_candidates=whole_candidates)


@pytest.mark.parametrize("W,H,S", CASES)
def test_wide_run_patchmatch_same_bits_with_and_without_the_cache(W, H, S, monkeypatch):
    _both_modes(W, H, S, lambda g: g.run_patchmatch(), monkeypatch, False, "run_patchmatch")


@pytest.mark.parametrize("W,H,S", CASES)
def test_wide_run_stage_same_bits_with_and_without_the_cache(W, H, S, monkeypatch):
    _both_modes(W, H, S, _by_stages, monkeypatch, True, "by stages")
