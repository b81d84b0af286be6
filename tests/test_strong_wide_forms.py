"""DVP_STRONG_WIDE (dvp-mvs_amd/csrc/dvp_forms.hpp): the switch that lets views with 17 ... 31 sources take the split strong
update, with the streaming decision kernel (decide = 32).  Unset or 0: every decision is what it was — S = 17 is monolithic, as
tests/test_forms.py pins it; 1: split for 17 <= S <= 31; 2: as 1, and the streaming kernel at every S <= 16 too (A/B).  Through
the same two exports of the host-emulation library as tests/test_forms.py, whose output layout does not grow."""
import itertools

import pytest

from test_forms import ALL_VARS, TRI, UNSET, SPLIT, MONO_V8, MONO_V16, MONO, decide, switches, on

WIDE = "DVP_STRONG_WIDE"


@pytest.fixture
def env(monkeypatch):
    for v in ALL_VARS + [WIDE]:
        monkeypatch.delenv(v, raising=False)

    def set_(**kw):
        for k, v in kw.items():
            if v is UNSET:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
    return set_


def got(**kw):
    return tuple(decide(**kw)[k] for k in ("strong", "eval_items", "decide", "refine_lanes", "plan"))


def mono(S):
    return (MONO_V8 if S <= 8 else (MONO_V16 if S <= 16 else MONO), 0, 0, 0, 0)


def bracket(S):
    return next(m for m in (4, 6, 8, 10, 12, 16) if S <= m)


def test_off_is_todays_rule(env):
    for v in (UNSET, "0", "", "x"):
        env(**{WIDE: v})
        assert got(S=17) == (MONO, 0, 0, 0, 0), v
        assert [got(S=S)[2] for S in range(1, 18)] == [4, 4, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 16, 16, 16, 16, 0], v
        assert [got(S=S) for S in (20, 31)] == [mono(20), mono(31)], v


def test_on_splits_17_to_31(env):
    for wide in ("1", "3", "-1", "7"):   # any value that is neither 0 nor 2
        env(**{WIDE: wide})
        for items, lanes in itertools.product(TRI, repeat=2):
            env(DVP_EVAL_ITEMS=items, DVP_REFINE_LANES=lanes)
            for S, hdr, big in itertools.product((17, 20, 31), (0, 1), (0, 1)):
                want = (SPLIT, int(on(items, True)), 32, int(on(lanes, True) and not big), hdr)
                assert got(S=S, reuse_hdr=hdr, big_images=big) == want, (wide, items, lanes, S, hdr, big)
        env(DVP_EVAL_ITEMS=UNSET, DVP_REFINE_LANES=UNSET)
        # S <= 16 is untouched
        assert got(S=16) == (SPLIT, 1, 16, 1, 1), wide
        assert [got(S=S)[2] for S in range(1, 17)] == [bracket(S) for S in range(1, 17)], wide
        # still monolithic: the cost buffer did not fit, or the split form is off
        assert [got(S=S, split_fits=0) for S in (9, 17, 20, 31)] == [mono(S) for S in (9, 17, 20, 31)], wide
        env(DVP_STRONG_SPLIT="0")
        assert [got(S=S) for S in (8, 16, 17, 20, 31)] == [mono(S) for S in (8, 16, 17, 20, 31)], wide
        env(DVP_STRONG_SPLIT=UNSET)


def test_two_streams_at_every_count(env):
    env(**{WIDE: "2"})
    for S in (1, 9, 16):
        assert got(S=S) == (SPLIT, 1, 32, 1, 1), S
    for S in (17, 20, 31):
        assert got(S=S) == (SPLIT, 1, 32, 1, 1), S
    assert got(S=9, reuse_hdr=0, big_images=1) == (SPLIT, 1, 32, 0, 0)
    assert [got(S=S, split_fits=0) for S in (1, 9, 16, 17)] == [mono(S) for S in (1, 9, 16, 17)]
    env(DVP_STRONG_SPLIT="0")
    assert [got(S=S) for S in (1, 9, 16, 17)] == [mono(S) for S in (1, 9, 16, 17)]


def test_the_switch_dictionary_is_unchanged(env):
    want = dict(no_images8=0, no_images16=0, strong_split=1, strong_reuse=1, refine_lanes=1, eval_items=1, sweep_split=1,
                sweep_force=0, anchor_tab_off=0, gn_wave=0, ransac_wave=0, cand_mask_mode=-1, weak_phased=1,
                weak_phased_min=8192, run0=64, run1=256, run2=1024, run3=1024, group0=1, group1=4, group2=4, group3=2,
                weak_split_colours=0, sweep_band_gb=0.0)
    for v in (UNSET, "0", "1", "2"):
        env(**{WIDE: v})
        assert switches() == want, v


def test_nothing_else_moves(env):
    """every other decision of emu_forms_decide is the same with the switch at any value"""
    keys = ("weak", "group0", "group1", "group2", "group3", "run0", "run1", "run2", "run3", "joins", "sweep", "second_eval",
            "border_kernel", "band_rows", "masked", "format")
    base = {S: decide(S=S) for S in (5, 17, 31)}
    for v in ("1", "2"):
        env(**{WIDE: v})
        for S in base:
            f = decide(S=S)
            assert {k: f[k] for k in keys} == {k: base[S][k] for k in keys}, (v, S)
