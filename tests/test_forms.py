"""The form every launch site takes (dvp-mvs_amd/csrc/dvp_forms.hpp): the parsed switches and the decision functions, through
the two exports of the host-emulation library, against the rule written out here — taken from dvp_ctx_create and launch_stage as
they stood before the rule moved into the header."""
import ctypes
import itertools
import math

import pytest

from tests.emul import emul as E

UNSET = None
TRI = (UNSET, "0", "1")
ALL_VARS = ["DVP_NO_IMAGES8", "DVP_NO_IMAGES16", "DVP_STRONG_SPLIT", "DVP_STRONG_REUSE", "DVP_REFINE_LANES", "DVP_EVAL_ITEMS",
            "DVP_SWEEP_SPLIT", "DVP_SWEEP_BAND_GB", "DVP_WEAK_ANCHOR_TAB", "DVP_GN_WAVE", "DVP_RANSAC_WAVE", "DVP_CAND_MASK",
            "DVP_WEAK_PHASED", "DVP_WEAK_PHASED_MIN", "DVP_WEAK_RUNS", "DVP_WEAK_GROUPS", "DVP_WEAK_SPLIT_COLOURS"]
# order of emu_forms_switches' output
SW_FIELDS = ["no_images8", "no_images16", "strong_split", "strong_reuse", "refine_lanes", "eval_items", "sweep_split", "sweep_force",
             "anchor_tab_off", "gn_wave", "ransac_wave", "cand_mask_mode", "weak_phased", "weak_phased_min",
             "run0", "run1", "run2", "run3", "group0", "group1", "group2", "group3", "weak_split_colours"]
# order of emu_forms_decide's input and output
IN_FIELDS = ["S", "split_fits", "reuse_hdr", "big_images", "table_present", "table_fits", "phase_fits", "count", "fused", "geom",
             "weak_peak_radius", "sweep_fits", "W", "H", "weak_count", "mask_fits", "inexact"]
OUT_FIELDS = ["strong", "eval_items", "decide", "refine_lanes", "plan", "weak", "group0", "group1", "group2", "group3",
              "run0", "run1", "run2", "run3", "joins", "sweep", "second_eval", "border_kernel", "band_rows", "masked", "format"]
SPLIT, MONO_V8, MONO_V16, MONO = 0, 1, 2, 3
PHASED, WAVE, WAVE_NOTAB = 0, 1, 2
PASSES, FUSED, SEPARATE = 0, 1, 2
DEFAULT_IN = dict(S=5, split_fits=1, reuse_hdr=1, big_images=0, table_present=1, table_fits=1, phase_fits=1, count=10000, fused=1, geom=1,
                  weak_peak_radius=4, sweep_fits=1, W=64, H=48, weak_count=100, mask_fits=1, inexact=0)


@pytest.fixture
def env(monkeypatch):
    for v in ALL_VARS:
        monkeypatch.delenv(v, raising=False)

    def set_(**kw):
        for k, v in kw.items():
            if v is UNSET:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
    return set_


def switches():
    out = (ctypes.c_int * len(SW_FIELDS))()
    gb = ctypes.c_double()
    E.lib().emu_forms_switches(out, ctypes.byref(gb))
    d = dict(zip(SW_FIELDS, out))
    d["sweep_band_gb"] = gb.value
    return d


def decide(**kw):
    a = dict(DEFAULT_IN, **kw)
    inp = (ctypes.c_int * len(IN_FIELDS))(*[int(a[k]) for k in IN_FIELDS])
    out = (ctypes.c_int * len(OUT_FIELDS))()
    E.lib().emu_forms_decide(inp, out)
    return dict(zip(OUT_FIELDS, out))


def on(v, unset):
    """atoi(e) != 0, or the default when the variable is not set"""
    return unset if v is UNSET else v != "0"


def test_defaults(env):
    assert switches() == dict(no_images8=0, no_images16=0, strong_split=1, strong_reuse=1, refine_lanes=1, eval_items=1, sweep_split=1,
                              sweep_force=0, anchor_tab_off=0, gn_wave=0, ransac_wave=0, cand_mask_mode=-1, weak_phased=1,
                              weak_phased_min=8192, run0=64, run1=256, run2=1024, run3=1024, group0=1, group1=4, group2=4, group3=2,
                              weak_split_colours=0, sweep_band_gb=0.0)


@pytest.mark.parametrize("var,field,unset,inverted", [
    ("DVP_STRONG_SPLIT", "strong_split", 1, False), ("DVP_STRONG_REUSE", "strong_reuse", 1, False), ("DVP_REFINE_LANES", "refine_lanes", 1, False),
    ("DVP_EVAL_ITEMS", "eval_items", 1, False), ("DVP_SWEEP_SPLIT", "sweep_split", 1, False), ("DVP_WEAK_ANCHOR_TAB", "anchor_tab_off", 0, True),
    ("DVP_GN_WAVE", "gn_wave", 0, False), ("DVP_RANSAC_WAVE", "ransac_wave", 0, False), ("DVP_WEAK_PHASED", "weak_phased", 1, False)])
def test_numeric_switches(env, var, field, unset, inverted):
    base = switches()
    for v, want in ((UNSET, unset), ("0", int(inverted)), ("1", int(not inverted)), ("2", int(not inverted)), ("", int(inverted)), ("x", int(inverted))):
        env(**{var: v})
        got = switches()
        assert got[field] == want, (var, v)
        assert {k: x for k, x in got.items() if k not in (field, "sweep_force")} == {k: x for k, x in base.items() if k not in (field, "sweep_force")}, (var, v)


def test_other_switches(env):
    for v, want in ((UNSET, (1, 0)), ("0", (0, 0)), ("1", (1, 0)), ("2", (1, 1)), ("3", (1, 0))):
        env(DVP_SWEEP_SPLIT=v)
        s = switches()
        assert (s["sweep_split"], s["sweep_force"]) == want, v
    env(DVP_SWEEP_SPLIT=UNSET)
    for var, field in (("DVP_NO_IMAGES8", "no_images8"), ("DVP_NO_IMAGES16", "no_images16"), ("DVP_WEAK_SPLIT_COLOURS", "weak_split_colours")):
        for v in ("0", "1", ""):   # presence only
            env(**{var: v})
            assert switches()[field] == 1, (var, v)
        env(**{var: UNSET})
        assert switches()[field] == 0
    for v, want in ((UNSET, -1), ("0", 0), ("1", 1), ("7", 1), ("", 0)):
        env(DVP_CAND_MASK=v)
        assert switches()["cand_mask_mode"] == want, v
    for v, want in ((UNSET, 8192), ("0", 0), ("-3", -3), ("500", 500), ("x", 0)):
        env(DVP_WEAK_PHASED_MIN=v)
        assert switches()["weak_phased_min"] == want, v
    for v, want in ((UNSET, 0.0), ("24", 24.0), ("0.0004", 0.0004), ("x", 0.0)):
        env(DVP_SWEEP_BAND_GB=v)
        assert switches()["sweep_band_gb"] == want, v


def test_weak_lists(env):
    runs, groups = (64, 256, 1024, 1024), (1, 4, 4, 2)

    def got():
        s = switches()
        return tuple(s["run%d" % i] for i in range(4)), tuple(s["group%d" % i] for i in range(4))
    # malformed lists leave the defaults
    for bad in ("", "3", "1,2,3", "1,2,3,x", "a,b,c,d", "1;2;3;4", "1,2,,4"):
        env(DVP_WEAK_RUNS=bad, DVP_WEAK_GROUPS=bad)
        assert got() == (runs, groups), bad
    env(DVP_WEAK_RUNS="0,-5,7,100000", DVP_WEAK_GROUPS=UNSET)
    assert got() == ((1, 1, 7, 100000), groups)
    env(DVP_WEAK_RUNS=UNSET, DVP_WEAK_GROUPS="0,9,3,-1")
    assert got() == (runs, (1, 4, 3, 1))
    env(DVP_WEAK_GROUPS="4,4,4,4,9")   # what follows four numbers is ignored; E0 is capped at two pixels per wave at the launch
    assert got() == (runs, (4, 4, 4, 4))
    f = decide()
    assert [f["group%d" % i] for i in range(4)] == [2, 4, 4, 4] and [f["run%d" % i] for i in range(4)] == list(runs)
    env(DVP_WEAK_GROUPS=UNSET, DVP_WEAK_RUNS="8,16,32,48")
    f = decide()
    assert [f["group%d" % i] for i in range(4)] == list(groups) and [f["run%d" % i] for i in range(4)] == [8, 16, 32, 48]


def test_strong_update(env):
    for split, items, lanes in itertools.product(TRI, repeat=3):
        env(DVP_STRONG_SPLIT=split, DVP_EVAL_ITEMS=items, DVP_REFINE_LANES=lanes)
        for S, fits, hdr, big in itertools.product((1, 4, 5, 8, 9, 12, 16, 17, 31), (0, 1), (0, 1), (0, 1)):
            f = decide(S=S, split_fits=fits, reuse_hdr=hdr, big_images=big)
            is_split = on(split, True) and fits and S <= 16
            key = (split, items, lanes, S, fits, hdr, big)
            if is_split:
                assert f["strong"] == SPLIT, key
                assert f["eval_items"] == on(items, True), key
                assert f["decide"] == next(m for m in (4, 6, 8, 10, 12, 16) if S <= m), key
                assert f["refine_lanes"] == (on(lanes, True) and not big), key   # a set of 4 GiB or more: 32-bit offsets do not reach
                assert f["plan"] == hdr, key
            else:
                assert f["strong"] == (MONO_V8 if S <= 8 else (MONO_V16 if S <= 16 else MONO)), key
                assert (f["eval_items"], f["decide"], f["refine_lanes"], f["plan"]) == (0, 0, 0, 0), key
    # a few rows in full
    env(DVP_STRONG_SPLIT=UNSET, DVP_EVAL_ITEMS=UNSET, DVP_REFINE_LANES=UNSET)
    got = lambda **kw: tuple(decide(**kw)[k] for k in ("strong", "eval_items", "decide", "refine_lanes", "plan"))
    assert got(S=9) == (SPLIT, 1, 10, 1, 1)
    assert [got(S=S)[2] for S in range(1, 18)] == [4, 4, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 16, 16, 16, 16, 0]
    assert [got(S=S, split_fits=0)[0] for S in (7, 8, 9, 16, 17)] == [MONO_V8, MONO_V8, MONO_V16, MONO_V16, MONO]
    assert got(S=9, big_images=1) == (SPLIT, 1, 10, 0, 1)
    assert got(S=16, reuse_hdr=0) == (SPLIT, 1, 16, 1, 0)
    assert got(S=17) == (MONO, 0, 0, 0, 0)
    assert got(S=9, split_fits=0) == (MONO_V16, 0, 0, 0, 0)
    env(DVP_STRONG_SPLIT="0")
    assert got(S=8) == (MONO_V8, 0, 0, 0, 0)


def test_weak_update(env):
    for phased, tab, minv, colours in itertools.product(TRI, TRI, (UNSET, "0"), (UNSET, "1")):
        env(DVP_WEAK_PHASED=phased, DVP_WEAK_ANCHOR_TAB=tab, DVP_WEAK_PHASED_MIN=minv, DVP_WEAK_SPLIT_COLOURS=colours)
        for present, tfits, pfits, count in itertools.product((0, 1), (0, 1), (0, 1), (0, 8191, 8192)):
            f = decide(table_present=present, table_fits=tfits, phase_fits=pfits, count=count)
            key = (phased, tab, minv, colours, present, tfits, pfits, count)
            if not present:
                want = WAVE_NOTAB
            elif on(phased, True) and pfits and (minv == "0" or count >= 8192):
                want = PHASED
            else:
                want = WAVE
            assert f["weak"] == want, key
            assert f["joins"] == (on(phased, True) and pfits and on(tab, True) and tfits and colours is UNSET), key
    env(DVP_WEAK_PHASED=UNSET, DVP_WEAK_ANCHOR_TAB=UNSET, DVP_WEAK_SPLIT_COLOURS=UNSET, DVP_WEAK_PHASED_MIN="-1")
    assert decide(count=1)["weak"] == PHASED
    env(DVP_WEAK_PHASED_MIN="100")
    assert [decide(count=n)["weak"] for n in (99, 100)] == [WAVE, PHASED]
    # rows in full: (DVP_WEAK_PHASED, DVP_WEAK_ANCHOR_TAB, DVP_WEAK_SPLIT_COLOURS, table_fits, phase_fits) -> one launch site for both colours
    env(DVP_WEAK_PHASED_MIN=UNSET)
    for row, want in (((UNSET, UNSET, UNSET, 1, 1), 1), (("0", UNSET, UNSET, 1, 1), 0), ((UNSET, "0", UNSET, 1, 1), 0), ((UNSET, UNSET, "1", 1, 1), 0),
                      ((UNSET, UNSET, "0", 1, 1), 0), ((UNSET, UNSET, UNSET, 0, 1), 0), ((UNSET, UNSET, UNSET, 1, 0), 0), (("1", "1", UNSET, 1, 1), 1)):
        env(DVP_WEAK_PHASED=row[0], DVP_WEAK_ANCHOR_TAB=row[1], DVP_WEAK_SPLIT_COLOURS=row[2])
        assert decide(table_fits=row[3], phase_fits=row[4])["joins"] == want, row


def test_sweeps(env):
    for sw in TRI + ("2",):
        env(DVP_SWEEP_SPLIT=sw)
        for fused, geom, fits, wpr, (W, H) in itertools.product((0, 1), (0, 1), (0, 1), (4, 29), ((11, 40), (12, 12), (40, 11))):
            f = decide(fused=fused, geom=geom, sweep_fits=fits, weak_peak_radius=wpr, W=W, H=H)
            key = (sw, fused, geom, fits, wpr, W, H)
            if fused and on(sw, True) and fits and (geom or sw == "2"):
                assert (f["sweep"], f["second_eval"], f["border_kernel"]) == (PASSES, int(wpr == 4), int(W >= 12 and H >= 12)), key
            else:
                assert (f["sweep"], f["second_eval"], f["border_kernel"]) == (FUSED if fused else SEPARATE, 0, 0), key
    env(DVP_SWEEP_SPLIT=UNSET)
    assert [decide(weak_peak_radius=r)["second_eval"] for r in (0, 28, 29, 30, 100)] == [1, 1, 0, 0, 0]


def band_rows(W, H, S, gb):
    """ensure_sweep_buffers' arithmetic: 73 floats per (pixel, view), pixels rounded up to groups of 64; bands of whole 14-row tiles"""
    if not gb > 0.0:
        return 0
    whole = (W * H + 63) // 64 * 64 * S * 73 * 4
    bands = math.ceil(whole / (gb * 1e9))
    if bands <= 1:
        return 0
    rows = (-(-H // bands) + 13) // 14 * 14
    return rows if rows < H else 0


def test_sweep_band_rows(env):
    cases = [(6208, 4128, 9, "24", 1386), (150, 97, 4, "0.0004", 14), (150, 97, 4, "0.006", 42),
             (150, 97, 4, "1", 0), (150, 97, 4, "0", 0), (150, 97, 4, "-1", 0), (150, 97, 4, "0.009", 56), (150, 97, 4, "0.02", 0), (64, 20, 2, "0.00001", 14), (64, 14, 2, "0.00001", 0)]
    for W, H, S, gb, want in cases:
        env(DVP_SWEEP_BAND_GB=gb)
        assert band_rows(W, H, S, float(gb)) == want, (W, H, S, gb)
        assert decide(W=W, H=H, S=S)["band_rows"] == want, (W, H, S, gb)
    env(DVP_SWEEP_BAND_GB=UNSET)
    assert decide(W=6208, H=4128, S=9)["band_rows"] == 0


def test_candidates(env):
    for mode in TRI:
        env(DVP_CAND_MASK=mode)
        for wc, fits in itertools.product((0, 1, 399, 400, 401, 10000), (0, 1)):   # L = 100 x 100: 4 % = 400 WEAK pixels
            want = wc > 0 and fits and (mode == "1" or (mode is UNSET and wc * 25 < 10000))
            assert decide(W=100, H=100, weak_count=wc, mask_fits=fits)["masked"] == want, (mode, wc, fits)
    # rows in full: (DVP_CAND_MASK, WEAK pixels of 10000, mask_fits) -> masked
    for row, want in (((UNSET, 399, 1), 1), ((UNSET, 400, 1), 0), ((UNSET, 0, 1), 0), ((UNSET, 399, 0), 0), (("1", 10000, 1), 1), (("1", 10000, 0), 0),
                      (("1", 0, 1), 0), (("0", 1, 1), 0)):
        env(DVP_CAND_MASK=row[0])
        assert decide(W=100, H=100, weak_count=row[1], mask_fits=row[2])["masked"] == want, row


def test_image_format(env):
    for no8, no16 in itertools.product((UNSET, "1"), repeat=2):
        env(DVP_NO_IMAGES8=no8, DVP_NO_IMAGES16=no16)
        for bits in (0, 1, 2, 3):
            want = 1 if (bits == 0 and no8 is UNSET) else (2 if (bits == 1 and no8 is UNSET and no16 is UNSET) else 0)
            assert decide(inexact=bits)["format"] == want, (no8, no16, bits)
