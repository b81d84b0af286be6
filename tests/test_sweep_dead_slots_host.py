"""The two end slots of DepthToWeak's cost line (disparity offsets -30 and +30; dvp_forms.hpp: sweep_slot_read) are read by no
decision, so the sweep site neither evaluates nor fetches them.  On the host emulation of the device headers (tests/emul, built with
the site's test entry points into tests/sweep_host): every form
of the site (view-compacted passes, the fused kernel, the two separate kernels) leaves the oracle's bits, and the bits of the same
run with DVP_SWEEP_ALL_SLOTS=1, which evaluates all 61 slots as before.

The state the site starts from is built directly (the planes of the scene with noise, random view selections and weights): the site
reads nothing else, and a wide baseline with a wide depth range puts both end slots INSIDE the depth range — with the parity
scenes' 0.4 baseline at 96x64 the disparity is about 8 and both are outside it everywhere, which would test nothing."""
import numpy as np
import pytest

from conftest import synth, make_params, count_diff
from oracle import oracle as O
from tests.sweep_host import sweep_host as E

W, H = 96, 64
L = W * H
FILL = np.float32(-7.0)   # tests/emul fills sweep_cost with it before the site: "a value no decision may ever read"
OUT = ("weak_info", "planes", "radius", "selected_views")
MODES = {"refine_geom": dict(state=synth.REFINE_ITER, geom_consistency=1), "first": dict(state=synth.FIRST_INIT, geom_consistency=0)}

_scenes, _oracles = {}, {}


def scene(S, flat=False):
    key = (S, flat)
    if key not in _scenes:
        sc = synth.make_scene(W, H, S, baseline=2.5)
        if flat:   # black in every view (variance exactly 0): every cost of a line there is 2, the line has no peak (the reference's min_peak == 0)
            sc["images"] = sc["images"].copy()
            sc["images"][:, 14:50, 20:76] = np.float32(0.0)
        rng = np.random.default_rng(7 + S)
        n = np.tile(sc["normal_gt"], (L, 1)) + rng.normal(0, 0.02, (L, 3)).astype(np.float32)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        depth = (sc["depth_gt"][0].reshape(-1) * (1 + rng.normal(0, 0.004, L))).astype(np.float32)
        depth[rng.random(L) < 0.01] = 0                       # no depth: UNKNOWN
        views = rng.integers(1, 1 << S, L).astype(np.uint32)
        views[rng.random(L) < 0.01] = 0                       # no view selected: UNKNOWN
        vw = rng.integers(1, 256, (L, 32)).astype(np.uint8)
        vw[rng.random((L, 32)) < 0.2] = 0                     # selected views of weight 0 are skipped
        vw[rng.random(L) < 0.01] = 0                          # weight sum 0: LocalRefine's own guard
        radius = np.full(L, 5, np.int32)
        radius[rng.random(L) < 0.1] = 0                       # DepthToWeak sets these
        st = dict(planes=np.concatenate([n, depth[:, None]], 1).astype(np.float32), views=views, edge=sc["edge"], label=sc["label"],
                  radius=radius, weak=np.full(L, synth.STRONG, np.uint8))
        _scenes[key] = (sc, st, vw)
    return _scenes[key]


def params(S, mode, wpr, depth_min=0.5, depth_max=100.0):
    return make_params(S + 1, max_iterations=1, use_APD=1, weak_peak_radius=wpr, depth_min=np.float32(depth_min), depth_max=np.float32(depth_max), **MODES[mode])


def engine(cls, S, p, flat=False):
    sc, st, vw = scene(S, flat)
    e = O.from_scene(sc, p, depths=sc["depth_gt"] if p["geom_consistency"] else None, cls=cls)
    e.upload_state(**st)
    e.set("view_weight", vw)
    return e


def oracle_result(S, mode, wpr, flat=False, **rng):
    key = (S, mode, wpr, flat, tuple(sorted(rng.items())))
    if key not in _oracles:
        o = engine(O.Oracle, S, params(S, mode, wpr, **rng), flat)
        o.run_stage("depth_to_weak")
        o.run_stage("local_refine")
        _oracles[key] = {n: o.get(n).copy() for n in OUT}
    return _oracles[key]


def run_site(S, mode, wpr, form, all_slots, monkeypatch, flat=False, **rng):
    """the site on the emulation in one form, the end slots skipped (the default) or evaluated"""
    monkeypatch.setenv("DVP_SWEEP_ALL_SLOTS", "1" if all_slots else "0")
    monkeypatch.setenv("DVP_SWEEP_SPLIT", "2" if form == "passes" else "0")   # 2: the passes also without the geometric term
    e = engine(E.SweepEmul, S, params(S, mode, wpr, **rng), flat)
    e.read_switches()
    e.count_evals(True)
    if form == "separate":
        e.run_stage("depth_to_weak")
        e.run_stage("local_refine")
    else:
        e.run_site(form == "passes")
    return e


def sweep_field(e, v, f):
    return e.sweep_field(v, f)


def window(wpr):
    """dvp_forms.hpp: sweep_window.  At 30 (weak_peak_radius >= 29) the whole line is the first stage and the end slots stay
    (sweep_slot_read): the switch changes nothing there."""
    return min(max(wpr + 1, 5), 30)


def check(S, mode, wpr, form, monkeypatch, flat=False, **rng):
    want = oracle_result(S, mode, wpr, flat, **rng)
    skip = run_site(S, mode, wpr, form, False, monkeypatch, flat, **rng)
    full = run_site(S, mode, wpr, form, True, monkeypatch, flat, **rng)
    for n in OUT:
        assert count_diff(skip.get(n), want[n]) == 0, n
        assert count_diff(skip.get(n), full.get(n)) == 0, n
    assert skip.evals() <= full.evals()
    if form == "passes" and window(wpr) < 30:
        # the end slots' fields keep the fill value: nothing wrote them, and a decision that read them would have met -7
        for v in range(S):
            for f in (0, 60):
                assert (sweep_field(skip, v, f) == FILL).all(), (v, f)
    return skip, full, want


@pytest.mark.parametrize("wpr", [2, 4, 6, 28, 29, 30])
@pytest.mark.parametrize("form", ["passes", "fused", "separate"])
@pytest.mark.parametrize("mode", ["refine_geom", "first"])
@pytest.mark.parametrize("S", [3, 9])
def test_every_form_leaves_the_oracles_bits(S, mode, form, wpr, monkeypatch):
    skip, full, want = check(S, mode, wpr, form, monkeypatch)
    w = want["weak_info"]
    assert (w == synth.STRONG).sum() > 0 and (w == synth.WEAK).sum() > 0 and (w == synth.UNKNOWN).sum() > 0
    # both end slots are inside the depth range somewhere, so the switch really adds evaluations
    assert (skip.evals() < full.evals()) == (window(wpr) < 30)


def line_geometry(S, p):
    """per pixel, in the engine's float arithmetic (sweep_prepare_px): is the site's pixel valid, and are the slots -30 / +30 inside
    the depth range"""
    sc, st, vw = scene(S)
    cams = sc["cameras"]
    c = cams["c"].astype(np.float32)
    base = np.zeros(L, np.float32)
    valid = np.zeros(L, np.int32)
    for v in range(S):
        d = c[0] - c[v + 1]
        bl = np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        on = (st["views"] >> v) & 1 == 1
        base = np.where(on, base + bl, base).astype(np.float32)
        valid += on
    depth = st["planes"][:, 3]
    ok = (valid > 0) & (depth != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        base = (base / valid.astype(np.float32)).astype(np.float32)
        k0 = np.float32(cams["K"][0][0])
        num = (k0 * base).astype(np.float32)
        disp = (num / depth).astype(np.float32)
        inside = {}
        for pd in (-30, 30):
            pdep = (num / (disp + np.float32(pd)).astype(np.float32)).astype(np.float32)
            inside[pd] = ok & ~((pdep < p["depth_min"]) | (pdep > p["depth_max"]))
    return ok, inside


@pytest.mark.parametrize("wpr", [4, 6])   # (at 28 stage 1 holds the end slots only: no other field tells which pairs it took)
def test_the_switch_adds_exactly_the_end_slots_evaluations(wpr, monkeypatch):
    """evaluations(all 61 slots) - evaluations(default) = the (pixel, selected view of weight > 0, end slot inside the depth range)
    triples of the pixels that reach stage 1, i.e. have a central peak.  Which (pixel, view) pairs stage 1 took is read from the cost
    buffer: one of its OTHER fields was written.  depth_max = 12 puts offset -30 outside the range for part of the image."""
    S, mode = 9, "refine_geom"
    p = params(S, mode, wpr, depth_max=12.0)
    skip, full, want = check(S, mode, wpr, "passes", monkeypatch, depth_max=12.0)
    ok, inside = line_geometry(S, p)
    assert 0 < inside[-30].sum() < ok.sum() and inside[30].sum() > 0
    cw = window(wpr)
    fields = [f for f in range(1, 60) if abs(f - 30) > cw]
    expected = 0
    for v in range(S):
        took = np.zeros(L, bool)
        for f in fields:
            took |= sweep_field(skip, v, f) != FILL
        assert (took <= ok).all()
        expected += int((took & inside[-30]).sum() + (took & inside[30]).sum())
        # ... and with the switch exactly these end-slot fields are written
        assert ((sweep_field(full, v, 0) != FILL) == (took & inside[-30])).all()
        assert ((sweep_field(full, v, 60) != FILL) == (took & inside[30])).all()
    assert expected > 0
    assert full.evals() - skip.evals() == expected


@pytest.mark.parametrize("form", ["passes", "fused", "separate"])
@pytest.mark.parametrize("wpr", [4, 30])
def test_a_line_without_any_peak(form, wpr, monkeypatch):
    """a black region: every cost is 2, the line has no peak, the reference reads p_costs[min_peak] with min_peak == 0 —
    the only read of the first entry.  The engine decides WEAK before that (no central peak); weak_peak_radius 30 is the one value at
    which the reference's `|min_peak - 30| > weak_peak_radius` does not decide first."""
    skip, full, want = check(9, "refine_geom", wpr, form, monkeypatch, flat=True)
    ok, _ = line_geometry(9, params(9, "refine_geom", wpr))   # (the state does not depend on the images)
    inner = np.zeros((H, W), bool)
    inner[26:38, 34:62] = True   # every patch tap inside the black block
    inner &= ok.reshape(H, W)
    assert inner.sum() > 200
    assert (want["weak_info"].reshape(H, W)[inner] == synth.WEAK).all()
    assert (skip.get("weak_info").reshape(H, W)[inner] == synth.WEAK).all()
