"""Wide-baseline and degenerate-hypothesis geometry (tests/wide_geometry.py) on the CPU: the class guards, the oracle against the
host emulation of the kernels bit for bit — the twin of every test of tests/test_gpu_wide_geometry.py, so that a GPU failure next
to a green twin points at a primitive whose device branch is other text than its host branch — and the oracle
against the float64 reading of the reference's source (tests/np_model.py) where that model is well conditioned."""
import numpy as np
import pytest

from conftest import make_params, count_diff, stage_sequence, CHECKED, first_pass_state, synth
from oracle import oracle as O
from tests.emul import emul as E
from test_edge_cases import image_set
import np_model as M
import test_forms as TF
import wide_geometry as G

pytestmark = pytest.mark.hostbox

W, H = 96, 64          # the smallest size at which the rig keeps the epipole and all six sources in view
S_KAT, S_PASS = 6, 5
KAT_CLASSES = {"C0": G.hypotheses_ordinary, "C1": G.hypotheses_straddling, "C2": G.hypotheses_far_outside,
               "C4": G.hypotheses_special}
FORM_KEYS = ("planes", "costs", "selected_views", "view_weight", "weak_info", "radius", "neighbours", "weak_reliable")

_MEMBERS = {}


def members(name, count=4096):
    """(px, planes, view) of a class on the KAT scene, generated once"""
    if (name, count) not in _MEMBERS:
        f = G.hypotheses_behind if name == "C3" else KAT_CLASSES[name]
        _MEMBERS[(name, count)] = f(G.scene(W, H, S_KAT), count=count)
    return _MEMBERS[(name, count)]


def emul_pair(scene, params, state, seed=1234, sampler=0, depths=None):
    a = O.from_scene(scene, params, seed=seed, sampler=sampler, depths=depths, cls=O.Oracle)
    b = O.from_scene(scene, params, seed=seed, sampler=sampler, depths=depths, cls=E.Emul)
    a.upload_state(**state)
    b.upload_state(**state)
    return a, b


def run_and_compare(a, b, iters, names=CHECKED):
    for st, it, col in stage_sequence(iters):
        a.run_stage(st, it, col)
        b.run_stage(st, it, col)
        for n in names:
            nd = count_diff(a.get(n), b.get(n))
            assert nd == 0, "%s differs in %d entries after %s(it=%d, colour=%d)" % (n, nd, st, it, col)


# ---- the cases, shared with the GPU file: `pair` makes (oracle, engine under test) -----------------------------------------------
def kat_case(pair, name, sampler):
    """eval_cost_vectors of the engine == the oracle's, every view of every member; on C1 every member is evaluated in the view
    it targets (not rejected at the centre test): as many costs below 2 as the classifier counted members"""
    sc = G.scene(W, H, S_KAT)
    p = G.wide_params(make_params, S_KAT + 1)
    a, b = pair(sc, p, first_pass_state(sc), sampler=sampler)
    px, planes, view = members(name)
    assert len(px) == 4096
    ca, cb = a.eval_cost_vectors(px, planes), b.eval_cost_vectors(px, planes)
    assert count_diff(ca, cb) == 0
    tgt = cb[np.arange(len(px)), view - 1]
    print("%s sampler %d: %d members, %d costs below 2 in the targeted view, %d distinct, %d NaN" %
          (name, sampler, len(px), int((tgt < 2).sum()), len(np.unique(tgt)), int(np.isnan(cb).sum())))
    if name == "C1":
        assert int((tgt < 2).sum()) == len(px)
        assert len(np.unique(tgt)) > 4000


def first_pass_case(pair, compare, sampler):
    sc = G.scene(W, H, S_PASS)
    p = G.wide_params(make_params, S_PASS + 1, max_iterations=2, state=synth.FIRST_INIT, use_APD=0)
    a, b = pair(sc, p, first_pass_state(sc), sampler=sampler)
    compare(a, b, 2)


def refine_inputs(images="int", monkeypatch=None, iters=2):
    """scene, params, state of the REFINE_ITER pass: arbitrary_state with the shallow C3 planes in a 16 x 16 block"""
    sc, fmt = image_set(G.scene(W, H, S_PASS), images, monkeypatch)
    st = G.arbitrary_state(sc, np.random.default_rng(7))
    behind = G.write_behind_block(sc, st)
    assert behind >= 200, behind       # of 256: the geometric term meets sd <= 0
    p = G.wide_params(make_params, S_PASS + 1, max_iterations=iters, state=synth.REFINE_ITER, use_APD=1, geom_consistency=1,
                      weak_peak_radius=4)
    return sc, fmt, p, st


def refine_pass_case(pair, compare, images, monkeypatch):
    sc, fmt, p, st = refine_inputs(images, monkeypatch)
    a, b = pair(sc, p, st, depths=sc["depth_gt"])
    assert b.image_format() == fmt
    assert a.weak_count() == b.weak_count() > 700
    compare(a, b, 2)
    wi = b.get("weak_info")
    print("REFINE_ITER %s: weak_count %d; weak_info after two iterations: %d WEAK, %d STRONG, %d UNKNOWN" %
          (images, b.weak_count(), int((wi == synth.WEAK).sum()), int((wi == synth.STRONG).sum()), int((wi == synth.UNKNOWN).sum())))
    assert (b.get("weak_reliable") == 1).sum() > 0


_FORMS_ORACLE = {}


def forms_oracle():
    """the one oracle run every form is compared with"""
    if not _FORMS_ORACLE:
        sc, _, p, st = refine_inputs()
        o = O.from_scene(sc, p, depths=sc["depth_gt"])
        o.upload_state(**st)
        assert o.weak_count() > 700
        o.run_patchmatch()
        _FORMS_ORACLE.update({k: o.get(k) for k in FORM_KEYS})
    return _FORMS_ORACLE


FORMS = {
    "strong_split": {},
    "strong_lockstep_refine": {"DVP_REFINE_LANES": "0"},
    "strong_monolithic": {"DVP_STRONG_SPLIT": "0"},
    "strong_streaming_decide": {"DVP_STRONG_WIDE": "2"},
    "strong_no_reuse": {"DVP_STRONG_REUSE": "0"},
    "sweep_passes": {"DVP_SWEEP_SPLIT": "2"},
    "sweep_fused": {"DVP_SWEEP_SPLIT": "0"},
    "weak_one_wave": {"DVP_WEAK_PHASED": "0"},
    "weak_per_item_anchors": {"DVP_WEAK_ANCHOR_TAB": "0"},
    "weak_short_runs": {"DVP_WEAK_RUNS": "1,2,3,8", "DVP_WEAK_GROUPS": "2,3,1,3"},
}
# what the launch-site rule (csrc/dvp_forms.hpp, read through the emulation library's exports as tests/test_forms.py does) must
# decide for the pass in each form: strong kernel and decision bracket, weak kernel, sweep kernel
FORM_DECISIONS = {
    "strong_split": (TF.SPLIT, 6, TF.PHASED, TF.PASSES),
    "strong_lockstep_refine": (TF.SPLIT, 6, TF.PHASED, TF.PASSES),
    "strong_monolithic": (TF.MONO_V8, 0, TF.PHASED, TF.PASSES),
    "strong_streaming_decide": (TF.SPLIT, 32, TF.PHASED, TF.PASSES),
    "strong_no_reuse": (TF.SPLIT, 6, TF.PHASED, TF.PASSES),
    "sweep_passes": (TF.SPLIT, 6, TF.PHASED, TF.PASSES),      # with the geometric term on, what the default decides too
    "sweep_fused": (TF.SPLIT, 6, TF.PHASED, TF.FUSED),
    "weak_one_wave": (TF.SPLIT, 6, TF.WAVE, TF.PASSES),
    "weak_per_item_anchors": (TF.SPLIT, 6, TF.WAVE_NOTAB, TF.PASSES),
    "weak_short_runs": (TF.SPLIT, 6, TF.PHASED, TF.PASSES),
}


def check_form_decisions(form, weak_count):
    """The environment of `form` makes the rule decide the form that the case's name says, for this pass' shape.  The engine and
    the emulation both take their forms from that rule; the C ABI reports the strong update's (dvp_strong_update_form), which the
    GPU test reads back as well."""
    sw = TF.switches()
    assert sw["weak_phased_min"] == 0      # (tests/conftest.py's default is pinned by forms_case: 780 WEAK pixels are below the engine's 8192)
    f = TF.decide(S=S_PASS, count=weak_count, weak_count=weak_count, fused=1, geom=1, weak_peak_radius=4, W=W, H=H,
                  table_present=0 if sw["anchor_tab_off"] else 1)
    assert (f["strong"], f["decide"], f["weak"], f["sweep"]) == FORM_DECISIONS[form], (form, f)
    assert f["refine_lanes"] == (0 if form in ("strong_lockstep_refine", "strong_monolithic") else 1)
    assert sw["strong_reuse"] == (0 if form == "strong_no_reuse" else 1)
    runs, groups = [f["run%d" % i] for i in range(4)], [f["group%d" % i] for i in range(4)]
    if form == "weak_short_runs":
        assert (runs, groups) == ([1, 2, 3, 8], [2, 3, 1, 3])
        # every evaluation launch walks tens of whole (run x group) blocks of the WEAK list; a colour's half of it ends in a partial one
        half = weak_count // 2
        assert all(half // (r * g) >= 16 for r, g in zip(runs, groups))
        print("weak_short_runs: %d WEAK pixels; blocks of %s pixels; remainders of the whole list %s" %
              (weak_count, [r * g for r, g in zip(runs, groups)], [weak_count % (r * g) for r, g in zip(runs, groups)]))
        assert any(weak_count % (r * g) for r, g in zip(runs, groups))
    else:
        assert (runs, groups) == ([64, 256, 1024, 1024], [1, 4, 4, 2])


def forms_case(make, form, monkeypatch):
    """run_patchmatch of the REFINE_ITER pass with the launch sites in form `form` == the oracle's run.  weak_short_runs: at run
    lengths 1, 2, 3, 8 the ~780 WEAK pixels cross several whole groups of the phased update's lists and leave a ragged tail.
    The environment is pinned here (every form switch unset, then the phased-update threshold, the masked candidates and the
    form's own variables) and the rule's decisions under it are asserted (check_form_decisions).  -> the engine"""
    for k in TF.ALL_VARS + ["DVP_STRONG_WIDE"]:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DVP_WEAK_PHASED_MIN", "0")     # the phased weak update also below 8192 WEAK pixels
    monkeypatch.setenv("DVP_CAND_MASK", "1")           # the masked candidate launch, as in every parity test
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    want = forms_oracle()
    sc, _, p, st = refine_inputs()
    b = make(sc, p, depths=sc["depth_gt"])
    b.upload_state(**st)
    check_form_decisions(form, b.weak_count())
    b.run_patchmatch()
    for k in FORM_KEYS:
        assert count_diff(want[k], b.get(k)) == 0, (form, k)
    return b


# ---- the classes and the rig -----------------------------------------------------------------------------------------------------
def test_rig_and_scene():
    """R R^T = I, the quarter turns and focal scales of the table, the forward camera's epipole inside the reference image, the
    rendered depths of every view inside the depth range the passes run with."""
    cams = G.rig(W, H)
    assert len(cams) == 7
    for cam, (c, roll, fs) in zip(cams, G.CAMERAS):
        R = cam["R"].reshape(3, 3).astype(np.float64)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.linalg.det(R) > 0.999
        got = np.degrees(np.arctan2(R[1, 0] - R[0, 1], R[0, 0] + R[1, 1]))      # the in-plane turn
        assert abs((got - roll + 180) % 360 - 180) < 10, (got, roll)
        assert R[2] @ (G.TARGET - np.asarray(c)) / np.linalg.norm(G.TARGET - np.asarray(c)) > 0.999   # looks at the target
        assert np.allclose(cam["c"], c, atol=1e-6)
        assert cam["K"][0] == np.float32(0.9 * W * fs) and abs(cam["K"][4] / cam["K"][0] - 1.01) < 1e-6
        assert cam["K"][2] != W / 2 and cam["K"][5] != H / 2
    e = G.epipole(cams[0], cams[G.FORWARD])
    print("epipole of the forward camera in the reference image: (%.1f, %.1f)" % (e[0], e[1]))
    assert 8 < e[0] < W - 8 and 8 < e[1] < H - 8
    for S in (S_PASS, S_KAT):
        sc = G.scene(W, H, S)
        assert sc["images"].shape == (S + 1, H, W) and sc["depth_gt"].shape == (S + 1, H, W) and len(sc["cameras"]) == S + 1
        assert sc["depth_gt"].min() > G.DEPTH_MIN and sc["depth_gt"].max() < G.DEPTH_MAX
        assert G.view_of(G.FORWARD, S) == 1 and G.view_of(G.SOURCE3, S) == 2
        assert sc["edge"].sum() > 0 and sc["flat"].sum() > 0 and set(np.unique(sc["label"])) >= {-1, 1, 2}
        for img in sc["images"]:
            assert img.std() > 10       # every view sees texture


def test_class_guards():
    """The classifier's own counts at 96 x 64 (no engine is asked).  Measured: C0 16275 of 24576 draws, C1 7278 of 20480,
    C2 8031 of 196608 (all but a handful against the forward camera; of the first 4096, 2611 have a tap beyond 1e6 pixels),
    C3 2779 of 3072; C4 is a list of 5600."""
    sc = G.scene(W, H, S_KAT)
    for name, f, guard in (("C0", G.hypotheses_ordinary, 500), ("C1", G.hypotheses_straddling, 500), ("C2", G.hypotheses_far_outside, 500),
                           ("C3", G.hypotheses_behind, 200), ("C4", G.hypotheses_special, 4096)):
        px, planes, view = f(sc, count=None)
        print("%s: %d members" % (name, len(px)))
        assert len(px) >= guard and planes.dtype == np.float32 and px.dtype == np.int32
        assert (px[:, 0] >= 0).all() and (px[:, 0] < W).all() and (px[:, 1] >= 0).all() and (px[:, 1] < H).all()
    # the properties, re-derived from the returned records
    px, planes, view = members("C1")
    c = G.classify(sc, view, px, planes)
    assert c["inside"].all() and c["straddles"].all() and (view == G.view_of(G.FORWARD, S_KAT)).all()
    px, planes, view = members("C2")
    c = G.classify(sc, view, px, planes)
    assert c["inside"].all() and (c["far"] > 1e4).all()
    print("C2: %d members with a tap beyond 1e6 pixels, %d of them not finite" % (int((c["far"] > 1e6).sum()), int(np.isinf(c["far"]).sum())))
    assert (c["far"] > 1e6).sum() > 500
    px, planes, view = members("C0")
    assert G.classify(sc, view, px, planes)["inside"].all() and len(np.unique(view)) == S_KAT
    px, planes, word = members("C3", 1024)
    sd = G.forward_point_depth(sc, G.view_of(G.FORWARD, S_KAT), px, planes)
    assert (sd <= 0).all() and (G.forward_point_depth(sc, G.view_of(G.SOURCE3, S_KAT), px, planes) > 0).all()
    px, planes, view = members("C4")
    w = planes[:, 3]
    assert np.isnan(w).any() and np.isposinf(w).any() and np.isneginf(w).any() and ((w == 0) & np.signbit(w)).any()
    assert ((w > 0) & (w < np.finfo(np.float32).tiny)).any() and (w == np.float32(3e38)).any() and (w == np.float32(1e-38)).any()
    assert np.isnan(planes[:, :3]).any() and (np.abs(planes[:, :3]).max(1) == 0).any() and (np.abs(planes[:, :3]) > 1e19).any()
    for corner in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
        assert ((px[:, 0] == corner[0]) & (px[:, 1] == corner[1])).any()
    # the 4096 records that are compared reach the inside of every border, not only its corners
    x, y = px[:, 0], px[:, 1]
    for name, on_border, along, length in (("left", x == 0, y, H), ("right", x == W - 1, y, H), ("top", y == 0, x, W), ("bottom", y == H - 1, x, W)):
        inner = along[on_border & (along > 0) & (along < length - 1)]
        assert len(np.unique(inner)) >= 25 and inner.max() - inner.min() > length // 2, (name, np.unique(inner))


def test_arbitrary_state():
    sc, fmt, p, st = refine_inputs()
    assert int((st["weak"] == synth.WEAK).sum()) > 700 and 50 < int((st["weak"] == synth.UNKNOWN).sum()) < 250
    assert len(np.unique(st["views"])) == 1 << S_PASS and st["views"].max() < (1 << S_PASS)
    n = np.linalg.norm(st["planes"][:, :3], axis=1)
    assert np.allclose(n, 1, atol=1e-5) and (st["planes"][:, 2] > 0).sum() > 1000      # normals that face away too


# ---- oracle == emulation, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [0, 1])
@pytest.mark.parametrize("name", ["C0", "C1", "C2", "C4"])
def test_cost_vectors_emulated_kernels(name, sampler):
    kat_case(emul_pair, name, sampler)


@pytest.mark.parametrize("sampler", [0, 1])
def test_cost_vectors_behind_emulated_kernels(sampler):
    """C3's shallow planes through the NCC as well (the geometric term meets them in the REFINE_ITER pass)"""
    sc = G.scene(W, H, S_KAT)
    a, b = emul_pair(sc, G.wide_params(make_params, S_KAT + 1), first_pass_state(sc), sampler=sampler)
    px, planes, _ = members("C3", 1024)
    assert count_diff(a.eval_cost_vectors(px, planes), b.eval_cost_vectors(px, planes)) == 0


@pytest.mark.parametrize("sampler", [0, 1])
def test_first_pass_stage_by_stage_emulated_kernels(sampler):
    first_pass_case(emul_pair, run_and_compare, sampler)


@pytest.mark.parametrize("images", ["int", "box", "scaled"])
def test_refine_pass_stage_by_stage_emulated_kernels(images, monkeypatch):
    """measured: weak_count 780; after two iterations weak_info holds 149 WEAK, 4213 STRONG, 1782 UNKNOWN pixels on the `int` set
    (`box`: 1212 / 3148 / 1784, `scaled`: 142 / 4219 / 1783)"""
    refine_pass_case(emul_pair, run_and_compare, images, monkeypatch)


@pytest.mark.parametrize("form", list(FORMS))
def test_forms_emulated_kernels(form, monkeypatch):
    forms_case(lambda sc, p, depths: O.from_scene(sc, p, depths=depths, cls=E.Emul), form, monkeypatch)


# ---- oracle against the float64 model ------------------------------------------------------------------------------------------------
def _model_scene():
    sc = G.scene(W, H, S_KAT)
    p = G.wide_params(make_params, S_KAT + 1, use_radius=0, geom_consistency=1)
    o = O.from_scene(sc, p, sampler=1, depths=sc["depth_gt"])
    o.upload_state(**first_pass_state(sc))
    cams = [M.cam64(c) for c in sc["cameras"]]
    imgs = [im.astype(np.float64) for im in sc["images"]]
    deps = [d.astype(np.float64) for d in sc["depth_gt"]]
    return sc, o, cams, imgs, deps


def _ncc_deviation(o, cams, imgs, px, planes, view):
    d = []
    for (x, y), pl, v in zip(px, planes, view):
        a = o.ncc_old(int(x), int(y), int(v), pl)
        b = M.ncc_old(imgs, cams, int(x), int(y), int(v), pl.astype(np.float64))
        d.append(abs(a - b))
    return np.array(d)


def test_ncc_ordinary_vs_numpy():
    """C0 at sampler 1, every member in the view it targets and in the forward camera: the bounds of test_numpy_kat.py
    (median < 2e-5, p99 < 5e-4, max < 5e-3), no member left out.
    Measured on 300 members (600 pairs): median 1.8e-06, p99 1.9e-05, max 3.5e-05."""
    sc, o, cams, imgs, _ = _model_scene()
    px, planes, view = members("C0")
    px, planes, view = px[:300], planes[:300], view[:300]
    d = np.concatenate([_ncc_deviation(o, cams, imgs, px, planes, view), _ncc_deviation(o, cams, imgs, px, planes, np.ones(len(px), int))])
    print("C0 ncc_old oracle vs numpy64: median %.2e p99 %.2e max %.2e on %d pairs" % (np.median(d), np.quantile(d, 0.99), d.max(), len(d)))
    assert np.median(d) < 2e-5 and np.quantile(d, 0.99) < 5e-4 and d.max() < 5e-3


def _geom_pairs(sc, o, cams, deps, px, planes, views):
    """the geometric term of every (member, view) pair on the oracle (a) and on the float64 model (b), without the pairs that the
    pixel-boundary guard of test_geom_cost_rotated_cameras_with_skew_vs_numpy leaves out; -> a, b, how many pairs were left out"""
    a, b, skipped = [], [], 0
    for (x, y), pl in zip(px, planes):
        for v in views:
            m = M.geom_cost(deps, cams, int(x), int(y), v, pl.astype(np.float64))
            if m is None:
                skipped += 1
                continue
            sx, sy, _ = M.project_on_camera(M.point_on_world(float(x), float(y), M.depth_from_plane(cams[0], pl.astype(np.float64), x, y), cams[0]), cams[v])
            if abs(sx - round(sx)) < 1e-3 or abs(sy - round(sy)) < 1e-3:
                skipped += 1
                continue
            a.append(o.geom_cost(int(x), int(y), v, pl))
            b.append(m)
    return np.array(a), np.array(b), skipped


def test_geom_ordinary_vs_numpy():
    """C0, the geometric term in every view: median < 1e-4, max < 5e-3 (test_numpy_kat.py's), pairs left out by the pixel-boundary
    guard only.  Measured on 200 members x 6 views: the guard leaves out 2 of 1200 pairs; median 0 (935 pairs saturate at 3 on both
    sides), the 263 un-saturated ones median 3.5e-06, max 3.8e-05."""
    sc, o, cams, _, deps = _model_scene()
    px, planes, _ = members("C0")
    a, b, skipped = _geom_pairs(sc, o, cams, deps, px[:200], planes[:200], range(1, S_KAT + 1))
    d = np.abs(a - b)
    un = b < 3.0
    print("C0 geom oracle vs numpy64: median %.2e max %.2e on %d pairs (%d left out by the guard); %d un-saturated: median %.2e max %.2e"
          % (np.median(d), d.max(), len(d), skipped, int(un.sum()), np.median(d[un]), d[un].max()))
    assert skipped <= 0.05 * (len(d) + skipped) and un.sum() > 100
    assert np.median(d) < 1e-4 and d.max() < 5e-3
    assert np.median(d[un]) < 1e-4


def test_geom_behind_vs_numpy():
    """C3: the forward point is behind the forward camera (its projection is the mirror image of where the point would be seen)
    and in front of source 3, where it projects far outside the image (the depth texel is a clamped border texel).  Only the
    outcomes are compared: where the float64 model saturates at 3.0 the oracle returns exactly 3.0; where it stays below 3 the
    oracle is within test_numpy_kat.py's 5e-3 of it.  Left out: the pixel-boundary guard's pairs and those within 1e-2 below the
    saturation point, together at most 5 % of the pairs.
    With the rendered depth maps every pair saturates (a point 0.3 ... 1.5 in front of the reference camera, re-projected from
    a depth of 2 ... 9, lands far from its pixel).  The clamped-texel outcome below 3 is met with source 3's map changed at the
    border: a member's clamped texel is given the member's own depth in source 3, 0.1 % off — as a depth map estimated by an
    earlier pass may hold anything — so that the re-projection comes back to within a pixel.
    Measured on 300 members x 2 views: 3 pairs left out, the model saturates on the other 597 and the oracle returns 3.0 on each;
    clamped texels: 48 members, all below 3 on both sides, max deviation 2.7e-04."""
    sc, o, cams, _, deps = _model_scene()
    px, planes, _ = members("C3", 1024)
    px, planes = px[:300], planes[:300]
    vf, v3 = G.view_of(G.FORWARD, S_KAT), G.view_of(G.SOURCE3, S_KAT)

    def outcomes(o, deps, px, planes, views, what):
        a, b, skipped = _geom_pairs(sc, o, cams, deps, px, planes, views)
        near = (b < 3.0) & (b > 3.0 - 1e-2)     # the model just below the saturation point: the oracle may be at it
        sat, below = (b >= 3.0) & ~near, (b < 3.0) & ~near
        print("C3 geom, %s: %d pairs (%d + %d left out), model saturated on %d, below 3 on %d; oracle: %d at 3.0; max deviation below 3: %.2e"
              % (what, len(a), skipped, int(near.sum()), int(sat.sum()), int(below.sum()), int((a == 3.0).sum()),
                 np.abs(a - b)[below].max() if below.any() else 0.0))
        assert skipped + near.sum() <= 0.05 * (len(a) + skipped)
        assert (a[sat] == 3.0).all()
        assert (np.abs(a - b)[below] < 5e-3).all()
        return int(sat.sum()), int(below.sum())
    sat, _ = outcomes(o, deps, px, planes, (vf, v3), "rendered depth maps")
    assert sat > 100
    # the clamped-texel outcome: members whose projection into source 3 leaves the image, one per border texel
    dep3 = sc["depth_gt"][v3].copy()
    taken, chosen = set(), []
    for k, ((x, y), pl) in enumerate(zip(px, planes)):
        pl64 = pl.astype(np.float64)
        sx, sy, sd = M.project_on_camera(M.point_on_world(float(x), float(y), M.depth_from_plane(cams[0], pl64, x, y), cams[0]), cams[v3])
        if not (np.isfinite(sx) and np.isfinite(sy)) or (0 <= sx < W and 0 <= sy < H) or sd <= 0 or max(abs(sx), abs(sy)) > 1e6:
            continue
        cx, cy = min(max(int(sx), 0), W - 1), min(max(int(sy), 0), H - 1)
        if (cx, cy) in taken:
            continue
        taken.add((cx, cy))
        dep3[cy, cx] = np.float32(sd * 1.001)
        chosen.append(k)
    assert len(chosen) >= 20, len(chosen)
    depths = sc["depth_gt"].copy()
    depths[v3] = dep3
    o.set_depths(depths)
    deps = [d.astype(np.float64) for d in depths]
    _, below = outcomes(o, deps, px[chosen], planes[chosen], (v3,), "source 3's border texels set, %d clamped texels" % len(chosen))
    assert below >= 20, below


def test_ncc_straddling_vs_numpy():
    """C1 at sampler 1 against the float64 model, on the members whose min|Z| / max|Z| > 0.05.  The model is ill conditioned here
    (a tap near Z = 0 moves by pixels for one binary32 rounding of H): no bound is chosen in advance; oracle == emulation == GPU
    bit for bit is what carries the class, and three times the measured p99 stands as a tripwire for a change of contract.
    Measured on the first 1500 members: 96 qualify; median 5.3e-06, p99 4.6e-05, max 5.3e-05.
    C2 has no such check: a tap at Z ~ 0 is what makes a member, so none of its members has min|Z| / max|Z| > 0.05 (the count is
    printed, not asserted) and the bitwise statements alone carry it."""
    measured_p99 = 4.6e-5
    sc, o, cams, imgs, _ = _model_scene()
    px2, planes2, view2 = members("C2")
    print("C2: %d of 4096 members have min|Z| / max|Z| > 0.05" % int((G.classify(sc, view2, px2, planes2)["cond"] > 0.05).sum()))
    px, planes, view = members("C1")
    px, planes, view = px[:1500], planes[:1500], view[:1500]
    ok = G.classify(sc, view, px, planes)["cond"] > 0.05
    print("C1: %d of %d members have min|Z| / max|Z| > 0.05" % (int(ok.sum()), len(ok)))
    assert ok.sum() >= 50
    d = _ncc_deviation(o, cams, imgs, px[ok], planes[ok], view[ok])
    print("C1 ncc_old oracle vs numpy64: median %.2e p99 %.2e max %.2e" % (np.median(d), np.quantile(d, 0.99), d.max()))
    assert np.quantile(d, 0.99) < 3 * measured_p99
