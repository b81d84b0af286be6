"""Every source-view count S = num_images - 1 the reference's driver can hand the engine (1 ... 20 from pair.txt, and the
C ABI's maximum of 31), and the kernel forms each count selects, against the oracle bit for bit after every launch.

Most launch sites pick their kernel by S: the split strong update's decision kernel (dvp_strong_decide_v4 / 6 / 8 / 10 / 12
/ 16), the monolithic strong update (_v8 / _v16 / generic for S > 16), the visibility-prior candidates (ceil(S / 5) lanes
per pixel), the one-wave weak update (seven views per batch of its prefetch table).  Each case is a FIRST_INIT pass and a
REFINE_ITER pass with geometric consistency, WEAK pixels, edge / label priors and adaptive radii; it asserts that the
selected-view masks really grew to the counts under test, so that a case cannot pass on masks of one or two views.
CPU: host emulation of the kernels; GPU (-m gpu): the HIP library through the C ABI."""
import functools

import numpy as np
import pytest

from conftest import pkg, synth, make_params, count_diff, stage_sequence, CHECKED, first_pass_state, second_pass_inputs
from oracle import oracle as O
from tests.emul import emul as E
from test_edge_cases import scene_with_views, image_set, image_env

W, H = 88, 64
SEED = 4321
SWEEP = list(range(1, 21)) + [31]
BOUNDARY = [4, 5, 6, 7, 8, 10, 11, 12, 13, 16, 17, 20]
# (form, environment before the context is created); "default" is the split strong update with (pixel, slot) evaluation
# items and lane-wise refinement, and the phased weak update (conftest: DVP_WEAK_PHASED_MIN=0)
FORMS = {
    "default": {},
    "strong_split_lockstep_refine": dict(DVP_STRONG_SPLIT="1", DVP_REFINE_LANES="0", DVP_EVAL_ITEMS="0"),
    "strong_monolithic": dict(DVP_STRONG_SPLIT="0"),
    "weak_one_wave": dict(DVP_WEAK_PHASED="0"),
}
SWEEP_FORMS = {"sweep_split": dict(DVP_SWEEP_SPLIT="2"), "sweep_fused": dict(DVP_SWEEP_SPLIT="0")}
# the image-format axis (test_edge_cases.IMAGE_SETS): binary16 tiles at the counts around the one-wave update's batches of seven
# views (kWeakViews), the float planes of the same images at a few
HALF_SWEEP = [1, 2, 7, 8, 9, 14, 15, 20, 31]
FLOAT_SWEEP = [1, 8, 15, 31]


def cases():
    out = [(S, "default") for S in SWEEP]
    for S in BOUNDARY:
        out += [(S, f) for f in list(FORMS)[1:] + list(SWEEP_FORMS)]
    return sorted(out, key=lambda c: c[0])   # same S next to each other: the oracle's run is cached per S


def format_cases():
    out = [(S, f, "box") for S in HALF_SWEEP for f in ("default", "weak_one_wave")]
    out += [(S, "default", "box_no16") for S in FLOAT_SWEEP]
    return sorted(out, key=lambda c: c[0])   # "box" and "box_no16" share the oracle's run


def popcount(a):
    a = np.asarray(a, np.uint32)
    return np.unpackbits(a.view(np.uint8).reshape(-1, 4), axis=1).sum(1)


def make_scene(S):
    return synth.make_scene(W, H, S) if S <= len(synth._RING) else scene_with_views(W, H, S)


def pass_params(S):
    p1 = make_params(S + 1, max_iterations=1, state=synth.FIRST_INIT, use_APD=0)
    p2 = make_params(S + 1, max_iterations=1, state=synth.REFINE_ITER, use_APD=1, geom_consistency=1,
                     weak_peak_radius=4, rotate_time=2, ransac_threshold=0.01)
    return p1, p2


def second_state(o1, sc):
    """pass 2's input from pass 1's result (as many_views_case in test_emul_parity): the low-texture window and a block
    of the textured part become WEAK"""
    st = second_pass_inputs(o1, sc)
    weak = st["weak"].reshape(H, W)
    weak[sc["flat"] & (weak == synth.STRONG)] = synth.WEAK
    weak[20:30, 40:60] = np.where(weak[20:30, 40:60] == synth.STRONG, synth.WEAK, weak[20:30, 40:60])
    st["weak"] = weak.reshape(-1)
    return st


def compare_run_patchmatch(final, b, what):
    """after run_patchmatch: every CHECKED buffer; the candidate records at the anchor pixels only — the engine forms them
    there and nowhere else (dvp_anchor_mask, DVP_CAND_MASK in conftest), the weak update reads no others"""
    for n in CHECKED:
        if n == "candidate":
            continue
        nd = count_diff(final[n], b.get(n))
        assert nd == 0, "%s: %s differs in %d entries after run_patchmatch" % (what, n, nd)
    nb = final["neighbours"].reshape(-1, 12, 2)[:, 1:].reshape(-1, 2)
    anchors = np.unique(nb[nb[:, 0] >= 0].astype(np.int64) @ np.array([1, W]))
    assert len(anchors) > 100, (what, len(anchors))
    ca, cb = (x.reshape(W * H, -1)[anchors] for x in (final["candidate"], b.get("candidate")))
    nd = count_diff(ca, cb)
    assert nd == 0, "%s: candidate records differ at %d entries of the %d anchor pixels after run_patchmatch" % (what, nd, len(anchors))


def run_stages(eng, iters, record):
    """stage_sequence(iters) on `eng`; record(stage, it, colour, eng) after every launch, and the masks of the WEAK pixels
    as they enter the weak update"""
    weak_in = []
    for st, it, col in stage_sequence(iters):
        if st == "weak_update":
            w = eng.get("weak_info") == synth.WEAK
            weak_in.append(eng.get("selected_views")[w].copy())
        eng.run_stage(st, it, col)
        record(st, it, col, eng)
    return weak_in


class Trace:
    """CHECKED after every stage; a buffer whose bits did not change keeps the previous array (the S = 31 candidate
    buffer alone is 5.6 MB)"""
    def __init__(self):
        self.steps = []

    def __call__(self, st, it, col, eng):
        prev = self.steps[-1][1] if self.steps else {}
        snap = {}
        for n in CHECKED:
            a = eng.get(n)
            snap[n] = prev[n] if n in prev and count_diff(prev[n], a) == 0 else a.copy()
        self.steps.append(((st, it, col), snap))


@functools.lru_cache(maxsize=1)
def oracle_run(S, images="int"):
    """The oracle's two passes at S on image set `images`, stage by stage; and pass 2 again in one run_patchmatch (the sweep
    forms)."""
    sc = make_scene(S)
    if images != "int":
        sc, _ = image_set(sc, images)
    p1, p2 = pass_params(S)
    o1 = O.from_scene(sc, p1, seed=SEED)
    o1.upload_state(**first_pass_state(sc))
    t1 = Trace()
    run_stages(o1, 1, t1)
    st = second_state(o1, sc)
    o1.close()
    o2 = O.from_scene(sc, p2, seed=SEED, depths=sc["depth_gt"])
    o2.upload_state(**st)
    assert o2.weak_count() > 50
    t2 = Trace()
    weak_in = run_stages(o2, 1, t2)
    o2.close()
    o3 = O.from_scene(sc, p2, seed=SEED, depths=sc["depth_gt"])
    o3.upload_state(**st)
    o3.run_patchmatch()
    final = {n: o3.get(n).copy() for n in CHECKED}
    o3.close()
    return sc, st, t1.steps, t2.steps, weak_in, final


def check_masks_are_large(S, steps, weak_in):
    """not vacuous: the view selection reached the counts whose kernels are under test (per pixel, the largest mask
    after any launch of the two passes)"""
    counts = np.max([popcount(snap["selected_views"]) for _, snap in steps], axis=0)
    # 15 draws against the CDF rarely collect all 12 of 12 views (3 pixels here): at S = 12, 11 views on 10 pixels and
    # all 12 on one
    want = min(S, 11 if S == 12 else 12)
    reached = int((counts >= want).sum())
    assert counts.max() >= min(S, 12), (S, counts.max())
    weak_most = max(int(popcount(m).max()) if len(m) else 0 for m in weak_in)
    print("S=%d: largest selected-view count %d (%d pixels >= %d); WEAK pixels enter the weak update with up to %d views"
          % (S, counts.max(), reached, want, weak_most))
    assert reached >= 10, (S, reached, want)
    assert counts.max() <= 15     # the view selection draws 15 times (APD.cu:2508, 2828)
    if S >= 8:
        assert weak_most >= 8, (S, weak_most)


def view_count_case(S, form, make_engine, monkeypatch, images=None):
    for k, v in dict(FORMS, **SWEEP_FORMS)[form].items():
        monkeypatch.setenv(k, v)
    fmt = None
    if images is None:
        sc, st, steps1, steps2, weak_in, final = oracle_run(S)
    else:
        sc, st, steps1, steps2, weak_in, final = oracle_run(S, "box" if images == "box_no16" else images)
        fmt = image_env(images, monkeypatch)
    check_masks_are_large(S, steps1 + steps2, weak_in)
    p1, p2 = pass_params(S)
    if form in SWEEP_FORMS:   # DepthToWeak + LocalRefine are one launch site of run_patchmatch only
        b = make_engine(sc, p2, sc["depth_gt"])
        b.upload_state(**st)
        b.run_patchmatch()
        compare_run_patchmatch(final, b, "S=%d %s" % (S, form))
        return
    for p, state, steps, dep in ((p1, first_pass_state(sc), steps1, None), (p2, st, steps2, sc["depth_gt"])):
        b = make_engine(sc, p, dep)
        if fmt is not None:
            assert b.image_format() == fmt, (S, form, images)
        b.upload_state(**state)
        ref = iter(steps)

        def compare(stg, it, col, eng):
            key, snap = next(ref)
            assert key == (stg, it, col)
            for n in CHECKED:
                nd = count_diff(snap[n], eng.get(n))
                assert nd == 0, "S=%d %s, state %d: %s differs in %d entries after %s(it=%d, colour=%d)" % (
                    S, form, int(p["state"]), n, nd, stg, it, col)
        run_stages(b, 1, compare)
    assert (steps2[-1][1]["weak_reliable"] == 1).sum() > 0


def emul_engine(sc, p, depths):
    return O.from_scene(sc, p, seed=SEED, depths=depths, cls=E.Emul)


def gpu_engine(sc, p, depths):
    return pkg("capi").from_scene(sc, p, seed=SEED, depths=depths)


@pytest.mark.parametrize("S,form", cases(), ids=lambda v: str(v))
def test_view_counts_emulated_kernels(S, form, monkeypatch):
    view_count_case(S, form, emul_engine, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("S,form", cases(), ids=lambda v: str(v))
def test_view_counts_gpu(S, form, monkeypatch):
    view_count_case(S, form, gpu_engine, monkeypatch)


@pytest.mark.parametrize("S,form,images", format_cases(), ids=lambda v: str(v))
def test_view_counts_image_formats_emulated_kernels(S, form, images, monkeypatch):
    view_count_case(S, form, emul_engine, monkeypatch, images)


@pytest.mark.gpu
@pytest.mark.parametrize("S,form,images", format_cases(), ids=lambda v: str(v))
def test_view_counts_image_formats_gpu(S, form, images, monkeypatch):
    view_count_case(S, form, gpu_engine, monkeypatch, images)


def full_masks_case(S, make_engine):
    """REFINE_INIT from uploaded masks with all S bits on a third of the pixels (legal input at any popcount): the
    reference keeps 20 view directions in GenerateRandomNormal_YZL (APD.cu:511, view_direction[20]; the oracle's
    `if (index < 20)`), every launch site that reads the mask must still agree with the oracle"""
    sc, st, steps1, _, _, _ = oracle_run(S)
    st = dict(st)
    views = st["views"].copy()
    full = np.arange(W * H) % 3 == 0
    views[full] = np.uint32((1 << S) - 1)
    st["views"] = views
    p = make_params(S + 1, max_iterations=1, state=synth.REFINE_INIT, use_APD=1, weak_peak_radius=6)
    a = O.from_scene(sc, p, seed=SEED)
    b = make_engine(sc, p, None)
    a.upload_state(**st)
    b.upload_state(**st)
    for stg, it, col in stage_sequence(1):
        a.run_stage(stg, it, col)
        b.run_stage(stg, it, col)
        for n in CHECKED:
            nd = count_diff(a.get(n), b.get(n))
            assert nd == 0, "S=%d full masks: %s differs in %d entries after %s(it=%d, colour=%d)" % (S, n, nd, stg, it, col)
        if stg == "random_init":   # the uploaded masks survive RandomInitialization's pruning on some pixels
            kept = int((popcount(a.get("selected_views")) == S).sum())
            print("S=%d: %d pixels keep all %d views after random_init" % (S, kept, S))
            assert kept >= 100


@pytest.mark.parametrize("S", [20, 31])
def test_refine_init_full_masks_emulated_kernels(S):
    full_masks_case(S, emul_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [20, 31])
def test_refine_init_full_masks_gpu(S):
    full_masks_case(S, gpu_engine)


# Patch geometries the parameters allow, each through a FIRST_INIT and a REFINE_ITER pass at S = 6: GenEdgeInform's sector
# table for a weak_radius other than 5 (dvp_set_params: make_sector_taps) and the per-view candidate kernels it selects
# (dvp_gen_candidates[_list]); fixed strong patches (use_radius = 0) where the 6-tap NCC table does not apply (r 3, inc 1)
# and where it applies with taps that are not symmetric about the pixel (r 8, inc 3: -8 ... 7); and a radius map with
# every adaptive radius from 5 to 15 (inc = max(2, int(2r / 5)): the 6-tap table at r 5, 8, 10, 11, 13, 14, 15).
GEOMETRIES = {
    "weak_radius_3": dict(weak_radius=3),
    "weak_radius_8": dict(weak_radius=8),
    "fixed_r3_inc1": dict(use_radius=0, strong_radius=3, strong_increment=1),
    "fixed_r8_inc3": dict(use_radius=0, strong_radius=8, strong_increment=3),
    "radius_map_5_to_15": dict(use_radius=1),
}


def geometry_case(name, make_engine, images=None, monkeypatch=None):
    S = 6
    over = GEOMETRIES[name]
    sc = synth.make_scene(W, H, S)
    fmt = None
    if images is not None:
        sc, fmt = image_set(sc, images, monkeypatch)
    p1 = make_params(S + 1, max_iterations=1, state=synth.FIRST_INIT, use_APD=0, **over)
    p2 = make_params(S + 1, max_iterations=1, state=synth.REFINE_ITER, use_APD=1, geom_consistency=1,
                     weak_peak_radius=4, rotate_time=2, ransac_threshold=0.01, **over)
    st1 = first_pass_state(sc)
    o1 = O.from_scene(sc, p1, seed=SEED)
    o1.upload_state(**st1)
    o1.run_patchmatch()
    st2 = second_state(o1, sc)
    o1.close()
    if name == "radius_map_5_to_15":
        st2["radius"] = (5 + np.arange(W * H) % 11).astype(np.int32)
    for p, st, dep in ((p1, st1, None), (p2, st2, sc["depth_gt"])):
        a = O.from_scene(sc, p, seed=SEED, depths=dep)
        b = make_engine(sc, p, dep)
        if fmt is not None:
            assert b.image_format() == fmt, (name, images)
        a.upload_state(**st)
        b.upload_state(**st)
        for stg, it, col in stage_sequence(1):
            a.run_stage(stg, it, col)
            b.run_stage(stg, it, col)
            for n in CHECKED:
                nd = count_diff(a.get(n), b.get(n))
                assert nd == 0, "%s, state %d: %s differs in %d entries after %s(it=%d, colour=%d)" % (
                    name, int(p["state"]), n, nd, stg, it, col)
            if stg == "gen_edge_inform" and int(p["state"]) == synth.REFINE_ITER:
                cand = a.get("candidate").reshape(W * H, S, 8, 2)
                weak = a.get("weak_info") == synth.WEAK
                found = int((cand[weak][..., 0] >= 0).sum())   # visibility-prior offsets of the WEAK pixels
                assert found > 1000, (name, found)
        assert a.weak_count() > 50 or int(p["state"]) == synth.FIRST_INIT
    # pass 2 again as one run_patchmatch: the candidate records at anchor pixels only (DVP_CAND_MASK, conftest), from the
    # list kernels (dvp_gen_candidates_list for weak_radius != 5)
    a = O.from_scene(sc, p2, seed=SEED, depths=sc["depth_gt"])
    b = make_engine(sc, p2, sc["depth_gt"])
    for x in (a, b):
        x.upload_state(**st2)
        x.run_patchmatch()
    compare_run_patchmatch({n: a.get(n) for n in CHECKED}, b, name)
    if name == "radius_map_5_to_15":
        assert set(np.unique(st2["radius"][st2["weak"] == synth.STRONG])) == set(range(5, 16))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_patch_geometries_emulated_kernels(name):
    geometry_case(name, emul_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_patch_geometries_gpu(name):
    geometry_case(name, gpu_engine)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_patch_geometries_half_planes_emulated_kernels(name, monkeypatch):
    geometry_case(name, emul_engine, "box", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_patch_geometries_half_planes_gpu(name, monkeypatch):
    geometry_case(name, gpu_engine, "box", monkeypatch)
