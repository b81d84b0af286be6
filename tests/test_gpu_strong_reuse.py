"""The plane cache of the split strong update (dvp_strong.hpp: strong_reuse_plan; DVP_STRONG_REUSE, on by default): a pixel keeps
the cost vectors of the planes it evaluated at its previous visit and evaluates only the planes it has not seen.  A vector is a
pure function of (pixel, plane, radius) within an epoch, so every result must stay bit-identical: with the cache on and off,
against the CPU oracle, through run_patchmatch and through run_stage, after the images or the radius map of a context change,
and when the cache's records do not fit.  Small scenes (one of odd width: half_w rounds), S = 3 / 9 / 16 (decide kernels v4 / v10 /
v16), 3 iterations, edge / label / radius priors on, FIRST_INIT followed by REFINE_ITER with geometric consistency and WEAK pixels
(RANSACToGetFitPlane rewrites their radius inside the loop)."""
import numpy as np
import pytest

from conftest import (pkg, synth, make_params, count_diff, stage_sequence, CHECKED, first_pass_state, second_pass_inputs)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ITERS = 3
CASES = [(71, 50, 3), (96, 64, 9), (71, 50, 16)]
_REF = {}


def capi():
    return pkg("capi")


def _params(S):
    p1 = make_params(S + 1, max_iterations=ITERS, state=synth.FIRST_INIT, use_APD=0)
    p2 = make_params(S + 1, max_iterations=ITERS, state=synth.REFINE_ITER, use_APD=1, geom_consistency=1,
                     weak_peak_radius=4, rotate_time=2, ransac_threshold=0.01)
    return p1, p2


def reference(W, H, S):
    """the oracle's two passes, computed once per case and shared (never modified)"""
    key = (W, H, S)
    if key not in _REF:
        sc = synth.make_scene(W, H, S)
        p1, p2 = _params(S)
        st1 = first_pass_state(sc)
        st1["radius"] = (5 + np.arange(W * H) % 3 * 5).astype(np.int32)   # radius prior: 5 / 10 / 15
        o1 = O.from_scene(sc, p1)
        o1.upload_state(**st1)
        o1.run_patchmatch()
        out1 = {n: o1.get(n).copy() for n in CHECKED}
        st2 = second_pass_inputs(o1, sc)
        o1.close()
        weak = st2["weak"].reshape(H, W).copy()
        weak[sc["flat"] & (weak == synth.STRONG)] = synth.WEAK
        st2["weak"] = weak.reshape(-1)
        o2 = O.from_scene(sc, p2, depths=sc["depth_gt"])
        o2.upload_state(**st2)
        assert o2.weak_count() > 50
        o2.run_patchmatch()
        out2 = {n: o2.get(n).copy() for n in CHECKED}
        o2.close()
        for d in (out1, out2):
            for a in d.values():
                a.setflags(write=False)
        _REF[key] = dict(sc=sc, st1=st1, st2=st2, out1=out1, out2=out2)
    return _REF[key]


def _anchors(final, W):
    nb = final["neighbours"].reshape(-1, 12, 2)[:, 1:].reshape(-1, 2)
    return np.unique(nb[nb[:, 0] >= 0].astype(np.int64) @ np.array([1, W]))


def _equal(final, eng, what, W, whole_candidates):
    """every CHECKED buffer; after run_patchmatch the candidate records at the anchor pixels only (the engine forms no others:
    DVP_CAND_MASK in conftest)"""
    for n in CHECKED:
        got = eng.get(n)
        if n == "candidate" and not whole_candidates:
            an = _anchors(final, W)
            if len(an) == 0:
                continue
            nd = count_diff(final[n].reshape(len(final["planes"]), -1)[an], got.reshape(len(final["planes"]), -1)[an])
        else:
            nd = count_diff(final[n], got)
        assert nd == 0, "%s: %s differs in %d entries" % (what, n, nd)


def _snapshot(eng):
    return {n: eng.get(n).copy() for n in CHECKED}


def _two_passes(ref, S, run):
    """FIRST_INIT, then REFINE_ITER on the SAME context (new parameters, depth maps, state: the cache must not carry over)"""
    sc = ref["sc"]
    p1, p2 = _params(S)
    g = capi().from_scene(sc, p1)
    g.upload_state(**ref["st1"])
    run(g)
    r1 = _snapshot(g)
    g.set_params(p2)
    g.set_depths(sc["depth_gt"])
    g.upload_state(**ref["st2"])
    run(g)
    r2 = _snapshot(g)
    g.close()
    return r1, r2


class _Snap:
    def __init__(self, d):
        self.d = d

    def get(self, n):
        return self.d[n]


def _by_stages(g):
    for st, it, col in stage_sequence(ITERS):
        g.run_stage(st, it, col)


@pytest.mark.parametrize("W,H,S", CASES)
def test_run_patchmatch_same_bits_with_and_without_the_cache(W, H, S, monkeypatch):
    ref = reference(W, H, S)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DVP_STRONG_REUSE", mode)
        res[mode] = _two_passes(ref, S, lambda g: g.run_patchmatch())
    for k, out in ((0, ref["out1"]), (1, ref["out2"])):
        for n in CHECKED:
            nd = count_diff(res["1"][k][n], res["0"][k][n])
            assert nd == 0, "pass %d: %s differs in %d entries between DVP_STRONG_REUSE=0 and the default" % (k + 1, n, nd)
        _equal(out, _Snap(res["1"][k]), "pass %d against the oracle" % (k + 1), W, whole_candidates=False)


@pytest.mark.parametrize("W,H,S", CASES)
def test_run_stage_same_bits_with_and_without_the_cache(W, H, S, monkeypatch):
    ref = reference(W, H, S)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DVP_STRONG_REUSE", mode)
        res[mode] = _two_passes(ref, S, _by_stages)
    for k, out in ((0, ref["out1"]), (1, ref["out2"])):
        for n in CHECKED:
            nd = count_diff(res["1"][k][n], res["0"][k][n])
            assert nd == 0, "pass %d: %s differs in %d entries between DVP_STRONG_REUSE=0 and the default" % (k + 1, n, nd)
        _equal(out, _Snap(res["1"][k]), "pass %d by stages against the oracle" % (k + 1), W, whole_candidates=True)


def _refine_pass(sc, st, S):
    _, p2 = _params(S)
    g = capi().from_scene(sc, p2, depths=sc["depth_gt"])
    g.upload_state(**st)
    return g


def test_new_images_and_a_new_radius_map_empty_the_cache():
    """a context that has run a pass gets other images (same size), the same state, and runs again: the result must be a fresh
    context's on the second inputs, and likewise after the radius map alone changes"""
    W, H, S = 71, 50, 3
    ref = reference(W, H, S)
    sc, st = ref["sc"], ref["st2"]
    g = _refine_pass(sc, st, S)
    g.run_patchmatch()
    # 1. other images
    sc_b = dict(sc)
    sc_b["images"] = np.ascontiguousarray(np.asarray(sc["images"])[:, ::-1, ::-1])   # every view upside down: other texels at every pixel
    assert count_diff(np.asarray(sc_b["images"]), np.asarray(sc["images"])) > W * H
    g.set_images(sc_b["images"])
    g.upload_state(**st)
    g.run_patchmatch()
    fresh = _refine_pass(sc_b, st, S)
    fresh.run_patchmatch()
    want = _snapshot(fresh)
    fresh.close()
    assert count_diff(want["planes"], ref["out2"]["planes"]) > 0   # the second inputs do give another result
    _equal(want, g, "after set_images", W, whole_candidates=False)
    # 2. another radius map
    st_r = dict(st)
    st_r["radius"] = np.where(st["radius"] == 5, 10, 5).astype(np.int32)
    g.upload_state(**st_r)
    g.run_patchmatch()
    fresh = _refine_pass(sc_b, st_r, S)
    fresh.run_patchmatch()
    want_r = _snapshot(fresh)
    fresh.close()
    assert count_diff(want_r["planes"], want["planes"]) > 0
    _equal(want_r, g, "after a new radius map", W, whole_candidates=False)
    g.close()


def _strong_evals_by_launch(sc, st, S):
    g = _refine_pass(sc, st, S)
    g.set_profiling(True)
    g.timings(reset=True)
    per = []
    for stg, it, col in stage_sequence(ITERS):
        g.run_stage(stg, it, col)
        if stg == "strong_update":
            per.append(int(g.timings(reset=True)["ncc_evals"]["strong_update"]))
    out = _snapshot(g)
    g.close()
    return per, out


def test_the_cache_is_live(monkeypatch):
    """REFINE_ITER pass: the strong update evaluates strictly less with the cache; every first visit misses, so iteration 0
    (its black and its red launch) evaluates exactly what it did"""
    W, H, S = 96, 64, 9
    ref = reference(W, H, S)
    monkeypatch.setenv("DVP_STRONG_REUSE", "0")
    off, out_off = _strong_evals_by_launch(ref["sc"], ref["st2"], S)
    monkeypatch.setenv("DVP_STRONG_REUSE", "1")
    on, out_on = _strong_evals_by_launch(ref["sc"], ref["st2"], S)
    print("strong update evaluations per launch: cache off %s, on %s" % (off, on))
    assert len(on) == len(off) == 2 * ITERS
    assert on[:2] == off[:2] and min(off[:2]) > 0
    assert sum(on) < sum(off)
    assert all(a <= b for a, b in zip(on, off))
    for n in CHECKED:
        assert count_diff(out_on[n], out_off[n]) == 0, n


def test_falls_back_when_the_records_do_not_fit(monkeypatch):
    """DVP_TEST_REUSE_ALLOC_FAIL makes the records' allocation report failure: the context carries on with the per-launch buffer"""
    W, H, S = 96, 64, 9
    ref = reference(W, H, S)
    monkeypatch.setenv("DVP_TEST_REUSE_ALLOC_FAIL", "1")
    r1, r2 = _two_passes(ref, S, lambda g: g.run_patchmatch())
    _equal(ref["out1"], _Snap(r1), "pass 1, no room for the cache", W, whole_candidates=False)
    _equal(ref["out2"], _Snap(r2), "pass 2, no room for the cache", W, whole_candidates=False)
    # ... and really did: no evaluation saved
    g = _refine_pass(ref["sc"], ref["st2"], S)
    g.set_profiling(True)
    g.timings(reset=True)
    g.run_patchmatch()
    with_hook = int(g.timings()["ncc_evals"]["strong_update"])
    g.close()
    monkeypatch.delenv("DVP_TEST_REUSE_ALLOC_FAIL")
    monkeypatch.setenv("DVP_STRONG_REUSE", "0")
    g = _refine_pass(ref["sc"], ref["st2"], S)
    g.set_profiling(True)
    g.timings(reset=True)
    g.run_patchmatch()
    assert with_hook == int(g.timings()["ncc_evals"]["strong_update"])
    g.close()
