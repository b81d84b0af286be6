"""The oracle pinned to the reference's own device text.

oracle/make_ref.py cuts everything in front of APD::RunPatchMatch out of the reference's APD.cu (the device functions and
the 16 kernels), compiles it unchanged for the host against the stand-in headers of oracle/ref_shim/ and wraps it in
oracle/ref_harness.cpp.  The claim tested here: that text, run thread by thread over the launch geometry, equals the
oracle in LITERAL mode (Oracle.set_numerics(1)) bit for bit — integer buffers exactly, float buffers bitwise with
NaN == NaN, on all pixels, launch site by launch site, each launch started from the oracle's state.  The engine is bit-exact
against the oracle's CONTRACT numerics; the distance from there to the reference text is measured per launch site and gated.

What can differ in principle between the two builds and does not: both are g++ -ffp-contract=off -fno-fast-math, libm for
expf / exp / atan2 in both; no float buffer needs a tolerance (measured maximum: 0 ulp at every site and shape below).

Deliberate, documented departures of the oracle (DESIGN.md §2, quirk ledger) are encoded as explicit expected differences:
  * APD.cu:3783 reads regions[r][0] of an EMPTY 30-degree sector uninitialised; the oracle defines it as offset (0, 0) with
    weight 0.  A candidate record (pixel, view) is compared where all 12 sectors have a member (restated here from the
    pre-launch selected views) and is exempt elsewhere.
  * APD.cu:4257 never assigns use_a/b/c_index, so APD.cu:4349-4351 read strong_points[-1] three times: whatever is there,
    A == B == C, the triangle has no area and the launch writes radius 0 (asserted here).  The oracle defines the triangle
    as the one that produced best_plane.  Exempt: `radius` after ransac_fit at WEAK pixels that got a fitted plane.
  * candidate_cuda has the reference's stride of 4 views (main.h:41) and aliases above: every scene here has S <= 4.
  * use_edge = 0 (legacy sampling, APD.cu:2142-2460) is not implemented in the oracle: no scene here turns it off.
What this does NOT pin: nvcc's --use_fast_math lowering, the hardware texture unit's last bits, cuRAND's stream (the draws
are the oracle's counter-based ones, keyed by source line: oracle/ref_draws.json) and APD.cpp's host side."""
import json
import os

import numpy as np
import pytest

import ref_pin as P
from ref_pin import O, R
from conftest import synth, make_params, count_diff, stage_sequence, CHECKED, first_pass_state

pytestmark = pytest.mark.hostbox   # no GPU needed; joins the `-m gpu` run on a GPU box (conftest.py)

_REASON = R.unavailable_reason()
needs_ref = pytest.mark.skipif(_REASON is not None, reason=_REASON or "")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INTS = [n for n in CHECKED if n not in P.FLOATS]

# (W, H, S, sampler, weak_peak_radius): odd height and narrower than two waves with one source; three sources; four (the
# reference's candidate stride), odd width, the long peak search
SHAPES = [(70, 33, 1, 1, 4), (64, 48, 3, 0, 4), (71, 50, 4, 0, 40), (64, 48, 3, 1, 40)]
SITES = [(ps, i) + s for ps in (1, 2) for i, s in enumerate(stage_sequence(P.ITERS))]
_WALKS = {}


class _Contract:
    """an oracle context that runs its launches in contract numerics while the process-wide switch is literal"""

    def __init__(self, o, main):
        self.o, self.main = o, main

    def __getattr__(self, name):
        return getattr(self.o, name)

    def run_stage(self, st, it, col):
        self.o.set_numerics(0)
        try:
            self.o.run_stage(st, it, col)
        finally:
            self.main.set_numerics(1)


def compared_rows(st, pre, ora, W, H, S, params):
    """{buffer: bool mask of the rows that are compared after this launch}: the departures of the module docstring"""
    L = W * H
    rows = {}
    if st == "gen_edge_inform":
        rows["candidate"] = P.full_sector_rows(pre["selected_views"], W, H, S, int(params["weak_radius"][0])).reshape(-1)
    if st == "ransac_fit" and params["use_radius"][0]:
        nb = pre["neighbours"].reshape(-1, 12, 2)[pre["neighbours_map"]][:, 1:, :]
        anchors = ((nb[:, :, 0] != -1) & (nb[:, :, 1] != -1)).sum(axis=1)
        rows["radius"] = ~((pre["weak_info"] == synth.WEAK) & (anchors >= 3) & (ora["fit_planes"] != 0).any(axis=1))
    return rows


def compare_launch(st, pre, ref, ora, W, H, S, params):
    """{buffer: (differing entries, exempt rows)} with the departures of the module docstring applied"""
    res = {}
    rows = compared_rows(st, pre, ora, W, H, S, params)
    for n in CHECKED:
        a, b = ref[n], ora[n]
        exempt = 0
        if n in rows:
            keep = rows[n]
            a, b = a.reshape(len(keep), -1), b.reshape(len(keep), -1)
            if n == "radius":
                assert (a[~keep] == 0).all(), "the reference's degenerate triangle (APD.cu:4349-4357) must give radius 0"
            a, b, exempt = a[keep], b[keep], int((~keep).sum())
        res[n] = (count_diff(a, b), exempt)
    return res


def contract_distance(st, pre, ref, con, W, H, S, params):
    """share of pixels whose integer outputs differ (the exempt rows of compared_rows left out); of pixels whose plane offset /
    cost moved by more than 1e-3 relative; the mean relative movement of each"""
    L = W * H
    keep = compared_rows(st, pre, con, W, H, S, params)
    rows = np.zeros(L, bool)
    for n in INTS:
        if n in P.WEAK_IDX:
            continue
        d = ref[n].reshape(L, -1) != con[n].reshape(L, -1)
        if n in keep:
            d &= np.repeat(keep[n].reshape(L, -1), d.shape[1] // (len(keep[n]) // L), axis=1)
        rows |= d.any(axis=1)
    out = dict(int_share=float(rows.mean()))
    for key, a, b in (("w", ref["planes"][:, 3], con["planes"][:, 3]), ("cost", ref["costs"], con["costs"])):
        a, b = a.astype(np.float64), b.astype(np.float64)
        ok = np.isfinite(a) & np.isfinite(b) & (a != 0)
        rel = np.abs(a[ok] - b[ok]) / np.abs(a[ok]) if ok.any() else np.zeros(1)
        out[key + "_over_1e3"] = float((rel > 1e-3).mean())
        out[key + "_mean"] = float(rel.mean())
    return out


def run_pass(sc, params, state, depths, sampler, seed=1234, debug=False, contract=True):
    """one pass, launch by launch: [(stage, it, colour, literal comparison, contract distance, ownership violations)]; the
    literal oracle is returned for the hand-over"""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    o = O.from_scene(sc, params, seed=seed, sampler=sampler, depths=depths)
    o.set_numerics(1)
    o.upload_state(**state)
    r = R.from_scene(sc, params, seed=seed, sampler=sampler, depths=depths)
    r.set_debug(debug)
    engines = dict(ref=r)
    if contract:
        engines["contract"] = _Contract(O.from_scene(sc, params, seed=seed, sampler=sampler, depths=depths), o)
    recs = []
    for st, it, col, pre, post in P.walk(o, engines):
        lit = compare_launch(st, pre, post["ref"], post["oracle"], W, H, S, o.params)
        dist = contract_distance(st, pre, post["ref"], post["contract"], W, H, S, o.params) if contract else None
        recs.append((st, it, col, lit, dist, r.violation() if debug else None))
    r.close()
    if contract:
        engines["contract"].o.close()
    return recs, o


def two_passes(shape, debug=False, contract=True):
    W, H, S, sampler, wpr = shape
    sc = synth.make_scene(W, H, S)
    p1, p2 = P.pass_params(S, wpr)
    try:
        recs1, o1 = run_pass(sc, p1, P.first_state(sc), None, sampler, debug=debug, contract=contract)
        st2 = P.second_state(o1, sc)
        o1.close()
        assert (st2["weak"] == synth.WEAK).sum() > 50
        recs2, o2 = run_pass(sc, p2, st2, sc["depth_gt"], sampler, debug=debug, contract=contract)
        o2.close()
    finally:
        _back_to_contract()
    return {1: recs1, 2: recs2}


def _back_to_contract():
    tmp = O.Oracle(8, 8, 2)
    tmp.set_numerics(0)      # the literal switch is process-wide
    tmp.close()


def walked(shape):
    """both passes of a shape, computed once and shared by its launch-site cases"""
    if shape not in _WALKS:
        _WALKS[shape] = two_passes(shape)
    return _WALKS[shape]


def _site_id(s):
    return "pass%d-%02d-%s-it%d-c%d" % s


def _shape_id(s):
    return "%dx%d-S%d-sampler%d-peak%d" % s


def _distance_key(shape, site):
    return _shape_id(shape) + "/" + _site_id(site)


@needs_ref
@pytest.mark.parametrize("site", SITES, ids=_site_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
def test_launch_site_equals_the_oracle_literal_mode(shape, site):
    """FIRST_INIT then REFINE_ITER (geometric consistency, > 50 WEAK pixels, priors, radius prior 5 / 10 / 15): after this
    launch, from the oracle's pre-launch state, every CHECKED buffer of the reference text is the literal oracle's."""
    ps, idx, st, it, col = site
    rec = walked(shape)[ps][idx]
    assert rec[:3] == (st, it, col)
    for n, (nd, exempt) in rec[3].items():
        assert nd == 0, "%s differs in %d entries after %s(it=%d, colour=%d) of pass %d (%d exempt)" % (n, nd, st, it, col, ps, exempt)
    if st == "gen_edge_inform" and ps == 2:
        L, S = shape[0] * shape[1], shape[2]
        assert rec[3]["candidate"][1] < 0.5 * L * S      # the second pass has selected views: most records are compared


@needs_ref
@pytest.mark.parametrize("site", SITES, ids=_site_id)
@pytest.mark.parametrize("shape", SHAPES[1:3], ids=_shape_id)
def test_launch_site_contract_distance(shape, site):
    """The same launch with the oracle in its default (contract) numerics, which is what the engine computes bit for bit:
    share of pixels whose integer outputs differ from the reference text, share of pixels whose plane offset / cost moved
    by more than 1e-3 relative, mean relative movement.  Gated at twice the recorded measurement
    (tests/golden/reference_contract_distance.json, written by tests/golden/make_reference_golden.py)."""
    ps, idx, st, it, col = site
    dist = walked(shape)[ps][idx][4]
    print("\n%s %s: %s" % (_shape_id(shape), _site_id(site), {k: "%.3g" % v for k, v in dist.items()}))
    with open(os.path.join(GOLDEN, "reference_contract_distance.json")) as f:
        recorded = json.load(f)["sites"][_distance_key(shape, site)]
    for k, v in dist.items():
        assert v <= 2 * recorded[k], (k, v, recorded[k])


@needs_ref
def test_every_thread_writes_its_own_rows_only():
    """The premise of the launch emulation: a launch is the per-pixel function of the pre-launch state.  With the harness's
    debug switch the whole state (guard bands included) is compared with the snapshot after every thread; on a tiny two-pass
    scene no thread of any launch site writes outside the rows its pixel owns."""
    for ps, recs in two_passes((40, 33, 2, 0, 4), debug=True, contract=False).items():
        assert len(recs) == len(stage_sequence(P.ITERS))
        for st, it, col, lit, _, viol in recs:
            assert viol[0] == 0, "pass %d %s(it=%d, colour=%d): %d threads wrote outside their rows, first pixel %d in %s" % ((ps, st, it, col) + viol)
            assert all(nd == 0 for nd, _ in lit.values()), (ps, st, it, col, lit)


def _edge_case(name):
    import test_edge_cases as T
    case = [c for c in T.cases() if c[0] == name][0]
    _, W, H, S, over, mutate = case
    sc = T.scene_with_views(W, H, S)
    sc["images"] = sc["images"].copy()
    p = make_params(S + 1, **dict(dict(state=synth.FIRST_INIT, use_APD=0), **over))
    st = first_pass_state(sc)
    mutate(sc, st, p)
    return sc, p, st


@needs_ref
@pytest.mark.parametrize("name", ["all_pixels_weak", "all_pixels_unknown"])
def test_degenerate_states_equal_the_oracle_literal_mode(name):
    """a pass whose pixels are all WEAK (no STRONG anchor anywhere) or all UNKNOWN, every launch site"""
    sc, p, st = _edge_case(name)
    try:
        recs, o = run_pass(sc, p, st, None, 0, seed=99, contract=False)
        o.close()
    finally:
        _back_to_contract()
    assert len(recs) == len(stage_sequence(P.ITERS))
    for stg, it, col, lit, _, _ in recs:
        for n, (nd, exempt) in lit.items():
            assert nd == 0, "%s: %s differs in %d entries after %s(it=%d, colour=%d)" % (name, n, nd, stg, it, col)


# ---- function-level pins (no state, no draws) -------------------------------------------------------------------------
def kat_pair(sampler):
    """(oracle, reference) holding the KAT scene after gen_edge_inform .. random_init of the oracle (contract numerics)"""
    W, H, S, sc, p, st = P.kat_scene()
    o = O.from_scene(sc, p, sampler=sampler, depths=sc["depth_gt"])
    o.upload_state(**st)
    for stg, it, col in stage_sequence(0)[:5]:
        o.run_stage(stg, it, col)
    r = R.from_scene(sc, p, sampler=sampler, depths=sc["depth_gt"])
    P.load_state(r, {n: o.get(n) for n in O.BUFFERS}, st["weak"])
    return W, H, S, sc, o, r


@needs_ref
@pytest.mark.parametrize("sampler", [0, 1])
def test_cost_functions_equal_the_oracle_literal_mode(sampler):
    """ComputeHomography, ComputeCorrespondingPoint, ComputeBilateralNCCOld at radius 5 / 10 /
    15, the multi-view cost vector, ComputeBilateralNCCNew at WEAK pixels and ComputeGeomConsistencyCost: bitwise."""
    W, H, S, sc, o, r = kat_pair(sampler)
    px, planes = P.kat_inputs(W, H, sc, 4096)
    try:
        o.set_numerics(1)
        cr, co = r.eval_cost_vectors(px, planes), o.eval_cost_vectors(px, planes)
        assert count_diff(cr, co) == 0
        assert (cr < 2.0).mean() > 0.3 and (cr == 2.0).mean() > 0.05      # real patches, and planes that project outside
        cams = sc["cameras"]
        for k in range(200):
            v = 1 + k % S
            hr = r.homography(cams[0], cams[v], planes[k])
            ho = np.empty(9, np.float32)
            O.lib().ora_homography(O._p(np.ascontiguousarray(cams[0:1])), O._p(np.ascontiguousarray(cams[v:v + 1])), O._p(planes[k]), O._p(ho))
            assert count_diff(hr, ho) == 0
            # ComputeCorrespondingPoint (APD.cu:741-748) as written: binary32, sums left to right, two true divisions
            f, x, y = np.float32, np.float32(px[k, 0]), np.float32(px[k, 1])
            row = lambda i: f(f(f(hr[i] * x) + f(hr[i + 1] * y)) + hr[i + 2])
            with np.errstate(all="ignore"):
                want = np.array([row(0) / row(6), row(3) / row(6)], np.float32)
            assert count_diff(r.corresponding_point(hr, int(px[k, 0]), int(px[k, 1])), want) == 0
        weak = np.flatnonzero(o.get("weak_info") == synth.WEAK)
        assert len(weak) > 200
        rng = np.random.default_rng(3)
        gt = o.get("planes")
        n_new = n_geom = 0
        for c in rng.choice(weak, 150, replace=False):
            x, y, v = int(c % W), int(c // W), 1 + int(c) % S
            for pl in (gt[c], planes[int(c) % len(planes)]):
                a, b = np.float32(r.ncc_new(x, y, v, pl)), np.float32(o.ncc_new(x, y, v, pl))
                assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), (x, y, v, a, b)
                n_new += a < 2.0
        for k in range(600):
            x, y, v = int(px[k, 0]), int(px[k, 1]), 1 + k % S
            a, b = np.float32(r.geom_cost(x, y, v, planes[k])), np.float32(o.geom_cost(x, y, v, planes[k]))
            assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), (x, y, v, a, b)
            n_geom += a < 3.0
        assert n_new > 50 and n_geom > 100
    finally:
        _back_to_contract()
        o.close()
        r.close()


@needs_ref
def test_bresenham_and_point_in_triangle_equal_np_model():
    """BresenhamLine (the walk from its SECOND argument, the step limit, the end-point rule) and PointinTriangle of the
    reference text against the reading of tests/np_model.py, on segments that stay inside the image and on triangles that
    are not collinear (there the side-length test is an equality in the reals and binary32 / binary64 may round it apart)."""
    import np_model as M
    W, H, S, sc, p, st = P.kat_scene()
    rng = np.random.default_rng(11)
    edge = (rng.uniform(size=W * H) < 0.04).astype(np.uint8)      # the scene's own edge map is too sparse to meet often
    r = R.from_scene(sc, p)
    r.upload_state(**dict(st, edge=edge))
    hit = 0
    for _ in range(3000):
        a = (int(rng.integers(2, W - 2)), int(rng.integers(2, H - 2)))
        b = (int(np.clip(a[0] + rng.integers(-14, 15), 2, W - 3)), int(np.clip(a[1] + rng.integers(-14, 15), 2, H - 3)))
        got = r.bresenham(a, b)
        assert got == bool(M.bresenham_hits_edge(edge, W, H, a, b)), (a, b)
        hit += got
    assert 30 < hit < 2970, hit
    inside = n = 0
    while n < 3000:
        t = rng.integers(0, 40, (4, 2))
        if (t[1][0] - t[0][0]) * (t[2][1] - t[0][1]) == (t[1][1] - t[0][1]) * (t[2][0] - t[0][0]):
            continue
        n += 1
        got = r.point_in_triangle(t[0], t[1], t[2], t[3])
        assert got == bool(M._point_in_triangle(t[0], t[1], t[2], t[3])), t
        inside += got
    assert 100 < inside < 2900, inside
    r.close()


# ---- the draws --------------------------------------------------------------------------------------------------------
@needs_ref
def test_draw_table_covers_every_call_site():
    """every cuRAND call site of the cut text is keyed by a line range of oracle/ref_draws.json (the recipe refuses to
    build otherwise); the library holds that table"""
    from oracle import make_ref
    table = json.load(open(make_ref.TABLE))
    assert R.lib().ref_draw_ranges() == len(table["draws"])
    if make_ref.available():
        lines = [l.decode("latin-1") for l in open(os.path.join(make_ref.reference_dir(), "APD.cu"), "rb").read().split(b"\n")]
        cut = lines[:make_ref.cut_device_text(lines)]
        make_ref.check_table(table, cut)
        assert sum(n for _, n in make_ref.draw_sites(cut)) == sum(d["calls"] for d in table["draws"]) == 25
        broken = dict(table, draws=table["draws"][:-1])
        with pytest.raises(RuntimeError):
            make_ref.check_table(broken, cut)


@needs_ref
def test_keyed_launch_reports_no_unkeyed_draw():
    """a launch that draws (random_init of a FIRST_INIT pass: every pixel gets a random plane) runs through the line-keyed
    draws without meeting a line the table does not know (Reference.run_stage raises DrawError otherwise)"""
    sc = synth.make_scene(32, 24, 2)
    p1, _ = P.pass_params(2)
    r = R.from_scene(sc, p1)
    r.upload_state(**P.first_state(sc))
    r.run_stage("random_init")
    assert R.lib().ref_last_bad_line(r.h) == 0
    assert np.isfinite(r.get("costs")).all() and (r.get("planes")[:, 3] != 0).all()
    r.close()


# ---- the goldens --------------------------------------------------------------------------------------------------------
@needs_ref
def test_goldens_are_what_the_reference_text_gives():
    """tests/golden/reference_*.npz and the contract-distance table regenerate to the committed bytes' contents"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_reference_golden", os.path.join(GOLDEN, "make_reference_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    try:
        fresh = G.make_all(distance=False)
    finally:
        _back_to_contract()
    for fname, arrays in fresh.items():
        with np.load(os.path.join(GOLDEN, fname)) as z:
            assert sorted(z.files) == sorted(arrays), fname
            for k in z.files:
                assert count_diff(z[k], np.asarray(arrays[k])) == 0, (fname, k)
