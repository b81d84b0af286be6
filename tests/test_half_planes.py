"""Image format 2 (binary16 tiles, Dev::images16): the weak update's planes for image sets that are not 8-bit exact but whose texels
are binary16 values in [0, 255] — the power-of-two down-sampled levels the default schedule runs (multiples of 0.25).  The format
is chosen at upload, in both upload paths, and must leave every buffer bit-identical to the float planes and to the oracle."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import (ROOT, pkg, synth, make_params, count_diff, stage_sequence, CHECKED, first_pass_state,
                      second_pass_inputs)
from oracle import oracle as O

pytestmark = pytest.mark.gpu
wl = pkg("workloads")


def capi():
    return pkg("capi")


def _box_scene(W, H, S):
    sc = synth.make_scene(W, H, S)
    sc["images"] = wl.box2x2(sc["images"])
    frac = np.unique(sc["images"] % np.float32(1.0))
    assert set(frac.tolist()) == {0.0, 0.25, 0.5, 0.75}, frac     # not an 8-bit exact set in disguise
    return sc


def _image_sets(W, H, S):
    sc = synth.make_scene(W, H, S)
    box = wl.box2x2(sc["images"])
    one = box.copy()
    one[1, H // 2, W // 3] = np.float32(100.1)                     # a single texel binary16 cannot hold
    return {"int": sc["images"], "box": box, "scaled": (sc["images"] * np.float32(0.97) + np.float32(1.3)).astype(np.float32),
            "one_inexact": one}, sc


def _context(W, H, NI, monkeypatch, env):
    for k in ("DVP_NO_IMAGES8", "DVP_NO_IMAGES16"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return capi().Context(W, H, NI)


@pytest.mark.parametrize("env,expect", [({}, dict(int=1, box=2, scaled=0, one_inexact=0)),
                                        ({"DVP_NO_IMAGES8": "1"}, dict(int=0, box=0, scaled=0, one_inexact=0)),
                                        ({"DVP_NO_IMAGES16": "1"}, dict(int=1, box=0, scaled=0, one_inexact=0))])
def test_format_is_chosen_at_upload(env, expect, monkeypatch):
    import torch
    W, H, S = 96, 64, 3
    sets, _ = _image_sets(W, H, S)
    g = _context(W, H, S + 1, monkeypatch, env)
    try:
        for name, imgs in sets.items():
            g.set_images(imgs)
            assert g.image_format() == expect[name], ("host upload", name)
            t = torch.from_numpy(np.ascontiguousarray(imgs)).to("cuda")
            g.set_images_device([t[i].data_ptr() for i in range(S + 1)], W)
            torch.cuda.synchronize()
            assert g.image_format() == expect[name], ("device upload", name)
            del t
    finally:
        g.close()


def _weak_pass_inputs(sc, S, border_weak):
    """a FIRST_INIT pass on the oracle, then the REFINE_ITER pass' inputs with WEAK pixels (the scene's flat window; with
    border_weak also frames along the left, right and bottom borders) and a depth range wide enough for footprints to leave the
    source images"""
    H, W = sc["height"], sc["width"]
    p1 = make_params(S + 1, max_iterations=2, state=synth.FIRST_INIT, use_APD=0)
    o = O.from_scene(sc, p1)
    o.upload_state(**first_pass_state(sc))
    o.run_patchmatch()
    st = second_pass_inputs(o, sc)
    o.close()
    weak = st["weak"].reshape(H, W)
    extra = sc["flat"].copy()
    if border_weak:
        extra[H - 12:H - 6, ::2] = True        # (DepthToWeak leaves the 6-pixel frame UNKNOWN)
        extra[6:, 6:11] = True
        extra[6:, W - 11:W - 6] = True
    weak[extra & (weak == synth.STRONG)] = synth.WEAK
    weak[:6, :] = synth.UNKNOWN
    st["weak"] = weak.reshape(-1)
    p2 = make_params(S + 1, max_iterations=2, state=synth.REFINE_ITER, use_APD=1, geom_consistency=1,
                     weak_peak_radius=4, rotate_time=2, ransac_threshold=0.01)
    if border_weak:
        p2["depth_min"] = np.float32(2.5) * np.float32(0.3)
        p2["depth_max"] = np.float32(6.5) * np.float32(2.0)
    return st, p2


def _run_and_compare(a, b, iters, what=""):
    for st, it, col in stage_sequence(iters):
        a.run_stage(st, it, col)
        b.run_stage(st, it, col)
        for n in CHECKED:
            nd = count_diff(a.get(n), b.get(n))
            assert nd == 0, "%s%s differs in %d entries after %s(it=%d, colour=%d)" % (what, n, nd, st, it, col)


@pytest.mark.parametrize("sampler", [0, 1])
@pytest.mark.parametrize("anchors", ["table", "one_wave", "alloc_fail", "per_item"])
def test_two_pass_weak_path_on_half_planes(anchors, sampler, monkeypatch):
    """the twin of test_gpu_parity.py::test_two_pass_weak_path_with_geom on box-filtered images (format 2), both samplers, with
    WEAK pixels along the borders and footprints outside the images (the clamp cases)"""
    monkeypatch.setenv("DVP_WEAK_ANCHOR_TAB", "0" if anchors == "per_item" else "1")
    if anchors == "one_wave":
        monkeypatch.setenv("DVP_WEAK_PHASED", "0")
    if anchors == "alloc_fail":
        monkeypatch.setenv("DVP_TEST_WEAK_PHASE_ALLOC_FAIL", "1")
    W, H, S = 112, 80, 3
    sc = _box_scene(W, H, S)
    st, p2 = _weak_pass_inputs(sc, S, border_weak=True)
    a = O.from_scene(sc, p2, seed=1234, sampler=sampler, depths=sc["depth_gt"])
    b = capi().from_scene(sc, p2, seed=1234, sampler=sampler, depths=sc["depth_gt"])
    a.upload_state(**st)
    b.upload_state(**st)
    assert b.image_format() == 2
    wk = st["weak"].reshape(H, W) == synth.WEAK
    assert a.weak_count() == b.weak_count() > 50
    assert wk[:, :11].sum() > 50 and wk[:, W - 11:].sum() > 50 and wk[H - 12:].sum() > 50
    _run_and_compare(a, b, 2)
    assert (b.get("weak_reliable") == 1).sum() > 0
    a.close()
    b.close()


def test_reupload_switches_format_and_keeps_the_bits(monkeypatch):
    """one context, image sets uploaded in the order 2 -> 1 -> 2 -> 0: after each switch the weak path's buffers are the oracle's
    (no stale plane set, no stale anchor table)"""
    monkeypatch.delenv("DVP_NO_IMAGES8", raising=False)
    monkeypatch.delenv("DVP_NO_IMAGES16", raising=False)
    W, H, S = 96, 72, 3
    sets, sc0 = _image_sets(W, H, S)
    st, p2 = _weak_pass_inputs(_box_scene(W, H, S), S, border_weak=False)
    b = capi().from_scene(dict(sc0, images=sets["box"]), p2, seed=99, depths=sc0["depth_gt"])
    try:
        for name, fmt in (("box", 2), ("int", 1), ("box", 2), ("scaled", 0), ("box", 2)):
            sc = dict(sc0, images=sets[name])
            b.set_images(sets[name])
            assert b.image_format() == fmt, name
            b.upload_state(**st)
            a = O.from_scene(sc, p2, seed=99, depths=sc0["depth_gt"])
            a.upload_state(**st)
            for n in O.BUFFERS:       # what the previous pass left in the recycled context (costs, candidates ...) as well
                a.set(n, b.get(n))
            assert b.weak_count() > 50
            _run_and_compare(a, b, 1, what="after switching to %s (format %d): " % (name, fmt))
            a.close()
    finally:
        b.close()


# ---- the upload probe at tile seams and plane corners ----
# One "spoiler" texel in an integer or box2x2 set.  Widths cover every residue of (W + 4) mod 7, heights every residue of (H + 4)
# mod 8 and so mod 4: the padded plane (kImgPad = 2) against the byte tiles (7 + 1 elements x 8 rows) and the binary16 tiles
# (7 + 1 elements x 4 rows), so the spoiler falls at every place of the last tile column and row.
PROBE_SIZES = [(60 + i, 44 + i) for i in range(8)]
PROBE_S = 3
TO_FORMAT_0 = [255.25, 128.0625, 2.0 ** -25, 100.1]     # in either set: not a binary16 value in [0, 255]
TO_FORMAT_2 = [0.5, 2.0 ** -24, 254.75]                 # in an integer set: binary16-exact, not 8-bit exact


def probe_scene(i):
    W, H = PROBE_SIZES[i]
    return synth.make_scene(W, H, PROBE_S)


def base_images(sc, base):
    return np.asarray(sc["images"], np.float32) if base == "int" else wl.box2x2(sc["images"])


def spoiler_places(sc, i):
    """(image, y, x): (W-1, H-1) of the reference image, (0, 0) of the last source view, the last column of a source view"""
    H, W, NI = sc["height"], sc["width"], len(sc["cameras"])
    return [(0, H - 1, W - 1), (NI - 1, 0, 0), (1 + i % (NI - 1), (5 * i + 3) % H, W - 1)]


def spoiled(images, places, value):
    out = images.copy()
    for k, y, x in places:
        out[k, y, x] = np.float32(value)
    return out


def check_probe(i, formats):
    """formats(images) -> the formats the upload paths report for the set"""
    sc = probe_scene(i)
    for base, fmt in (("int", 1), ("box", 2)):
        assert set(formats(base_images(sc, base))) == {fmt}, (PROBE_SIZES[i], base)
    cases = [(base, v, 0) for base in ("int", "box") for v in TO_FORMAT_0] + [("int", v, 2) for v in TO_FORMAT_2]
    for base, v, fmt in cases:
        for place in spoiler_places(sc, i):
            got = formats(spoiled(base_images(sc, base), [place], v))
            assert set(got) == {fmt}, (PROBE_SIZES[i], base, v, place, got)


def spoiled_weak_pass(i, fmt, make_engine):
    """a weak pass on a set whose spoilers sit inside pixels that WEAK pixels' patches read: one value of TO_FORMAT_2 in the
    integer set (format 2) or of TO_FORMAT_0 in the box set (format 0) at every place of spoiler_places, against the oracle bit for
    bit.  A probe that missed a spoiler would store it rounded in the tiles."""
    sc = probe_scene(i)
    H, W = sc["height"], sc["width"]
    base, values = ("int", TO_FORMAT_2) if fmt == 2 else ("box", TO_FORMAT_0)
    sc = dict(sc, images=spoiled(base_images(sc, base), spoiler_places(sc, i), values[i % len(values)]))
    st, p2 = _weak_pass_inputs(sc, PROBE_S, border_weak=True)
    wk = st["weak"].reshape(H, W) == synth.WEAK
    assert wk[H - 11:, W - 11:].any()     # a WEAK pixel within a patch radius (5) of the reference image's (W-1, H-1)
    a = O.from_scene(sc, p2, seed=1234 + i, sampler=i % 2, depths=sc["depth_gt"])
    b = make_engine(sc, p2, 1234 + i, i % 2)
    assert b.image_format() == fmt
    a.upload_state(**st)
    b.upload_state(**st)
    assert a.weak_count() == b.weak_count() > 50
    _run_and_compare(a, b, 2, what="%dx%d, format %d: " % (W, H, fmt))
    a.close()
    b.close()


@pytest.mark.parametrize("i", range(len(PROBE_SIZES)), ids=lambda i: "%dx%d" % PROBE_SIZES[i])
def test_probe_finds_spoilers_at_tile_seams(i, monkeypatch):
    """both upload paths"""
    import torch
    for k in ("DVP_NO_IMAGES8", "DVP_NO_IMAGES16"):
        monkeypatch.delenv(k, raising=False)
    W, H = PROBE_SIZES[i]
    g = capi().Context(W, H, PROBE_S + 1)

    def formats(imgs):
        g.set_images(imgs)
        host = g.image_format()
        t = torch.from_numpy(np.ascontiguousarray(imgs)).to("cuda")
        g.set_images_device([t[k].data_ptr() for k in range(PROBE_S + 1)], W)
        torch.cuda.synchronize()
        return host, g.image_format()
    try:
        check_probe(i, formats)
    finally:
        g.close()


@pytest.mark.parametrize("fmt", [2, 0])
@pytest.mark.parametrize("i", range(len(PROBE_SIZES)), ids=lambda i: "%dx%d" % PROBE_SIZES[i])
def test_weak_pass_with_spoilers(i, fmt, monkeypatch):
    for k in ("DVP_NO_IMAGES8", "DVP_NO_IMAGES16"):
        monkeypatch.delenv(k, raising=False)
    spoiled_weak_pass(i, fmt, lambda sc, p, seed, smp: capi().from_scene(sc, p, seed=seed, sampler=smp, depths=sc["depth_gt"]))


def _all_buffers_equal(g1, g2, what):
    for n in CHECKED:
        nd = count_diff(g1.get(n), g2.get(n))
        assert nd == 0, "%s: %s differs in %d entries" % (what, n, nd)


def test_regime_size_half_planes_equal_float_planes_and_the_oracle():
    """3104x2064, S = 9, REFINE_ITER with geometric consistency, ~25 % WEAK, box-filtered images: the timed regime of
    tools/half_planes_bench.py.  Format 2 and the float planes (DVP_NO_IMAGES16) leave the same bits on every pixel; launch by
    launch, the oracle's per-pixel bodies reproduce the engine on >= 20 000 sampled pixels (tests/test_fullsize_sampled_parity.py)."""
    import time
    from test_fullsize_sampled_parity import _sample_pixels, _rows, WEAK_IDX
    W, H, S, iters = 3104, 2064, 9, 2
    L = W * H
    env = dict(DVP_WEAK_PHASED_MIN=None, DVP_CAND_MASK="1")      # the shipped weak-update dispatch
    r = wl.quarter_level_pass(W, H, S, iters, 0.25, images="box", env=env)
    g = r["g"]
    assert g.image_format() == 2
    wc = g.weak_count()
    assert 0.18 * L < wc < 0.40 * L, wc / L
    # ---- launch by launch against the oracle on sampled pixels ----
    o = O.Oracle(W, H, S + 1)
    sc = r["sc"]
    o.set_images([sc["images"][i].cpu().numpy() for i in range(S + 1)])
    o.set_depths([sc["depth_gt"][i].cpu().numpy() for i in range(S + 1)])
    o.set_cameras(sc["cameras"])
    o.set_params(r["params"])
    o.set_seed(77)
    o.set_sampler(0)
    pre = {n: g.get(n) for n in O.BUFFERS}
    o.upload_state(planes=pre["planes"], views=pre["selected_views"], weak=pre["weak_info"], edge=pre["edge"], label=pre["label"], radius=pre["radius"])
    assert o.weak_count() == wc
    for n in O.BUFFERS:
        o.set(n, pre[n])
    px = _sample_pixels(W, H, pre["weak_info"], pre["edge"], pre["label"], 16000, np.random.default_rng(2027))
    idx = px[:, 1].astype(np.int64) * W + px[:, 0]
    was_weak = pre["weak_info"][idx] == synth.WEAK
    widx = pre["neighbours_map"][idx[was_weak]].astype(np.int64)
    assert len(px) >= 20000 and was_weak.sum() >= 2000
    del pre
    t0 = time.time()
    for st, it, col in stage_sequence(iters):
        g.run_stage(st, it, col)
        names = [n for n in CHECKED if n != "candidate" or st == "gen_edge_inform"]
        post = {n: g.get(n) for n in names}
        assert o.run_stage_pixels(st, it, col, px) > 0
        for n in names:
            a, b = _rows(n, o.get(n), L, wc), _rows(n, post[n], L, wc)
            sel = widx if n in WEAK_IDX else idx
            if len(sel):
                nd = count_diff(a[sel], b[sel])
                assert nd == 0, "%s differs in %d entries of the %d sampled pixels after %s(it=%d, colour=%d)" % (n, nd, len(sel), st, it, col)
        for n in names:
            o.set(n, post[n])
    o.close()
    print("format 2 at %dx%d: %d sampled pixels (%d WEAK) match the oracle, %.0f s" % (W, H, len(px), int(was_weak.sum()), time.time() - t0))
    # ---- the whole pass on every pixel: format 2 == float planes ----
    g.set("candidate", np.zeros_like(g.get("candidate")))   # dvp_run_patchmatch forms the records at anchor pixels only: start both from zeros
    g.restore_state()
    g.run_patchmatch()
    r2 = wl.quarter_level_pass(W, H, S, iters, 0.25, images="box", env=dict(env, DVP_NO_IMAGES16="1"))
    assert r2["g"].image_format() == 0
    r2["g"].run_patchmatch()
    _all_buffers_equal(g, r2["g"], "format 2 vs float planes at %dx%d" % (W, H))
    r2["g"].close()
    g.close()


def _read_outputs(d):
    out = {}
    for root, _, files in os.walk(os.path.join(d, "APD")):
        for f in files:
            if f.endswith(".dmb") or f.endswith(".ply"):
                out[os.path.relpath(os.path.join(root, f), d)] = open(os.path.join(root, f), "rb").read()
    return out


def test_apd_default_schedule_reads_half_planes(tmp_path):
    """`apd` with the default schedule (--min-scale 2) on a scene whose pyramid has two levels: every pass runs on a down-sampled
    level, whose images take format 2; with DVP_NO_IMAGES16 they take the float planes.  The files are byte-identical."""
    W, H, NV = 1200, 900, 4
    d = str(tmp_path / "scene")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_dataset.py"), d, str(W), str(H), str(NV), "3"], stdout=subprocess.DEVNULL)
    apd = os.path.join(ROOT, "dvp-mvs_amd", "apd")
    runs = {}
    for tag, extra in (("f16", {}), ("f32", {"DVP_NO_IMAGES16": "1"})):
        env = dict(os.environ, DVP_HOST_TIMING="1", **extra)
        env.pop("DVP_NO_IMAGES8", None)
        if not extra:
            env.pop("DVP_NO_IMAGES16", None)
        out = subprocess.run([apd, d, "0", "--iters", "2", "--passes", "1", "--seed", "11"], capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
        gpu = [l for l in out.stdout.splitlines() if "[gpu]" in l]
        assert len(gpu) >= 2 * NV, out.stdout[-2000:]
        assert all(l.rstrip().endswith("images " + tag) for l in gpu), [l[-40:] for l in gpu]
        runs[tag] = _read_outputs(d)
        assert any(k.endswith(".ply") for k in runs[tag]) and sum(k.endswith(".dmb") for k in runs[tag]) >= 2 * NV
        shutil.rmtree(os.path.join(d, "APD"))
    assert sorted(runs["f16"]) == sorted(runs["f32"])
    for k in runs["f16"]:
        assert runs["f16"][k] == runs["f32"][k], k
