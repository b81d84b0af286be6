"""The level images made on the device (csrc/dvp_pyramid.hip, include/dvp_mvs.h dvp_images_* / dvp_upload_images_u8) against the
numpy model of np_pyramid.py (host/APD.cpp load_image + host/io.cpp ResizeLinear): every level of every case bit for bit, the
store's bookkeeping, and a context fed through dvp_upload_images_u8 against one fed the model's floats through dvp_upload_images —
the images it holds, dvp_image_format, and a REFINE_ITER pass with geometric consistency and WEAK pixels (the only reader of the
byte and binary16 tiles) — for formats 1, 2 and 0, with one source file smaller and one larger than the reference."""
import ctypes
import threading

import numpy as np
import pytest

import np_pyramid as N
from conftest import pkg, synth, count_diff, stage_sequence

pytestmark = pytest.mark.gpu

W, H, S, ITERS = 192, 128, 3, 2
# name -> (size of the reference's file, expected dvp_image_format, environment while the contexts are created)
SETS = {
    "scale1": ((192, 128), 1, {}),
    "half": ((384, 256), 2, {}),
    "inexact": ((383, 255), 0, {}),              # 191.5 -> 192, 127.5 -> 128: fractions that are no binary16 values
    "half-no16": ((384, 256), 0, {"DVP_NO_IMAGES16": "1"}),
}
COMPARED = ["planes", "costs", "selected_views", "weak_info"]
_SCENES = {}


def capi():
    return pkg("capi")


def workloads():
    return pkg("workloads")


@pytest.fixture(scope="module")
def store():
    st = capi().ImageStore()
    for k in range(len(N.CASES)):
        st.put(k, N.image(k))
    yield st
    st.close()


# ---- levels
@pytest.mark.parametrize("item", N.LEVELS, ids=N.level_id)
def test_levels_equal_the_model(store, item):
    k, (lw, lh) = item
    pad = N.CASES[k][1] or (0, 0)
    got = store.level(k, lw, lh, *pad)
    want = N.expected(item)
    assert N.same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    if not N.CASES[k][1]:   # the image's own size, stated
        assert N.same_bits(store.level(k, lw, lh, *N.CASES[k][0]), want)


def test_store_bookkeeping(store):
    c = capi()
    assert store.bytes() == sum(w * h for (w, h), _, _, _ in N.CASES)
    assert store.size(0) == (67, 35) and store.size(4) == (40, 1082)
    with pytest.raises(c.DvpError, match="already"):
        store.put(3, N.image(1))
    assert store.size(3) == (123, 77)                       # ... and the image is still the old one
    assert N.same_bits(store.level(3, 62, 39), N.expected((3, (62, 39))))
    st = c.ImageStore()
    st.put(7, N.image(3))
    before = st.bytes()
    st.drop(7)
    assert st.bytes() == 0 and before == 123 * 77
    with pytest.raises(c.DvpError, match="not in the store"):
        st.size(7)
    with pytest.raises(c.DvpError, match="not in the store"):
        st.drop(7)
    st.put(7, N.image(1))                                   # another image under the same id
    assert st.size(7) == (96, 64) and st.bytes() == 96 * 64
    assert N.same_bits(st.level(7, 48, 32), N.expected((1, (48, 32))))
    st.close()


# ---- a context fed from the store
def scene(name, seed=1234):
    """the files (uint8), the model's level floats, and the level-size cameras / depths / priors; computed once, never modified"""
    key = (name, seed)
    if key not in _SCENES:
        (bw, bh), fmt, env = SETS[name]
        sc = synth.make_scene(bw, bh, S, seed=seed)
        rng = np.random.default_rng(seed + 5)
        files = [sc["images"][i].astype(np.uint8) for i in range(S + 1)]
        assert all((f == sc["images"][i]).all() for i, f in enumerate(files))
        files[1] = np.ascontiguousarray(files[1][:bh - 16, :bw - 24])             # a smaller file: zero padding
        big = rng.integers(0, 256, (bh + 8, bw + 16), dtype=np.uint8)             # a larger one: cropped
        big[:bh, :bw] = files[2]
        files[2] = big
        floats = np.stack([N.level(f, W, H, bw, bh) for f in files])
        cams = sc["cameras"].copy()
        step = 1 if (bw, bh) == (W, H) else 2
        for cam in cams:                                                          # the driver's camera scaling
            if step == 2:
                cam["K"][[0, 2, 4, 5]] *= np.float32(0.5)
            cam["width"], cam["height"] = W, H
        sub = lambda a: np.ascontiguousarray(a[..., ::step, ::step][..., :H, :W])
        out = dict(files=files, floats=floats, cameras=cams, depths=sub(sc["depth_gt"]), edge=sub(sc["edge"]), label=sub(sc["label"]), flat=sub(sc["flat"]),
                   pad=(bw, bh), fmt=fmt, env=env)
        for v in [floats, out["depths"], out["edge"], out["label"]] + files:
            v.setflags(write=False)
        _SCENES[key] = out
    return _SCENES[key]


def put_scene(st, sc, base=0):
    ids = [base + i for i in range(S + 1)]
    for i, f in zip(ids, sc["files"]):
        st.put(i, f)
    return ids


def load(g, sc, st=None, ids=None):
    if st is None:
        g.set_images(sc["floats"])
    else:
        g.set_images_u8(st, ids, *sc["pad"])


def first_pass(g, sc):
    """workloads.quarter_level_pass's set-up on a context that holds its images: a FIRST_INIT pass, its hand-over with WEAK tiles,
    the REFINE_ITER parameters and the depth maps; returns the second pass's input state"""
    wl = workloads()
    L = W * H
    g.set_cameras(sc["cameras"])
    p1 = wl.first_init_params(S, ITERS)
    g.set_params(p1)
    g.set_seed(77)
    g.upload_state(planes=np.zeros((L, 4), np.float32), views=np.zeros(L, np.uint32), weak=np.full(L, synth.STRONG, np.uint8),
                   edge=sc["edge"], label=sc["label"], radius=np.full(L, 5, np.int32))
    g.run_patchmatch()
    st = wl.hand_over(g.get("planes"), g.get("selected_views"), g.get("weak_info"), g.get("radius"), p1, W, H,
                      extra_weak=wl.weak_tiles(W, H, 0.15, sc["flat"]))
    g.set_params(wl.refine_iter_params(S, ITERS, round_index=2))
    g.set_depths(sc["depths"])
    return dict(planes=st[0], views=st[1], weak=st[2], radius=st[3])


def snapshot(g):
    return {n: g.get(n).copy() for n in COMPARED}


def whole_flow(sc, st=None, ids=None, by_stages=False):
    g = capi().Context(W, H, S + 1)
    load(g, sc, st, ids)
    fmt = g.image_format()
    images = [g.image(i) for i in range(S + 1)]
    state = first_pass(g, sc)
    g.upload_state(**state)
    weak = g.weak_count()
    if by_stages:
        for stg, it, col in stage_sequence(ITERS):
            g.run_stage(stg, it, col)
    else:
        g.run_patchmatch()
    out = snapshot(g)
    g.close()
    return dict(fmt=fmt, images=images, state=state, weak=weak, out=out)


@pytest.mark.parametrize("name", list(SETS))
def test_context_from_the_store_equals_context_from_the_models_floats(name, monkeypatch):
    sc = scene(name)
    for k, v in sc["env"].items():
        monkeypatch.setenv(k, v)
    st = capi().ImageStore()
    ids = put_scene(st, sc, base=40)
    a = whole_flow(sc)
    b = whole_flow(sc, st, ids)
    st.close()
    assert a["fmt"] == b["fmt"] == sc["fmt"], (a["fmt"], b["fmt"])
    for i in range(S + 1):
        assert N.same_bits(a["images"][i], sc["floats"][i]) and N.same_bits(b["images"][i], sc["floats"][i]), i
    # the files do what they were built for: zeros right of and below the smaller file's level, the larger one's excess is gone
    assert (sc["floats"][1][:, -10:] == 0).all() and (sc["floats"][1][-6:, :] == 0).all() and (sc["floats"][3] != 0).any()
    assert a["weak"] == b["weak"] and b["weak"] > 0
    assert count_diff(b["out"]["planes"], b["state"]["planes"]) > 0       # the pass did change the planes
    for n in a["state"]:
        assert count_diff(a["state"][n], b["state"][n]) == 0, "first pass: " + n
    for n in COMPARED:
        nd = count_diff(a["out"][n], b["out"][n])
        assert nd == 0, "%s differs in %d entries" % (n, nd)


def test_new_images_through_the_store_empty_the_plane_cache():
    """default DVP_STRONG_REUSE: a context runs a pass stage by stage, gets OTHER images through set_images_u8 and the same
    state, and runs again: the result is a fresh context's on the second images"""
    sc1, sc2 = scene("half"), scene("half", seed=4321)
    assert count_diff(sc1["floats"], sc2["floats"]) > W * H
    sc2 = dict(sc2, cameras=sc1["cameras"], depths=sc1["depths"], edge=sc1["edge"], label=sc1["label"], flat=sc1["flat"])   # only the images differ
    st = capi().ImageStore()
    ids1, ids2 = put_scene(st, sc1, 0), put_scene(st, sc2, 10)
    g = capi().Context(W, H, S + 1)
    g.set_images_u8(st, ids1, *sc1["pad"])
    state = first_pass(g, sc1)
    g.upload_state(**state)
    for stg, it, col in stage_sequence(ITERS):
        g.run_stage(stg, it, col)
    first = snapshot(g)
    g.set_images_u8(st, ids2, *sc2["pad"])
    g.upload_state(**state)
    for stg, it, col in stage_sequence(ITERS):
        g.run_stage(stg, it, col)
    got = snapshot(g)
    g.close()
    fresh = capi().Context(W, H, S + 1)
    fresh.set_images(sc2["floats"])
    fresh.set_cameras(sc1["cameras"])
    fresh.set_params(workloads().refine_iter_params(S, ITERS, round_index=2))
    fresh.set_seed(77)
    fresh.set_depths(sc1["depths"])
    fresh.upload_state(edge=sc1["edge"], label=sc1["label"], **state)
    for stg, it, col in stage_sequence(ITERS):
        fresh.run_stage(stg, it, col)
    want = snapshot(fresh)
    fresh.close()
    st.close()
    assert count_diff(want["planes"], first["planes"]) > 0               # the second images do give another result
    for n in COMPARED:
        nd = count_diff(want[n], got[n])
        assert nd == 0, "%s differs in %d entries" % (n, nd)


def test_two_threads_upload_while_the_store_grows():
    """two threads, a context each, upload four image sets from one store while the main thread puts new ids: what every upload
    leaves in the context is what it leaves in a serial run — the model's floats"""
    sets = [scene("half"), scene("inexact"), scene("half", seed=4321), scene("scale1")]
    st = capi().ImageStore()
    ids = [put_scene(st, sc, 10 * k) for k, sc in enumerate(sets)]
    results, errors = {}, []

    def worker(t):
        try:
            g = capi().Context(W, H, S + 1)
            for r in range(4):
                k = (r + t) % 4
                g.set_images_u8(st, ids[k], *sets[k]["pad"])
                results[(t, r)] = (k, g.image_format(), [g.image(i) for i in range(S + 1)])
            g.close()
        except Exception as e:   # noqa: BLE001 — reported by the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    extra = 0
    while any(th.is_alive() for th in threads) or extra < 8:
        st.put(1000 + extra, N.image(extra % len(N.CASES)))
        extra += 1
        if extra >= 64:
            break
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(results) == 8
    for (t, r), (k, fmt, images) in results.items():
        assert fmt == sets[k]["fmt"], (t, r, k, fmt)
        for i in range(S + 1):
            assert N.same_bits(images[i], sets[k]["floats"][i]), (t, r, k, i)
    for e in range(extra):   # ... and what was put meanwhile is served
        k = e % len(N.CASES)
        assert st.size(1000 + e) == N.CASES[k][0]
    assert N.same_bits(st.level(1003, 62, 39), N.expected((3, (62, 39))))
    st.close()


def test_bad_arguments_leave_the_context_alone():
    c = capi()
    L = c.lib()
    sc = scene("half")
    st = c.ImageStore()
    ids = put_scene(st, sc)
    g = c.Context(W, H, S + 1)
    g.set_images(sc["floats"][::-1])                 # some previous images
    held = g.image(0)
    assert N.same_bits(held, sc["floats"][S])
    bw, bh = sc["pad"]
    arr = lambda v: np.ascontiguousarray(v, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def refused(rc):
        assert rc != 0
        assert L.dvp_last_error(g.h).decode().startswith("dvp_upload_images_u8"), L.dvp_last_error(g.h)
        assert N.same_bits(g.image(0), held) and g.image_format() == 2

    good = arr(ids)
    refused(L.dvp_upload_images_u8(g.h, None, ptr(good), bw, bh))                    # null pointers
    refused(L.dvp_upload_images_u8(g.h, st.h, None, bw, bh))
    assert L.dvp_upload_images_u8(None, st.h, ptr(good), bw, bh) != 0
    refused(L.dvp_upload_images_u8(g.h, st.h, ptr(arr(ids[:3] + [99])), bw, bh))     # a missing id
    for pw, ph in ((0, bh), (bw, 0), (-1, -1), (40000, bh)):                         # sizes smaller than 1 (and too large)
        refused(L.dvp_upload_images_u8(g.h, st.h, ptr(good), pw, ph))
    refused(L.dvp_upload_images_u8(g.h, st.h, ptr(good), bw - 1, bh))                # ids[0] not of pad size
    refused(L.dvp_upload_images_u8(g.h, st.h, ptr(arr([ids[1]] + ids[1:])), bw, bh))
    # a store on another device index: with one device the store itself is refused, with several the upload is
    other = ctypes.c_void_p()
    if L.dvp_images_create(1, ctypes.byref(other)) != 0:
        assert L.dvp_images_last_error().decode() and not other.value
    else:
        try:
            for i, f in zip(ids, sc["files"]):
                assert L.dvp_images_put(other, i, ptr(f), f.shape[1], f.shape[0], f.strides[0]) == 0
            refused(L.dvp_upload_images_u8(g.h, other, ptr(good), bw, bh))
        finally:
            L.dvp_images_destroy(other)
    # the store's own calls
    f = sc["files"][0]

    def store_refused(rc):
        assert rc != 0 and L.dvp_images_last_error().decode().startswith("dvp_images_")

    before = st.bytes()
    store_refused(L.dvp_images_put(st.h, 50, None, bw, bh, bw))
    store_refused(L.dvp_images_put(None, 50, ptr(f), bw, bh, bw))
    store_refused(L.dvp_images_put(st.h, 50, ptr(f), bw, bh, bw - 1))                # pitch smaller than width
    store_refused(L.dvp_images_put(st.h, 50, ptr(f), 0, bh, bw))
    store_refused(L.dvp_images_put(st.h, 50, ptr(f), bw, -3, bw))
    out = np.zeros((H, W), np.float32)
    store_refused(L.dvp_images_level(st.h, ids[0], 0, 0, W, H, None))
    store_refused(L.dvp_images_level(st.h, 99, 0, 0, W, H, ptr(out)))
    store_refused(L.dvp_images_level(st.h, ids[0], 0, 0, 0, H, ptr(out)))
    store_refused(L.dvp_images_level(st.h, ids[0], 0, 0, W, -1, ptr(out)))
    store_refused(L.dvp_images_level(st.h, ids[0], -2, bh, W, H, ptr(out)))
    store_refused(L.dvp_images_level(st.h, ids[0], bw, 0, W, H, ptr(out)))
    store_refused(L.dvp_images_create(0, None))
    assert st.bytes() == before and (out == 0).all()
    with pytest.raises(c.DvpError):
        st.size(50)
    # Context.image's own arguments
    assert L.dvp_download_image(g.h, S + 1, ptr(out), W) != 0 and L.dvp_download_image(g.h, 0, ptr(out), W - 1) != 0 and L.dvp_download_image(g.h, 0, None, W) != 0
    fresh = c.Context(W, H, S + 1)
    assert L.dvp_download_image(fresh.h, 0, ptr(out), W) != 0                       # no images yet
    fresh.close()
    # ... and the good call still works afterwards
    g.set_images_u8(st, ids, bw, bh)
    assert N.same_bits(g.image(0), sc["floats"][0]) and g.image_format() == 2
    g.close()
    st.close()
