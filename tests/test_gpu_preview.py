"""The device JPEG encoder and the preview images on the GPU: files byte-identical to libjpeg-turbo's (Pillow) at the restart
interval the engine chose, previews equal to the numpy reading of the reference's renderers (np_preview)."""
import numpy as np
import pytest

import np_preview as P
from conftest import make_params, pkg, synth

capi = pkg("capi")
KINDS = dict(depth=capi.PREVIEW_DEPTH, normal=capi.PREVIEW_NORMAL, weak=capi.PREVIEW_WEAK)


def images(rs, W, H, C):
    sh = (H, W) if C == 1 else (H, W, 3)
    g = np.add.outer(np.arange(H, dtype=np.int64) * 3, np.arange(W, dtype=np.int64) * 2) % 256
    grad = g if C == 1 else np.stack([g, 255 - g, (g * 7) % 256], -1)
    return dict(noise=rs.randint(0, 256, sh).astype(np.uint8), const=np.full(sh, 255, np.uint8), grad=grad.astype(np.uint8))


def check_file(img, q, got, R_asked):
    """`got` (the engine's file for `img`) equals Pillow's at the restart interval read from got's DRI segment, and decodes
    to what Pillow's marker-free file decodes to"""
    R = P.dri(got)
    assert R >= 1 and (R_asked == 0 or R == R_asked)
    ref = P.pil_jpeg(img, q, R)
    assert got == ref, (img.shape, q, R, len(got), len(ref))
    return R


SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (1000, 3), (255, 129), (3104, 2064), (6208, 4128)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("C", [1, 3])
def test_jpeg_encode_equals_libjpeg_turbo(W, H, C):
    rs = np.random.RandomState(W + 3 * H + C)
    big = W * H > 1 << 20
    for name, img in images(rs, W, H, C).items():
        for q in (50, 75, 95, 100):
            for R in (0, 1):
                got = capi.jpeg_encode(img, q, R)
                check_file(img, q, got, R)
                if R == 0 and (not big or q == 95):
                    a, b = P.decode(got), P.decode(P.pil_jpeg(img, q, None))
                    assert np.array_equal(a, b), (W, H, C, name, q)


@pytest.mark.gpu
def test_jpeg_encode_arguments():
    img = np.zeros((9, 9, 3), np.uint8)
    with pytest.raises(capi.DvpError):
        capi.jpeg_encode(img, 0)
    with pytest.raises(capi.DvpError):
        capi.jpeg_encode(img, 95, 70000)
    # a strided view (pitch > width * 3) encodes like its contiguous copy
    wide = np.random.RandomState(2).randint(0, 256, (40, 64, 3)).astype(np.uint8)
    assert capi.jpeg_encode(wide[:, 5:50], 90, 3) == capi.jpeg_encode(np.ascontiguousarray(wide[:, 5:50]), 90, 3)


def crafted(W, H, dmin, dmax, rs):
    from test_preview_host import crafted_state
    planes, weak = crafted_state(dmin, dmax, rs)
    n = W * H
    reps = (n + len(planes) - 1) // len(planes)
    return np.tile(planes, (reps, 1))[:n].copy(), np.tile(weak, reps)[:n].copy()


def previews_of(ctx, q):
    ctx.preview_begin(capi.PREVIEW_DEPTH | capi.PREVIEW_NORMAL | capi.PREVIEW_WEAK, q)
    return {k: (ctx.preview_pixels(v), ctx.preview_finish(v)) for k, v in KINDS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,dmin,dmax", [(61, 37, 1.5, 7.8), (128, 96, -2.0, 3.0), (33, 17, 2.0, 2.0)])
def test_previews_from_crafted_state(W, H, dmin, dmax):
    rs = np.random.RandomState(W)
    planes, weak = crafted(W, H, dmin, dmax, rs)
    p = make_params(2)
    p["depth_min"], p["depth_max"] = np.float32(dmin), np.float32(dmax)
    ctx = capi.Context(W, H, 2)
    try:
        ctx.set_params(p)
        ctx.upload_state(planes=planes, weak=weak)
        ref = P.previews(planes, weak, dmin, dmax, H, W)
        for q in (95, 60):
            got = previews_of(ctx, q)
            for k in KINDS:
                pix, jpg = got[k]
                assert np.array_equal(pix, ref[k]), (k, int((pix != ref[k]).any(2).sum()))
                check_file(ref[k], q, jpg, 0)
        # only the kinds asked for are available
        ctx.preview_begin(capi.PREVIEW_WEAK, 95)
        with pytest.raises(capi.DvpError):
            ctx.preview_finish(capi.PREVIEW_DEPTH)
        ctx.preview_begin(capi.PREVIEW_WEAK, 60)
        assert ctx.preview_finish(capi.PREVIEW_WEAK) == got["weak"][1]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_previews_after_a_pass():
    W, H, S = 160, 112, 3
    sc = synth.make_scene(W, H, S)
    p = make_params(S + 1, max_iterations=2, state=synth.FIRST_INIT)
    g = capi.from_scene(sc, p)
    try:
        g.upload_state(planes=np.zeros((H * W, 4), np.float32), edge=sc["edge"], label=sc["label"], radius=np.full(H * W, 5, np.int32))
        g.run_patchmatch()
        planes, weak = g.get("planes"), g.get("weak_info")
        dmin, dmax = float(p["depth_min"]), float(p["depth_max"])
        ref = P.previews(planes, weak, dmin, dmax, H, W)
        # the maps the driver stores give the same images
        depth, normal, _, state, _ = g.download_maps()
        assert np.array_equal(P.depth_preview(depth, dmin, dmax).reshape(H, W, 3), ref["depth"])
        assert np.array_equal(P.weak_preview(state).reshape(H, W, 3), ref["weak"])
        got = previews_of(g, 95)
        for k in KINDS:
            assert np.array_equal(got[k][0], ref[k]), k
            check_file(ref[k], 95, got[k][1], 0)
        assert len(np.unique(ref["depth"].reshape(-1, 3), axis=0)) > 20   # a real depth map, not a blank image
    finally:
        g.close()
