"""The device level images' arithmetic without a GPU: csrc/dvp_pyramid.hpp, built for the host in tests/pyramid_host and run one
texel after the other, against the numpy model of np_pyramid.py, and both against the host mirror — host/io.cpp ResizeLinear
(tests/host/test_host --resize) on the padded float image, and at equal sizes the canvas itself, where load_image skips the resize.
Every comparison is bitwise on all pixels."""
import numpy as np
import pytest

import np_pyramid as N

pytestmark = pytest.mark.hostbox


@pytest.mark.parametrize("item", N.LEVELS, ids=N.level_id)
def test_serial_build_model_and_mirror_agree(tmp_path, item):
    k, (lw, lh) = item
    img = N.image(k)
    pad_w, pad_h = N.pad_of(k)
    want = N.expected(item)
    rc, got = N.serial(img, lw, lh, pad_w, pad_h)
    assert rc == 0 and N.same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    canvas = N.canvas(img, pad_w, pad_h)
    mirror = canvas if (lw, lh) == (pad_w, pad_h) else N.mirror_resize(tmp_path, canvas, lw, lh)
    assert N.same_bits(mirror, want), int((mirror.view(np.uint32) != want.view(np.uint32)).sum())


def test_cases_say_what_they_claim():
    for k, case in enumerate(N.CASES):
        img = N.image(k)
        assert img.shape == case[0][::-1] and img.max() == 255 and (img.size == 1 or img.min() == 0)
    assert N.image(0).strides[0] == 80
    # 123 -> 62, 77 -> 39, 1082 -> 271 are halves rounded away from zero, and their fractions are not binary16 values
    assert (N.round_half_away(123, 2), N.round_half_away(77, 2), N.round_half_away(1082, 4), N.round_half_away(838, 8)) == (62, 39, 271, 105)
    for k in (3, 4):
        e = N.expected((k, N.CASES[k][2][0]))
        assert not (e.astype(np.float16).astype(np.float32) == e).all()
    # exact halves: multiples of 0.25, not all integers
    e = N.expected((1, (48, 32)))
    assert (e * 4 == np.floor(e * 4)).all() and not (e == np.floor(e)).all()
    # up-sampling: the low and the high clamp both fire, in x and in y
    for n_src, n_dst in ((40, 100), (30, 70), (1, 3), (1, 2)):
        i0, i1, f = N.taps(n_src, n_dst)
        raw = np.floor(((np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5).astype(np.float32))
        assert (raw < 0).any() and (raw >= n_src - 1).any() and f[0] == 0 and f[-1] == 0
    # padding: a destination pixel blends the image's last column with the zero canvas, and others lie wholly outside
    (sw, sh), (pw, ph) = N.CASES[8][0], N.CASES[8][1]
    e = N.expected((8, (48, 32)))
    assert (e[:, 36:] == 0).all() and (e[24:, :] == 0).all() and (e[:24, :36] != 0).any()
    for n_img, n_lvl in ((71, 48), (47, 32)):
        i0, i1, f = N.taps(96 if n_img == 71 else 64, n_lvl)
        assert ((i0 == n_img - 1) & (i1 == n_img) & (f > 0)).any()
    e, img = N.expected((11, (48, 32))), N.image(11).astype(np.float32)
    assert np.array_equal(e[:23, 35], (img[0:46:2, 70] * np.float32(0.5)) * np.float32(0.5) + (img[1:47:2, 70] * np.float32(0.5)) * np.float32(0.5))
    straddle = N.expected((8, (96, 64)))
    assert np.array_equal(straddle[:sh, :sw], N.image(8).astype(np.float32)) and (straddle[sh:] == 0).all() and (straddle[:, sw:] == 0).all()
    # crop: the level does not depend on what lies beyond the canvas
    img = N.image(9).copy()
    img[:, 96:] ^= 0xff
    img[64:, :] ^= 0xff
    assert N.same_bits(N.level(img, 48, 32, 96, 64), N.expected((9, (48, 32))))


def test_pad_zero_means_the_images_own_size():
    img = N.image(3)
    rc, got = N.serial(img, 62, 39)
    assert rc == 0 and N.same_bits(got, N.expected((3, (62, 39))))


@pytest.mark.parametrize("lw,lh,pad_w,pad_h", [(0, 4, 8, 8), (4, 0, 8, 8), (4, 4, -1, 8), (4, 4, 8, -2)])
def test_bad_sizes_are_an_error(lw, lh, pad_w, pad_h):
    rc, _ = N.serial(np.zeros((8, 8), np.uint8), lw, lh, pad_w, pad_h)
    assert rc != 0


def test_the_library_exports_the_store_and_the_upload():
    """every dvp_images_* entry point of include/dvp_mvs.h, dvp_upload_images_u8 and dvp_download_image (the library loads without a GPU)"""
    import os
    import re
    from conftest import ROOT, pkg
    hdr = open(os.path.join(ROOT, "include", "dvp_mvs.h")).read()
    declared = set(re.findall(r"\b(dvp_images_[a-z_]+|dvp_upload_images_u8|dvp_download_image)\s*\(", hdr))
    assert declared == {"dvp_images_create", "dvp_images_destroy", "dvp_images_put", "dvp_images_drop", "dvp_images_size", "dvp_images_bytes", "dvp_images_level",
                        "dvp_images_last_error", "dvp_upload_images_u8", "dvp_download_image"}
    capi = pkg("capi")
    assert declared <= set(capi.EXPORTS + capi.EXPORTS_WITH_DIGITS)
    L = capi.lib()
    for name in declared:
        assert hasattr(L, name), name
