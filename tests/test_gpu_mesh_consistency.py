"""dvp_fuse_consistency, the per-view mask the mesher integrates: on the fusion ABI test's scene (with outliers, holes, tilted normals
and a block mask put in) it equals its serial twin (host/fusion.cpp's ConsistencyMaskHost, through tests/consistency_host) byte for
byte at min_views 0, 1, 2 and num_src + 1 - tests/test_mesh_consistency_host.py holds the twin against the float64 model -; it refuses
what it cannot do; and the point list of dvp_fuse_view is the same with the calls as without."""
import ctypes

import numpy as np
import pytest

import np_mesh_mask as K
from conftest import pkg

pytestmark = pytest.mark.gpu

W, H = K.W, K.H


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module", autouse=True)
def built():
    K.build_program()


@pytest.fixture(scope="module")
def L():
    lib = pkg("capi").lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.dvp_fuse_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
    lib.dvp_fuse_destroy.argtypes = [vp]
    lib.dvp_fuse_last_error.restype = ctypes.c_char_p
    lib.dvp_fuse_last_error.argtypes = [vp]
    lib.dvp_fuse_set_view.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.dvp_fuse_view.argtypes = [vp, ci, vp, ci]
    lib.dvp_fuse_count.restype = ctypes.c_longlong
    lib.dvp_fuse_count.argtypes = [vp]
    lib.dvp_fuse_download.argtypes = [vp, vp]
    return lib


@pytest.fixture(scope="module")
def scene():
    return K.scene()


def make_job(L, sc):
    job = ctypes.c_void_p()
    assert L.dvp_fuse_create(0, 3, ctypes.byref(job)) == 0
    for v in range(3):
        assert L.dvp_fuse_set_view(job, v, ctypes.c_void_p(sc["cams"].ctypes.data + 112 * v), W, H, _p(sc["dep"][v]), _p(sc["nrm"][v]), None, _p(sc["bgr"]),
                                   _p(sc["block"]) if v == 0 else None) == 0, L.dvp_fuse_last_error(job)
    return job


@pytest.mark.parametrize("ref, src", K.PAIRS)
def test_the_mask_equals_its_serial_twin(L, scene, tmp_path, ref, src):
    job = make_job(L, scene)
    try:
        src_arr = np.array(src + [0], np.int32)
        for min_views in (0, 1, 2, len(src) + 1):
            mask = np.full(H * W, 9, np.uint8)
            assert L.dvp_fuse_consistency(job, ref, _p(src_arr), len(src), min_views, _p(mask)) == 0, L.dvp_fuse_last_error(job)
            want = K.twin(scene, ref, src, min_views, tmp_path)
            assert mask.tobytes() == want.tobytes(), (min_views, int((mask != want).sum()))
    finally:
        L.dvp_fuse_destroy(job)


def test_refusals(L, scene):
    job = make_job(L, scene)
    try:
        mask = np.zeros(H * W, np.uint8)
        src = np.array([1, 2], np.int32)
        err = lambda: L.dvp_fuse_last_error(job)
        assert L.dvp_fuse_consistency(None, 0, _p(src), 2, 1, _p(mask)) != 0
        assert L.dvp_fuse_consistency(job, 0, _p(src), 2, 1, None) != 0 and b"dvp_fuse_consistency: bad arguments" in err()
        assert L.dvp_fuse_consistency(job, 3, _p(src), 2, 1, _p(mask)) != 0 and b"bad arguments" in err()
        assert L.dvp_fuse_consistency(job, 0, None, 2, 1, _p(mask)) != 0 and b"bad arguments" in err()
        assert L.dvp_fuse_consistency(job, 0, _p(src), -1, 1, _p(mask)) != 0 and b"bad arguments" in err()
        for bad in (-1, 3):
            assert L.dvp_fuse_consistency(job, 0, _p(np.array([bad], np.int32)), 1, 1, _p(mask)) != 0 and b"bad source slot" in err()
    finally:
        L.dvp_fuse_destroy(job)


def test_the_point_list_of_a_later_scan_is_unchanged(L, scene):
    order = [(0, [1, 2]), (1, [0, 2]), (2, [0, 1])]

    def cloud(with_masks):
        job = make_job(L, scene)
        try:
            mask = np.zeros(H * W, np.uint8)
            for v, src in order:
                s = np.array(src, np.int32)
                if with_masks:
                    for w, other in order:      # every view's mask, before each scan
                        assert L.dvp_fuse_consistency(job, w, _p(np.array(other, np.int32)), 2, 2, _p(mask)) == 0
                assert L.dvp_fuse_view(job, v, _p(s), 2) == 0, L.dvp_fuse_last_error(job)
            if with_masks:
                assert L.dvp_fuse_consistency(job, 0, _p(np.array([1, 2], np.int32)), 2, 2, _p(mask)) == 0
            n = L.dvp_fuse_count(job)
            pts = np.zeros((n, 6), np.float32)
            assert L.dvp_fuse_download(job, _p(pts)) == 0
            return pts, mask.copy()
        finally:
            L.dvp_fuse_destroy(job)
    plain, _ = cloud(False)
    masked, after = cloud(True)
    assert len(plain) > 100 and plain.tobytes() == masked.tobytes()
    job = make_job(L, scene)
    try:
        before = np.zeros(H * W, np.uint8)
        assert L.dvp_fuse_consistency(job, 0, _p(np.array([1, 2], np.int32)), 2, 2, _p(before)) == 0
    finally:
        L.dvp_fuse_destroy(job)
    assert (before == after).all()                # ... and the scans' claims do not change a mask
