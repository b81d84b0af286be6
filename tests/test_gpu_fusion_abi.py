"""The fusion entry points of include/dvp_mvs.h driven straight through ctypes (the C++ host goes through the same calls):
argument checks, the life cycle of a job, and a case whose answer is known in closed form."""
import ctypes

import numpy as np
import pytest

from conftest import pkg, synth

pytestmark = pytest.mark.gpu


def _lib():
    L = pkg("capi").lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.dvp_fuse_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
    L.dvp_fuse_destroy.argtypes = [vp]
    L.dvp_fuse_last_error.restype = ctypes.c_char_p
    L.dvp_fuse_last_error.argtypes = [vp]
    L.dvp_fuse_set_view.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp, vp]
    L.dvp_fuse_view.argtypes = [vp, ci, vp, ci]
    L.dvp_fuse_view_graded.argtypes = [vp, ci, vp, ci, ci]
    L.dvp_fuse_count.restype = ctypes.c_longlong
    L.dvp_fuse_count.argtypes = [vp]
    L.dvp_fuse_download.argtypes = [vp, vp]
    L.dvp_fuse_last_rounds.argtypes = [vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_fusion_job_life_cycle_and_source_checks():
    L = _lib()
    job = ctypes.c_void_p()
    assert L.dvp_fuse_create(0, 0, ctypes.byref(job)) != 0 and b"bad arguments" in L.dvp_fuse_last_error(None)
    assert L.dvp_fuse_create(0, 3, ctypes.byref(job)) == 0
    W, H = 48, 32
    sc = synth.make_scene(W, H, 2)
    cams = np.ascontiguousarray(sc["cameras"])
    dep = [np.ascontiguousarray(sc["depth_gt"][v], np.float32) for v in range(3)]
    nrm = np.ascontiguousarray(np.tile(sc["normal_gt"].astype(np.float32), (H, W, 1)))
    bgr = np.full((H, W, 3), 77, np.uint8)

    def set_view(v):
        return L.dvp_fuse_set_view(job, v, ctypes.c_void_p(cams.ctypes.data + 112 * v), W, H, _p(dep[v]), _p(nrm), None, _p(bgr), None)
    assert set_view(0) == 0 and set_view(1) == 0
    assert set_view(1) != 0 and b"set before" in L.dvp_fuse_last_error(job)
    assert L.dvp_fuse_set_view(job, 5, _p(cams), W, H, _p(dep[0]), _p(nrm), None, _p(bgr), None) != 0
    src = np.array([1, 2], np.int32)
    assert L.dvp_fuse_view(job, 0, _p(src), 2) != 0 and b"bad source" in L.dvp_fuse_last_error(job)   # view 2 has no maps yet
    for bad in (-1, 3):                                                                                 # no such slot
        assert L.dvp_fuse_view(job, 0, _p(np.array([bad], np.int32)), 1) != 0 and b"bad source" in L.dvp_fuse_last_error(job)
    assert L.dvp_fuse_view(job, 0, _p(np.zeros(65, np.int32)), 65) != 0 and b"64" in L.dvp_fuse_last_error(job)
    assert set_view(2) == 0
    assert L.dvp_fuse_count(job) == 0
    assert L.dvp_fuse_view(job, 0, _p(src), 2) == 0
    n0 = L.dvp_fuse_count(job)
    rounds, rest = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.dvp_fuse_last_rounds(job, ctypes.byref(rounds), ctypes.byref(rest)) == 0 and rounds.value >= 1 and rest.value >= 0
    # true depth maps, one true normal: nearly every pixel of view 0 that both other views see is kept, exactly once
    assert 0.5 * W * H < n0 <= W * H
    assert L.dvp_fuse_view(job, 1, _p(np.array([0, 2], np.int32)), 2) == 0
    assert L.dvp_fuse_view(job, 2, _p(np.array([0, 1], np.int32)), 2) == 0
    n = L.dvp_fuse_count(job)
    # the witnesses of view 0's points were claimed: views 1 and 2 add only what view 0 did not see or could not confirm
    assert n0 <= n < n0 + 0.8 * W * H
    pts = np.zeros((n, 6), np.float32)
    assert L.dvp_fuse_download(job, _p(pts)) == 0
    assert np.isfinite(pts).all() and (pts[:, 3:] == 77).all()          # mean of equal colours
    # the points of view 0 lie on the scene's surface: lift(x, y, depth_gt) — the first n0 records, in raster order
    X = pts[:n0, :3].astype(np.float64)
    cam = sc["cameras"][0]
    R, t, K = cam["R"].astype(np.float64).reshape(3, 3), cam["t"].astype(np.float64), cam["K"].astype(np.float64)
    xc = (R @ X.T).T + t
    u, v = K[0] * xc[:, 0] / xc[:, 2] + K[2], K[4] * xc[:, 1] / xc[:, 2] + K[5]
    assert np.abs(u - np.round(u)).max() < 1e-2 and np.abs(v - np.round(v)).max() < 1e-2          # pixel centres of view 0
    order = np.round(v).astype(np.int64) * W + np.round(u).astype(np.int64)
    assert (np.diff(order) > 0).all()                                                                # scan order
    assert np.abs(xc[:, 2] - dep[0].reshape(-1)[order]).max() < 1e-3
    # a view may be among its own sources, as a pair.txt may list it (APD.cpp:1894-1925 just processes it)
    assert L.dvp_fuse_view(job, 0, _p(np.array([0, 1], np.int32)), 2) == 0, L.dvp_fuse_last_error(job)
    assert L.dvp_fuse_count(job) >= n
    assert L.dvp_fuse_destroy(job) == 0


def test_graded_fusion_counts_every_listed_source():
    """dvp_fuse_view_graded: a source without maps (-1) takes part in the number of sources the acceptance loop runs to but
    never agrees; with one real source no pixel reaches k = 2 agreeing sources."""
    L = _lib()
    job = ctypes.c_void_p()
    assert L.dvp_fuse_create(0, 2, ctypes.byref(job)) == 0
    W, H = 40, 30
    sc = synth.make_scene(W, H, 1)
    cams = np.ascontiguousarray(sc["cameras"])
    nrm = np.ascontiguousarray(np.tile(sc["normal_gt"].astype(np.float32), (H, W, 1)))
    bgr = np.zeros((H, W, 3), np.uint8)
    for v in range(2):
        dep = np.ascontiguousarray(sc["depth_gt"][v], np.float32)
        assert L.dvp_fuse_set_view(job, v, ctypes.c_void_p(cams.ctypes.data + 112 * v), W, H, _p(dep), _p(nrm), None, _p(bgr), None) == 0
    assert L.dvp_fuse_view_graded(job, 0, _p(np.array([1, -1, -1], np.int32)), 3, 0) == 0
    assert L.dvp_fuse_count(job) == 0
    assert L.dvp_fuse_view_graded(job, 0, _p(np.array([1, 7], np.int32)), 2, 1) != 0      # slot 7 does not exist
    assert L.dvp_fuse_destroy(job) == 0


def _plane_job(L, views, nv, shift=0.0):
    """A job over views that see the fronto-parallel plane z = 4 from the same pose; views: (cols, rows, focal) per slot; the
    principal points of the views after the first move by `shift` px (away from rounding ties)."""
    job = ctypes.c_void_p()
    assert L.dvp_fuse_create(0, nv, ctypes.byref(job)) == 0
    cams = np.zeros(len(views), synth.CAMERA_DTYPE)
    keep = []
    for v, (W, H, f) in enumerate(views):
        d = shift if v > 0 else 0.0
        cams[v]["K"] = [f, 0, W / 2.0 + d, 0, f, H / 2.0 + d, 0, 0, 1]
        cams[v]["R"] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        cams[v]["width"], cams[v]["height"] = W, H
        dep = np.full((H, W), 4.0, np.float32)
        nrm = np.ascontiguousarray(np.tile(np.array([0, 0, -1], np.float32), (H, W, 1)))
        bgr = np.ascontiguousarray((np.arange(H * W * 3) % 251).astype(np.uint8).reshape(H, W, 3))
        keep += [dep, nrm, bgr]
        assert L.dvp_fuse_set_view(job, v, ctypes.c_void_p(cams.ctypes.data + 112 * v), W, H, _p(dep), _p(nrm), None, _p(bgr), None) == 0
    return job, keep


def test_fusion_accepts_a_view_among_its_own_sources():
    """A pair.txt may list a view among its own sources: the reference then compares each pixel with itself (APD.cpp:1894-1925),
    a witness at the pixel itself.  Each pixel is the only lister of its candidate, so one resolve round decides everything and
    nothing is left to the sequential finish; every pixel is kept, with its own colour."""
    L = _lib()
    W, H = 64, 48
    job, keep = _plane_job(L, [(W, H, 60.0)], 1)
    assert L.dvp_fuse_view(job, 0, _p(np.array([0], np.int32)), 1) == 0, L.dvp_fuse_last_error(job)
    rounds, rest = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.dvp_fuse_last_rounds(job, ctypes.byref(rounds), ctypes.byref(rest)) == 0
    assert rounds.value == 1 and rest.value == 0, (rounds.value, rest.value)
    assert L.dvp_fuse_count(job) == W * H
    pts = np.zeros((W * H, 6), np.float32)
    assert L.dvp_fuse_download(job, _p(pts)) == 0
    assert (pts[:, 3:].astype(np.uint8) == keep[2].reshape(-1, 3)).all()     # mean of the pixel's colour and its own
    assert L.dvp_fuse_destroy(job) == 0
    # the graded variants (a fresh job: the witnesses above are claimed): the view listed twice agrees with itself at k = 2
    for advanced in (0, 1):
        job, keep = _plane_job(L, [(W, H, 60.0)], 1)
        assert L.dvp_fuse_view_graded(job, 0, _p(np.array([0, 0], np.int32)), 2, advanced) == 0, L.dvp_fuse_last_error(job)
        assert L.dvp_fuse_count(job) == W * H
        assert L.dvp_fuse_destroy(job) == 0


def test_fusion_long_claim_chains_end_in_the_sequential_rest():
    """A source at an eighth of the reference's resolution: each source pixel lies under 8 x 8 reference pixels, a chain of
    pixels that share one witness.  The resolve rounds shorten the chains one pixel per round and hand the rest to the
    sequential finish (last_rounds > 1, last_rest > 0).  The result is the sequential scan's: per source pixel the FIRST lister
    in raster order that the vote accepts takes it, the later ones find it claimed."""
    L = _lib()
    W, H, s = 96, 64, 8
    job, _ = _plane_job(L, [(W, H, 80.0), (W // s, H // s, 80.0 / s)], 2, shift=1.0 / 16)
    assert L.dvp_fuse_view(job, 0, _p(np.array([1], np.int32)), 1) == 0, L.dvp_fuse_last_error(job)
    rounds, rest = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.dvp_fuse_last_rounds(job, ctypes.byref(rounds), ctypes.byref(rest)) == 0
    assert rounds.value > 1 and rest.value > 0, (rounds.value, rest.value)
    n = L.dvp_fuse_count(job)
    pts = np.zeros((n, 6), np.float32)
    assert L.dvp_fuse_download(job, _p(pts)) == 0
    # closed form: pixel (x, y) lands on source pixel (int((x - 48) / 8 + 6 + 1/16 + 0.5), ...), which re-projects to
    # 8 (sx - 6 - 1/16) + 48: err^2 is 0.5 (vote exp(-err) = 0.49) or >= 2.5 (vote <= 0.21, or err >= 2), against the 0.3 of a
    # STRONG pixel (no weak map).  The first lister with err^2 = 0.5 in raster order takes the source pixel.
    c = 1.0 / 16
    want, claimed = [], set()
    for y in range(H):
        sy = int((y - H / 2.0) / s + H / s / 2.0 + c + 0.5)
        for x in range(W):
            sx = int((x - W / 2.0) / s + W / s / 2.0 + c + 0.5)
            if not (0 <= sx < W // s and 0 <= sy < H // s) or (sx, sy) in claimed:
                continue
            err2 = (x - s * (sx - W / s / 2.0 - c) - W / 2.0) ** 2 + (y - s * (sy - H / s / 2.0 - c) - H / 2.0) ** 2
            if err2 < 4 and np.exp(-np.sqrt(err2)) > 0.3:
                claimed.add((sx, sy))
                want.append((x, y))
    assert len(want) == (W // s) * (H // s)
    u = np.round(80.0 * pts[:, 0] / pts[:, 2] + W / 2.0).astype(int)
    v = np.round(80.0 * pts[:, 1] / pts[:, 2] + H / 2.0).astype(int)
    assert list(zip(u.tolist(), v.tolist())) == want
    assert L.dvp_fuse_destroy(job) == 0


def test_fusion_takes_64_sources_and_refuses_65():
    """The stated maximum of dvp_fuse_view / dvp_fuse_view_graded: 64 sources (one bit each in the witness masks).  The same
    source listed 64 times is 64 witnesses with equal votes: the same decisions as listing it once."""
    L = _lib()
    W, H = 40, 30
    sc = synth.make_scene(W, H, 1)
    cams = np.ascontiguousarray(sc["cameras"])
    nrm = np.ascontiguousarray(np.tile(sc["normal_gt"].astype(np.float32), (H, W, 1)))
    bgr = np.full((H, W, 3), 90, np.uint8)
    deps = [np.ascontiguousarray(sc["depth_gt"][v], np.float32) for v in range(2)]

    def run(src, graded=None):
        job = ctypes.c_void_p()
        assert L.dvp_fuse_create(0, 2, ctypes.byref(job)) == 0
        for v in range(2):
            assert L.dvp_fuse_set_view(job, v, ctypes.c_void_p(cams.ctypes.data + 112 * v), W, H, _p(deps[v]), _p(nrm), None, _p(bgr), None) == 0
        src = np.asarray(src, np.int32)
        rc = L.dvp_fuse_view(job, 0, _p(src), len(src)) if graded is None else L.dvp_fuse_view_graded(job, 0, _p(src), len(src), graded)
        err = L.dvp_fuse_last_error(job)
        pts = np.zeros((max(L.dvp_fuse_count(job), 0), 6), np.float32)
        if rc == 0:
            assert L.dvp_fuse_download(job, _p(pts)) == 0
        assert L.dvp_fuse_destroy(job) == 0
        return rc, err, pts

    rc1, _, one = run([1])
    rc64, _, many = run([1] * 64)
    assert rc1 == 0 and rc64 == 0 and len(one) > 0.5 * W * H
    assert np.array_equal(one[:, :3].view(np.uint32), many[:, :3].view(np.uint32))
    rc65, err65, _ = run([1] * 65)
    assert rc65 != 0 and b"64" in err65
    for adv in (0, 1):
        rc, _, pts = run([1] * 64, graded=adv)
        assert rc == 0 and len(pts) > 0.5 * W * H     # 64 agreeing copies: kept at k = 2
        rc, err, _ = run([1] * 65, graded=adv)
        assert rc != 0 and b"64" in err
