"""The out-of-memory paths of the side stages (edges, view clean-up, previews, labels, level images, plane prior, fusion): every
device block they own goes through DevBlock::reserve (csrc/dvp_devmem.hpp), which DVP_TEST_SIDE_ALLOC_FAIL=N makes refuse every
request of at least N bytes.  Each entry point runs under a sweep of N over the powers of two from 1 to above the largest block
the call can ask for; a fresh job, store or context per N, since a scratch that already fits asks for nothing.  At every N the
call either raises DvpError with "out of device memory" in its text or returns what a run without the variable returns; N = 1
must raise and the largest N must succeed.  After each refusal the same job, with the variable removed, gives what a fresh one
gives, and launch-checked calls on an engine context still return 0: no sticky status was left behind."""
import ctypes

import numpy as np
import pytest

import np_labels as NL
import np_prior as NP
from conftest import make_params, pkg, synth

pytestmark = pytest.mark.gpu

VAR = "DVP_TEST_SIDE_ALLOC_FAIL"
REFUSED = "out of device memory"


def capi():
    return pkg().get_capi()


def thresholds(largest_block):
    out, t = [], 1
    while True:
        out.append(t)
        if t > largest_block:
            return out
        t *= 2


def small_context(W=96, H=64):
    sc = synth.make_scene(W, H, 1)
    g = capi().from_scene(sc, make_params(2))
    g.upload_state(planes=np.zeros((H * W, 4), np.float32), edge=sc["edge"], label=sc["label"], radius=np.full(H * W, 5, np.int32))
    return g


@pytest.fixture(scope="module")
def witness():
    """an engine context whose launch-checked calls show a status that an earlier call left behind"""
    g = small_context()
    yield g
    g.close()


def no_sticky_status(witness):
    witness.synchronize()
    witness.edge_map_begin(False)     # (its launches are followed by hipGetLastError)
    witness.edge_map_finish()
    witness.synchronize()


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def sweep(monkeypatch, witness, largest_block, call, make=lambda: None, close=lambda job: None, refused_state=lambda job: None):
    """call(job) under every threshold, on a job that make() made without the variable; returns how many thresholds refused"""
    monkeypatch.delenv(VAR, raising=False)
    job = make()
    want = call(job)
    close(job)
    ts = thresholds(largest_block)
    refused = 0
    for t in ts:
        job = make()
        try:
            monkeypatch.setenv(VAR, str(t))
            try:
                got, error = call(job), None
            except capi().DvpError as e:
                got, error = None, str(e)
            monkeypatch.delenv(VAR)
            if error is None:
                assert t != 1, "a threshold of one byte refused nothing"
                assert same(got, want), t
            else:
                assert REFUSED in error, (t, error)
                assert t != ts[-1], (t, error)
                refused += 1
                refused_state(job)
                assert same(call(job), want), t       # the same job as a fresh one
                no_sticky_status(witness)
        finally:
            monkeypatch.delenv(VAR, raising=False)
            close(job)
    assert refused >= 1
    return refused


def smooth_image(W, H, seed):
    rs = np.random.RandomState(seed)
    a = rs.rand(H + 4, W + 4)
    a = sum(np.roll(np.roll(a, dy, 0), dx, 1) for dy in range(-2, 3) for dx in range(-2, 3))[2:-2, 2:-2]
    a = (a - a.min()) / (a.max() - a.min())
    return np.ascontiguousarray(np.rint(a * 255 + rs.rand(H, W) * 12).clip(0, 255).astype(np.uint8))


# ---- the one-shot calls ---------------------------------------------------------------------------------------------------------
def test_canny_edge_map(monkeypatch, witness):
    W, H = 37, 29
    img = smooth_image(W, H, 3)
    assert capi().canny_edge_map(img).any()
    # one scratch block of under 8 bytes per pixel + 5 x 256 of alignment + 1032, one map of a byte per pixel
    sweep(monkeypatch, witness, 8 * W * H + 4096, lambda _: capi().canny_edge_map(img))


def test_edge_hysteresis(monkeypatch, witness):
    W, H = 37, 29
    m = np.random.RandomState(5).choice(np.array([0, 0, 1, 1, 1, 2], np.uint8), (H, W))
    assert capi().edge_hysteresis(m).any()
    sweep(monkeypatch, witness, 8 * W * H + 4096, lambda _: capi().edge_hysteresis(m))


def test_clean_selected_views(monkeypatch, witness):
    W, H, S = 70, 41, 3
    words = (np.random.RandomState(70 * 31 + 41).rand(H, W, S) < 0.6).astype(np.uint32)
    words = np.ascontiguousarray((words << np.arange(S, dtype=np.uint32)).sum(2).astype(np.uint32))
    assert not same(capi().clean_selected_views(words, S, 6), words)
    # a parent and a size word per plane and pixel; the words
    sweep(monkeypatch, witness, 8 * S * W * H, lambda _: capi().clean_selected_views(words, S, 6))


@pytest.mark.parametrize("W,H,C", [(17, 9, 1), (33, 17, 3)])
def test_jpeg_encode(monkeypatch, witness, W, H, C):
    img = np.random.RandomState(W).randint(0, 256, (H, W) if C == 1 else (H, W, 3)).astype(np.uint8)
    # per 8 x 8 block 128 bytes of coefficients, at most 6 blocks per 16 x 16 pixels; the tables; the output is below dvp_jpeg_bound
    largest = max(int(capi().lib().dvp_jpeg_bound(W, H, C)), 65536)
    sweep(monkeypatch, witness, largest, lambda _: capi().jpeg_encode(img, 90))


# ---- the label prior ------------------------------------------------------------------------------------------------------------
LABEL_CASE = ("frame", 63, 65, 2)


def test_label_job_run(monkeypatch, witness):
    c, W, H, s = LABEL_CASE
    img = NL.image(c, W, H, s)
    # the pool: under 16 bytes per full-size pixel and 13 x 256 of alignment
    sweep(monkeypatch, witness, 16 * W * H + 8192, lambda job: job.run(img, s), make=capi().LabelJob, close=lambda job: job.close())


def test_label_map(monkeypatch, witness):
    c, W, H, s = LABEL_CASE
    img = NL.image(c, W, H, s)
    sweep(monkeypatch, witness, 16 * W * H + 8192, lambda _: capi().label_map(img, s))


# ---- the image store --------------------------------------------------------------------------------------------------------------
def test_image_store_put(monkeypatch, witness):
    W, H = 40, 24
    img = smooth_image(W, H, 9)
    monkeypatch.delenv(VAR, raising=False)
    fresh = capi().ImageStore()
    fresh.put(7, img)
    want = fresh.level(7, 20, 12)
    fresh.close()
    ts = thresholds(W * H)     # the image's bytes
    for t in ts:
        st = capi().ImageStore()
        try:
            monkeypatch.setenv(VAR, str(t))
            try:
                st.put(7, img)
                error = None
            except capi().DvpError as e:
                error = str(e)
            monkeypatch.delenv(VAR)
            if error is None:
                assert t > W * H, t
            else:
                assert REFUSED in error and t <= W * H, (t, error)
                # the id is not in the store, and can be put again
                with pytest.raises(capi().DvpError, match="not in the store"):
                    st.size(7)
                assert st.bytes() == 0
                st.put(7, img)
                no_sticky_status(witness)
            assert st.size(7) == (W, H) and st.bytes() == W * H
            assert same(st.level(7, 20, 12), want), t
        finally:
            monkeypatch.delenv(VAR, raising=False)
            st.close()


def test_image_store_level(monkeypatch, witness):
    W, H = 40, 24
    img = smooth_image(W, H, 9)

    def store():
        st = capi().ImageStore()
        st.put(7, img)
        return st

    def still_stored(st):
        assert st.size(7) == (W, H) and st.bytes() == W * H

    sweep(monkeypatch, witness, 4 * W * H, lambda st: st.level(7, 20, 12), make=store, close=lambda st: st.close(), refused_state=still_stored)


# ---- the engine's contexts --------------------------------------------------------------------------------------------------------
def test_plane_prior(monkeypatch, witness):
    case = NP.case(0)
    cams = np.zeros(2, synth.CAMERA_DTYPE)
    cams[:] = NP.camera()

    def context():
        c = capi().Context(case["W"], case["H"], 2)
        c.set_cameras(cams)
        return c

    def prior(c):
        status = c.plane_prior(case["raw"], case["xy"], case["xyz"], NP.camera())
        c.synchronize()
        return status, c.get("planes")

    def refused(c):
        with pytest.raises(capi().DvpError, match="no dvp_plane_prior with status 0"):
            c.plane_prior_stage(capi().PRIOR_STAGE_OWNER)
        c.synchronize()

    # 12 bytes per dep-map pixel, 4 per working pixel, the triangle list and a float per sweep row
    rows = NP.expected(0)[3]["rows"]
    sweep(monkeypatch, witness, 16 * case["raw"].size + 4 * case["W"] * case["H"] + 4 * rows + 65536, prior, make=context, close=lambda c: c.close(), refused_state=refused)


def test_edge_map_begin(monkeypatch, witness):
    def edge_map(g):
        g.edge_map_begin(True)
        out = g.edge_map_finish()
        g.synchronize()
        return out, g.get("edge")

    sweep(monkeypatch, witness, 8 * 96 * 64 + 4096, edge_map, make=small_context, close=lambda g: g.close(), refused_state=lambda g: g.synchronize())


def test_preview_begin(monkeypatch, witness):
    W, H = 96, 64
    rs = np.random.RandomState(4)
    planes = np.ascontiguousarray(np.concatenate([rs.randn(H * W, 3), rs.uniform(1.0, 8.0, (H * W, 1))], 1).astype(np.float32))
    weak = rs.randint(0, 3, H * W).astype(np.uint8)
    kinds = dict(depth=capi().PREVIEW_DEPTH, normal=capi().PREVIEW_NORMAL, weak=capi().PREVIEW_WEAK)

    def context():
        g = small_context(W, H)
        g.upload_state(planes=planes, weak=weak)
        return g

    def previews(g):
        g.preview_begin(capi().PREVIEW_DEPTH | capi().PREVIEW_NORMAL | capi().PREVIEW_WEAK, 90)
        out = [g.preview_finish(v) for v in kinds.values()]
        g.synchronize()
        return out

    largest = max(int(capi().lib().dvp_jpeg_bound(W, H, 3)), 65536)
    sweep(monkeypatch, witness, largest, previews, make=context, close=lambda g: g.close(), refused_state=lambda g: g.synchronize())


# ---- fusion -------------------------------------------------------------------------------------------------------------------------
def fuse_lib():
    L = capi().lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.dvp_fuse_create.argtypes = [ci, ci, ctypes.POINTER(vp)]
    L.dvp_fuse_destroy.argtypes = [vp]
    L.dvp_fuse_last_error.restype, L.dvp_fuse_last_error.argtypes = ctypes.c_char_p, [vp]
    L.dvp_fuse_set_view.argtypes = [vp, ci, vp, ci, ci, vp, vp, vp, vp, vp]
    L.dvp_fuse_view.argtypes = [vp, ci, vp, ci]
    L.dvp_fuse_view_graded.argtypes = [vp, ci, vp, ci, ci]
    L.dvp_fuse_count.restype, L.dvp_fuse_count.argtypes = ctypes.c_longlong, [vp]
    L.dvp_fuse_download.argtypes = [vp, vp]
    return L


class FuseJob:
    """a dvp_fuse job over three views of 40 x 30 pixels with true depth maps — the size of test_gpu_fusion_abi's smallest scene, with
    a third view, so that the graded kinds, which need two agreeing sources, keep points and ask for the points' block.
    set_views() and fuse() go on where the last call stopped: after a refused call they begin with the slot / the view refused"""
    W, H, NV = 40, 30, 3

    def __init__(self):
        self.L = fuse_lib()
        sc = synth.make_scene(self.W, self.H, self.NV - 1)
        self.cams = np.ascontiguousarray(sc["cameras"])
        self.dep = [np.ascontiguousarray(sc["depth_gt"][v], np.float32) for v in range(self.NV)]
        self.nrm = np.ascontiguousarray(np.tile(sc["normal_gt"].astype(np.float32), (self.H, self.W, 1)))
        self.bgr = np.ascontiguousarray((np.arange(self.H * self.W * 3) % 251).astype(np.uint8).reshape(self.H, self.W, 3))
        self.job = ctypes.c_void_p()
        assert self.L.dvp_fuse_create(0, self.NV, ctypes.byref(self.job)) == 0
        self.next_slot = self.next_view = 0

    def ck(self, rc):
        if rc != 0:
            raise capi().DvpError(self.L.dvp_fuse_last_error(self.job).decode())

    def set_views(self):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        while self.next_slot < self.NV:
            v = self.next_slot
            self.ck(self.L.dvp_fuse_set_view(self.job, v, ctypes.c_void_p(self.cams.ctypes.data + 112 * v), self.W, self.H, p(self.dep[v]), p(self.nrm), None, p(self.bgr), None))
            self.next_slot += 1
        return self

    def fuse_view(self, v, graded):
        src = np.array([s for s in range(self.NV) if s != v], np.int32)
        p = src.ctypes.data_as(ctypes.c_void_p)
        return self.L.dvp_fuse_view(self.job, v, p, len(src)) if graded is None else self.L.dvp_fuse_view_graded(self.job, v, p, len(src), graded)

    def fuse(self, graded=None):
        """every view against the two others, then the cloud; graded: None, 0 (intermediate) or 1 (advanced)"""
        while self.next_view < self.NV:
            self.ck(self.fuse_view(self.next_view, graded))
            self.next_view += 1
        pts = np.zeros((self.L.dvp_fuse_count(self.job), 6), np.float32)
        self.ck(self.L.dvp_fuse_download(self.job, pts.ctypes.data_as(ctypes.c_void_p)))
        return pts

    def close(self):
        if self.job:
            assert self.L.dvp_fuse_destroy(self.job) == 0
            self.job = None


# the largest blocks: 12 bytes per pixel for a view's normals, 4 per pixel and source in the candidate arrays, 24 per point
FUSE_LARGEST = 24 * FuseJob.W * FuseJob.H


def test_fuse_set_view(monkeypatch, witness):
    sizes = sorted({k * FuseJob.W * FuseJob.H for k in (1, 3, 4, 8, 12)})     # the blocks of a view: claims, colours, depths, the two witness words, normals

    def refused_slot_is_unset(job):
        if job.next_slot < FuseJob.NV:      # (else the views were set and the fusion was refused)
            assert job.fuse_view(job.next_slot, None) != 0 and b"bad arguments" in job.L.dvp_fuse_last_error(job.job)

    # what comes after a refused slot: the slot set again (on the same job), the later slots, the fusion
    n = sweep(monkeypatch, witness, FUSE_LARGEST, lambda job: job.set_views().fuse(), make=FuseJob, close=lambda job: job.close(), refused_state=refused_slot_is_unset)
    # a threshold between two of a view's block sizes refuses a later block after an earlier one was granted
    assert n > len([t for t in thresholds(FUSE_LARGEST) if t <= sizes[0]])


@pytest.mark.parametrize("graded", [None, 0, 1], ids=["fuse_view", "graded_intermediate", "graded_advanced"])
def test_fuse_view(monkeypatch, witness, graded):
    def points_so_far_are_whole(job):
        # a refused call added nothing: the cloud holds the views before it
        assert job.next_view < FuseJob.NV
    fresh = FuseJob().set_views()
    assert len(fresh.fuse(graded)) > 0          # the points' block is asked for
    fresh.close()
    sweep(monkeypatch, witness, FUSE_LARGEST, lambda job: job.fuse(graded), make=lambda: FuseJob().set_views(), close=lambda job: job.close(),
          refused_state=points_so_far_are_whole)
