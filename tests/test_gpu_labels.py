"""The label prior on the device (csrc/dvp_labels.hip) through the C ABI: dvp_label_map, and dvp_labels_run + dvp_labels_stage on a
job, on the cases of test_labels_host.py, against the host mirror's LabelSegment with its intermediate maps — exact, every
value of every map.  Then: one job across sizes that grow and shrink, two jobs on two threads, the argument checks, a
1552 x 1032 image and one corridor of more than 100 k level pixels."""
import ctypes
import threading

import numpy as np
import pytest

import np_labels as N
from conftest import pkg

pytestmark = pytest.mark.gpu


def capi():
    return pkg().get_capi()


def job_maps(job, img, scale):
    out = dict(labels=job.run(img, scale))
    for n in N.STAGES + ("region",):
        out[n] = job.stage(n)
    return out


@pytest.fixture(scope="module")
def job():
    j = capi().LabelJob()
    yield j
    j.close()


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_every_stage_equals_the_host_mirror(case, job):
    content, W, H, scale = case
    img = N.image(content, W, H, scale)
    want = N.expected(case)
    N.check_against_mirror(job_maps(job, img, scale), want, N.sizes(W, H, scale)["weak_tex_num"])
    one_shot = capi().label_map(img, scale)
    assert np.array_equal(one_shot, want["labels"]), int((one_shot != want["labels"]).sum())


def test_sizes_call_agrees_with_the_host():
    for (W, H) in N.SIZES:
        for s in N.SCALES:
            got, want = capi().labels_sizes(W, H, s), N.sizes(W, H, s)
            assert (got["quarter"], got["level"], got["weak_tex_num"]) == (want["quarter"], want["level"], want["weak_tex_num"])


def test_pitch_is_honoured():
    wide = np.zeros((65, 80), np.uint8)
    wide[:, :63] = N.image("picture", 63, 65, 1)
    assert np.array_equal(capi().label_map(wide[:, :63], 1), N.expected(("picture", 63, 65, 1))["labels"])


def test_one_job_across_sizes_equals_fresh_jobs():
    """the scratch grows, is kept, and serves a smaller image after a larger one"""
    order = [("picture", 130, 70, 1), ("serpentine", 515, 259, 0), ("frame", 63, 65, 2), ("picture", 480, 360, 0), ("picture", 130, 70, 1)]
    j = capi().LabelJob()
    for case in order:
        content, W, H, scale = case
        img = N.image(content, W, H, scale)
        kept = job_maps(j, img, scale)
        fresh_job = capi().LabelJob()
        fresh = job_maps(fresh_job, img, scale)
        fresh_job.close()
        for n in kept:
            assert np.array_equal(kept[n], fresh[n]), (case, n)
        N.check_against_mirror(kept, N.expected(case), N.sizes(W, H, scale)["weak_tex_num"])
    j.close()


def test_two_jobs_from_two_threads_equal_serial_runs():
    cases = [("spiral", 480, 360, 0), ("picture", 515, 259, 1)]
    got, errors = {}, []
    capi().lib()

    def work(k):
        try:
            j = capi().LabelJob()
            content, W, H, scale = cases[k]
            for _ in range(4):
                got[k] = job_maps(j, N.image(content, W, H, scale), scale)
            j.close()
        except Exception as e:      # noqa: BLE001 (reported below, on the test's thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, case in enumerate(cases):
        N.check_against_mirror(got[k], N.expected(case), N.sizes(case[1], case[2], case[3])["weak_tex_num"])


def test_bad_arguments_are_errors_with_a_message():
    L, C = capi().lib(), capi()
    img = np.zeros((40, 40), np.uint8)
    out = np.zeros((40, 40), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    assert L.dvp_labels_create(0, None) != 0 and b"required" in L.dvp_labels_last_error()
    assert L.dvp_labels_create(0, ctypes.byref(h)) == 0
    bad = [((h, None, 40, 40, 40, 0, p(out)), b"required"), ((h, p(img), 40, 40, 40, 0, None), b"required"), ((None, p(img), 40, 40, 40, 0, p(out)), b"required"),
           ((h, p(img), 40, 40, 40, -1, p(out)), b"scale"), ((h, p(img), 40, 40, 39, 0, p(out)), b"pitch"), ((h, p(img), 11, 40, 40, 0, p(out)), b"quarter-size"),
           ((h, p(img), 40, 11, 40, 0, p(out)), b"quarter-size"), ((h, p(img), 16, 16, 16, 3, p(out)), b"level-size"), ((h, p(img), 0, 40, 40, 0, p(out)), b"geometry")]
    for args, word in bad:
        assert L.dvp_labels_run(*args) != 0, args
        assert word in L.dvp_labels_last_error(), (args, L.dvp_labels_last_error())
    assert L.dvp_labels_stage(h, 0, p(out)) != 0 and b"no run" in L.dvp_labels_last_error()
    assert L.dvp_labels_run(h, p(img), 40, 40, 40, 0, p(out)) == 0 and L.dvp_labels_last_error() == b""
    assert L.dvp_labels_stage(h, 9, p(out)) != 0 and b"no such stage" in L.dvp_labels_last_error()
    assert L.dvp_labels_stage(h, 0, None) != 0 and b"required" in L.dvp_labels_last_error()
    assert L.dvp_labels_destroy(h) == 0
    assert L.dvp_label_map(0, p(img), 40, 40, 39, 0, p(out)) != 0 and b"pitch" in L.dvp_labels_last_error()
    with pytest.raises(C.DvpError, match="scale"):
        C.labels_sizes(40, 40, -1)


def _large_image(W, H):
    """flat walls with grain, textured bands and blocks, a ramp: large regions, small ones and lines at 1552 x 1032"""
    rs = np.random.RandomState(17)
    img = np.full((H, W), 90, np.uint8)
    img[:, W // 2:] = 170
    img[H // 3:H // 3 + 40, :] = rs.randint(0, 256, (40, W))
    img[:, W // 2 - 30:W // 2 + 30] = rs.randint(0, 256, (H, 60))
    for k in range(12):
        y, x = rs.randint(0, H - 120), rs.randint(0, W - 160)
        img[y:y + 120, x:x + 160] = rs.randint(0, 256, (120, 160))
        img[y + 30:y + 30 + 8 * (k + 1), x + 40:x + 40 + 10 * (k + 1)] = 30 + 15 * k      # flat islands of growing size inside the texture
    img += rs.randint(0, 2, (H, W)).astype(np.uint8)
    return img


@pytest.mark.parametrize("scale", [0, 1])
def test_1552x1032_equals_the_host_mirror(scale, job):
    W, H = 1552, 1032
    img = _large_image(W, H)
    want = N.mirror(img, scale)
    assert (want["labels"] > 0).any() and (want["labels"] == -1).any() and len(np.unique(want["labels"])) > 4
    assert (want["lines"] != want["texture"]).sum() > 0
    got = job_maps(job, img, scale)
    for n in N.STAGES + ("labels",):
        assert np.array_equal(got[n], want[n]), (n, int((got[n] != want[n]).sum()))


def test_long_corridor(job):
    """1023 x 515, scale 0: one flat corridor of more than 100 k level pixels through every tile row and column"""
    img = N.long_corridor()
    want = N.mirror(img, 0)
    lab, size = N.components(want["cleaned"] == 0)
    assert size[1:].max() >= 100000
    N.check_against_mirror(job_maps(job, img, 0), want, N.sizes(1023, 515, 0)["weak_tex_num"])
