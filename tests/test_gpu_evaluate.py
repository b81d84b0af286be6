"""`apd --evaluate` on the device (csrc/dvp_cloudeval.hip): dvp_cloud_distances and dvp_cloud_evaluate equal the same text run
serially on the host (tests/cloudeval_host) bit for bit on d2 and exactly on the counts, in both query forms, on the smallest shapes
at which the kernels can go wrong - the case table of tests/np_evaluate.py: one point, no points, a target at exactly T and one ulp
beyond, two cells away, 63 / 64 / 65 / 129 targets or queries in one cell (the LDS chunks, the ragged last wave), the nearest target
in each of the 26 neighbour cells, 6 000 occupied cells in a table of the smallest capacity with shared home slots, identical
targets, negative coordinates, coordinates near 1e4 at T = 0.01, NaN and infinities, ragged query counts - and on 20 000 targets in a
3 x 3 x 3 block of cells, run twice; the extent limit and the argument checks with their messages; two threads at once."""
import ctypes
import threading

import numpy as np
import pytest

import np_evaluate as N
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = N.cases()
_REFERENCE = {}


def capi():
    return pkg().get_capi()


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> the serial text's result, made once"""
    N.build_program()
    scenes = dict(CASES, contention=N.contention_scene(), random=N.random_scene(5))

    def get(name):
        if name not in _REFERENCE:
            recon, truth, tol = scenes[name]
            rc, err, want = N.serial(recon, truth, tol, tmp_path_factory.mktemp(name), "grid")
            assert rc == 0, err
            for v in want.values():
                v.setflags(write=False)
            _REFERENCE[name] = (recon, truth, tol, want)
        return _REFERENCE[name]
    return get


def device(recon, truth, tol):
    return capi().cloud_evaluate(recon, truth, tol, distances=True)


@pytest.mark.parametrize("form", ["wave", "lane"])
@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_the_serial_text(reference, monkeypatch, case, form):
    monkeypatch.setenv("DVP_CLOUD_QUERY", form)
    recon, truth, tol, want = reference(case)
    assert N.same_result(device(recon, truth, tol), want) == ""
    assert N.same_bits(capi().cloud_distances(recon, truth, tol[-1]), want["d2_recon"])
    assert N.same_bits(capi().cloud_distances(truth, recon, tol[-1]), want["d2_truth"])


@pytest.mark.parametrize("form", ["wave", "lane"])
def test_contention_on_the_table_and_the_cursors(reference, monkeypatch, form):
    monkeypatch.setenv("DVP_CLOUD_QUERY", form)
    recon, truth, tol, want = reference("contention")
    assert 0 < want["within_recon"][0] < want["within_recon"][1] <= 5000
    for _ in range(2):      # min and integer sums: the same result whatever the order
        assert N.same_result(device(recon, truth, tol), want) == ""


def test_random_clouds(reference):
    recon, truth, tol, want = reference("random")
    assert N.same_result(device(recon, truth, tol), want) == ""
    got = capi().cloud_evaluate(recon, truth, tol)      # without the distances
    assert "d2_recon" not in got and N.same_result(got, want) == ""
    a, c = want["within_recon"] / 4000, want["within_truth"] / 4000
    assert np.array_equal(got["accuracy"], a) and np.array_equal(got["completeness"], c) and np.allclose(got["f1"], 2 * a * c / (a + c), rtol=1e-15)


def test_query_form_is_checked(monkeypatch):
    monkeypatch.setenv("DVP_CLOUD_QUERY", "warp")
    with pytest.raises(capi().DvpError, match="DVP_CLOUD_QUERY takes wave or lane"):
        device(N.cloud([[0, 0, 0]]), N.cloud([[0, 0, 0]]), [0.1])


def test_extent_limit():
    C = capi()
    a, far = N.cloud([[0, 0, 0], [1, 1, 1]]), N.cloud([[0, 0, 0], [0, 30000, 0]])
    with pytest.raises(C.DvpError, match=r"dvp_cloud_evaluate: the clouds extend over 30000 along axis 1, which is \d+ cells of the largest tolerance 0.00999999978; at most 2097150"):
        C.cloud_evaluate(a, far, [0.005, 0.01])
    with pytest.raises(C.DvpError, match=r"dvp_cloud_distances: the clouds extend over 30000 along axis 1"):
        C.cloud_distances(a, far, 0.01)
    # just inside: 2 097 150 cells of edge 0.5 (1 + 2^-10) along x
    edge = N.cloud([[0, 0, 0], [0.5 * (1 + 2.0 ** -10) * 2097149.5, 0, 0]])
    got = C.cloud_evaluate(edge, edge, [0.5], distances=True)
    assert got["d2_recon"].tolist() == [0.0, 0.0] and got["within_recon"].tolist() == [2]
    with pytest.raises(C.DvpError, match="2097151 cells"):
        C.cloud_evaluate(N.cloud([[0, 0, 0], [0.5 * (1 + 2.0 ** -10) * 2097150.5, 0, 0]]), edge, [0.5])


def test_argument_checks(monkeypatch):
    C = capi()
    L = C.lib()
    pts = N.cloud(np.random.default_rng(1).random((5, 3)))
    out, tol = np.zeros(5, np.float32), np.array([0.1, 0.2], np.float32)
    w, used = np.zeros(8, np.int64), np.zeros(2, np.int64)
    f = ctypes.c_float

    def last():
        return L.dvp_cloud_last_error().decode()

    assert L.dvp_cloud_distances(0, None, 5, C._p(pts), 5, f(0.1), C._p(out)) != 0 and last() == "dvp_cloud_distances: the point arrays are required"
    assert L.dvp_cloud_distances(0, C._p(pts), 5, None, 5, f(0.1), C._p(out)) != 0 and last() == "dvp_cloud_distances: the point arrays are required"
    assert L.dvp_cloud_distances(0, C._p(pts), 5, C._p(pts), 5, f(0.1), None) != 0 and last() == "dvp_cloud_distances: d2_out is required"
    assert L.dvp_cloud_distances(0, C._p(pts), -1, C._p(pts), 5, f(0.1), C._p(out)) != 0 and "a cloud holds 0 ... 2^31 - 1 points, got -1" in last()
    assert L.dvp_cloud_distances(0, C._p(pts), 5, C._p(pts), 2 ** 31, f(0.1), C._p(out)) != 0 and "a cloud holds 0 ... 2^31 - 1 points, got 2147483648" in last()
    for bad in (0.0, -0.1, float("nan"), float("inf"), 1e-30, 1e30):
        assert L.dvp_cloud_distances(0, C._p(pts), 5, C._p(pts), 5, f(bad), C._p(out)) != 0 and last().startswith("dvp_cloud_distances: tolerance 0 (") and "must be finite and positive" in last()
    assert L.dvp_cloud_evaluate(0, C._p(pts), 5, C._p(pts), 5, C._p(tol), 2, None, C._p(w), C._p(used), None, None) != 0 and last() == "dvp_cloud_evaluate: within_recon, within_truth and used are required"
    assert L.dvp_cloud_evaluate(0, C._p(pts), 5, C._p(pts), 5, C._p(tol), 2, C._p(w), C._p(w), None, None, None) != 0 and "are required" in last()
    assert L.dvp_cloud_evaluate(0, C._p(pts), 5, C._p(pts), 5, None, 2, C._p(w), C._p(w), C._p(used), None, None) != 0 and last() == "dvp_cloud_evaluate: the tolerances are required"
    for n in (0, 9, -1):
        assert L.dvp_cloud_evaluate(0, C._p(pts), 5, C._p(pts), 5, C._p(np.linspace(0.1, 0.9, 9).astype(np.float32)), n, C._p(w), C._p(w), C._p(used), None, None) != 0
        assert last() == "dvp_cloud_evaluate: num_tol must be 1 ... 8, got %d" % n
    with pytest.raises(C.DvpError, match="dvp_cloud_evaluate: the tolerances must be strictly ascending, 0.100000001 follows 0.100000001"):
        C.cloud_evaluate(pts, pts, [0.1, 0.1])
    with pytest.raises(C.DvpError, match=r"dvp_cloud_evaluate: tolerance 1 \(nan\) must be finite and positive"):
        C.cloud_evaluate(pts, pts, [0.1, float("nan")])
    with pytest.raises(ValueError, match="a \\(N, 3\\) array"):
        C.cloud_evaluate(np.zeros((4, 2)), pts, [0.1])
    # out of device memory is an error, not a crash
    monkeypatch.setenv("DVP_TEST_SIDE_ALLOC_FAIL", "1")
    with pytest.raises(C.DvpError, match="dvp_cloud_evaluate: out of device memory"):
        C.cloud_evaluate(pts, pts, [0.1])
    monkeypatch.delenv("DVP_TEST_SIDE_ALLOC_FAIL")
    # an error leaves the next call alone
    got = C.cloud_evaluate(pts, pts, [0.1], distances=True)
    assert got["within_recon"].tolist() == [5] and got["used"].tolist() == [5, 5] and not got["d2_truth"].any() and last() == ""


def test_two_threads_evaluate_at_once(reference):
    jobs = [reference("ragged_1000_777"), reference("table")]
    bad = []

    def work(k):
        try:
            recon, truth, tol, want = jobs[k]
            for _ in range(3):
                what = N.same_result(device(recon, truth, tol), want)
                if what:
                    bad.append((k, what))
                if not N.same_bits(capi().cloud_distances(truth, recon, tol[-1]), want["d2_truth"]):
                    bad.append((k, "distances"))
        except Exception as e:      # noqa: BLE001
            bad.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad
