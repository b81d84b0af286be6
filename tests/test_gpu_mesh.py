"""The mesher on the device: dvp_mesh_build equals the serial text of csrc/dvp_mesh.hpp (tests/mesh_host) bit for bit at every stage
the ABI hands out - block keys, SF, W, colour sums, vertices, colours, faces - over the case table of tests/np_mesh.py (the serial text
has no cull: a view culled wrongly for a block shows in SF and W); a table that starts with 4 slots regrows to the same mesh, with
general cameras and past 512 blocks too; two threads build at once, a general camera among them; out of device memory is an error or
changes nothing; the refusals carry their messages."""
import ctypes
import os
import threading

import numpy as np
import pytest

import np_mesh as M
from conftest import pkg

pytestmark = pytest.mark.gpu

CASES = M.cases()


@pytest.fixture(scope="module", autouse=True)
def built():
    M.build_program()


@pytest.fixture(scope="module")
def capi():
    return pkg("capi")


@pytest.fixture(scope="module")
def serial_of(tmp_path_factory):
    done = {}

    def get(name):
        if name not in done:
            c = CASES[name]
            rc, err, got = M.serial(c["views"], c["s"], c["tau"], c["min_weight"], tmp_path_factory.mktemp(name))
            assert rc == 0, err
            done[name] = got
        return done[name]
    return get


def device(capi, c, **kw):
    return capi.mesh_build(c["views"], c["s"], c["tau"], c["min_weight"], table_slots=c["table"], volume=True, **kw)


@pytest.mark.parametrize("case", list(CASES))
def test_every_stage_equals_the_serial_text(capi, serial_of, case):
    got = device(capi, CASES[case])
    assert M.same(got, serial_of(case)) == ""
    assert got["blocks"] == len(serial_of(case)["keys"])


def test_a_table_of_four_slots_regrows_to_the_same_mesh(capi, serial_of):
    c = CASES["table_regrows"]
    small = device(capi, c, timings=True)
    roomy = capi.mesh_build(c["views"], c["s"], c["tau"], c["min_weight"], table_slots=1 << 16, volume=True, timings=True)
    assert small["regrows"] >= 4 and roomy["regrows"] == 0
    assert M.same(small, roomy) == "" and M.same(small, serial_of("table_regrows")) == ""


@pytest.mark.parametrize("case", ["oblique_sphere", "blocks_513"])
def test_general_cameras_and_a_second_scan_chunk_regrow_to_the_same_mesh(capi, serial_of, case):
    """(blocks_513: 4 slots double eight times before 513 blocks fill at most half of them)"""
    c = CASES[case]
    small = capi.mesh_build(c["views"], c["s"], c["tau"], c["min_weight"], table_slots=4, volume=True, timings=True)
    roomy = capi.mesh_build(c["views"], c["s"], c["tau"], c["min_weight"], table_slots=1 << 16, volume=True, timings=True)
    assert small["regrows"] >= 4 and roomy["regrows"] == 0
    assert M.same(small, roomy) == "" and M.same(small, serial_of(case)) == ""


def test_two_threads_build_at_once(capi, serial_of):
    names, got = ["sphere", "sphere_at_origin", "oblique_sphere"], {}

    def work(name):
        try:
            got[name] = [device(capi, CASES[name]) for _ in range(3)]
        except Exception as e:   # (reported by the assertions below)
            got[name] = e
    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for n in names:
        assert not isinstance(got[n], Exception), got[n]
        for g in got[n]:
            assert M.same(g, serial_of(n)) == ""


def test_out_of_device_memory_is_an_error_or_changes_nothing(capi, serial_of, monkeypatch):
    c = CASES["sphere"]
    refused = 0
    for power in range(0, 27):
        monkeypatch.setenv("DVP_TEST_SIDE_ALLOC_FAIL", str(1 << power))
        try:
            got = device(capi, c)
        except capi.DvpError as e:
            assert "out of device memory" in str(e), str(e)
            refused += 1
            continue
        assert M.same(got, serial_of("sphere")) == ""
    monkeypatch.delenv("DVP_TEST_SIDE_ALLOC_FAIL")
    assert refused >= 10
    assert M.same(device(capi, c), serial_of("sphere")) == ""


def test_refusals_carry_their_messages(capi):
    L = capi.lib()
    err = lambda: L.dvp_mesh_last_error().decode()
    job = ctypes.c_void_p()
    assert L.dvp_mesh_create(0, 0.05, 0.2, 1, None) != 0 and "the job pointer is required" in err()
    for s, tau, mw, message in ((0.0, 1.0, 1, "the voxel edge must be finite and positive"), (float("nan"), 1.0, 1, "the voxel edge must be finite and positive"),
                                (float("inf"), float("inf"), 1, "the voxel edge must be finite and positive"), (-1.0, 1.0, 1, "the voxel edge must be finite and positive"),
                                (0.05, 0.04, 1, "must be finite and at least the voxel edge"), (0.05, float("inf"), 1, "must be finite and at least the voxel edge"),
                                (0.05, 3.3, 1, "spans more than 64 voxels"), (0.05, 0.2, 0, "min_weight must be at least 1")):
        assert L.dvp_mesh_create(0, s, tau, mw, ctypes.byref(job)) != 0 and message in err() and not job.value, (s, tau, mw, err())
    assert L.dvp_mesh_build(None) != 0 and "the job is required" in err()
    assert L.dvp_mesh_download(None, None, None, None) != 0 and "a built job is required" in err()
    assert L.dvp_mesh_block_count(None) == -1 and L.dvp_mesh_destroy(None) == 0
    cam, depth, mask, bgr = CASES["plane_one_view"]["views"][0]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    c = np.ascontiguousarray(cam).reshape(1)
    assert L.dvp_mesh_create(0, 0.05, 0.2, 1, ctypes.byref(job)) == 0
    try:
        for args in ((None, p(depth), p(mask), p(bgr)), (p(c), None, p(mask), p(bgr)), (p(c), p(depth), None, p(bgr)), (p(c), p(depth), p(mask), None)):
            assert L.dvp_mesh_add_view(job, args[0], 24, 24, *args[1:]) != 0 and "are required" in err()
        assert L.dvp_mesh_add_view(None, p(c), 24, 24, p(depth), p(mask), p(bgr)) != 0 and "are required" in err()
        assert L.dvp_mesh_add_view(job, p(c), 0, 24, p(depth), p(mask), p(bgr)) != 0 and "a view has 1 ... 2^31 - 1 pixels" in err()
        assert L.dvp_mesh_download(job, None, None, None) != 0 and "a built job is required" in err()
        assert L.dvp_mesh_vertex_count(job) == -1
        for slots in (0, 3, 6, 1 << 33):
            assert L.dvp_mesh_set_table(job, slots) != 0 and "a power of two from 4 to 2^32" in err()
        assert L.dvp_mesh_add_view(job, p(c), 24, 24, p(depth), p(mask), p(bgr)) == 0
        assert L.dvp_mesh_build(job) == 0 and L.dvp_mesh_vertex_count(job) == 64
        assert L.dvp_mesh_download(job, None, None, None) != 0 and "the vertex, colour and face arrays are required" in err()
    finally:
        assert L.dvp_mesh_destroy(job) == 0
    with pytest.raises(capi.DvpError, match=r"a lattice index beyond 21 bits \(view 0\)"):
        capi.mesh_build(CASES["plane_one_view"]["views"], 1e-7, 4e-7, 1)
    wild = depth.copy()
    wild[3, 4] = np.inf
    with pytest.raises(capi.DvpError, match=r"a lattice index beyond 21 bits \(view 1\)"):
        capi.mesh_build([(cam, depth, mask, bgr), (cam, wild, mask, bgr)], 0.05, 0.2, 1)


def test_a_job_takes_more_views_and_builds_again(capi, tmp_path):
    """(the driver adds every view before it builds; the ABI allows more)"""
    c = CASES["two_views_disagree"]
    L = capi.lib()
    job = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.dvp_mesh_create(0, c["s"], c["tau"], 1, ctypes.byref(job)) == 0
    try:
        counts = []
        for cam, depth, mask, bgr in c["views"]:
            assert L.dvp_mesh_add_view(job, p(np.ascontiguousarray(cam).reshape(1)), 24, 24, p(depth), p(mask), p(bgr)) == 0
            assert L.dvp_mesh_build(job) == 0, L.dvp_mesh_last_error()
            counts.append((L.dvp_mesh_block_count(job), L.dvp_mesh_vertex_count(job), L.dvp_mesh_face_count(job)))
        v, col, f = np.empty((counts[1][1], 3), np.float32), np.empty((counts[1][1], 3), np.uint8), np.empty((counts[1][2], 3), np.int32)
        assert L.dvp_mesh_download(job, p(v), p(col), p(f)) == 0
    finally:
        L.dvp_mesh_destroy(job)
    rc, err, one = M.serial(c["views"][:1], c["s"], c["tau"], 1, tmp_path)
    assert rc == 0 and counts[0] == (len(one["keys"]), len(one["vertices"]), len(one["faces"]))
    rc, err, two = M.serial(c["views"], c["s"], c["tau"], 1, tmp_path)
    assert rc == 0 and v.tobytes() == two["vertices"].tobytes() and col.tobytes() == two["colours"].tobytes() and f.tobytes() == two["faces"].tobytes()
