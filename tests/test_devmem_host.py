"""The owner of the side stages' device memory (csrc/dvp_devmem.hpp) without a GPU: tests/devmem_host builds the header for the
host — no HIP header, a counting stand-in for the allocator that refuses the k-th request or every request above a size — into a
stand-alone program under the address and undefined-behaviour sanitizers.  It checks that a block only grows, that a refused
request leaves it empty and frees the old block exactly once, that a move leaves the source empty, that nothing is live at the
end of a scenario, and that Carve lays a pool out as labels_reserve and dvpprior::reserve did with their own take(): here for the
geometries of np_labels.SIZES x SCALES and the np_prior cases with their real triangle and sweep-row counts."""
import os
import subprocess

import pytest

import np_labels as NL
import np_prior as NP

pytestmark = pytest.mark.hostbox

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devmem_host")


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", _HERE])
    return os.path.join(_HERE, "devmem_host")


def _run(exe, *args):
    env = {k: v for k, v in os.environ.items() if k != "DVP_TEST_SIDE_ALLOC_FAIL"}
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("checks ok"), r.stdout + r.stderr
    return int(r.stdout.split()[-3])


def test_block_scenarios_and_built_in_layouts(exe):
    assert _run(exe) > 1000


def test_carve_equals_the_label_pools_own_arithmetic(exe):
    args = []
    for (W, H) in NL.SIZES:
        for s in NL.SCALES:
            args += ["labels", W, H, s]
    assert _run(exe, *args) > _run(exe)


def test_carve_equals_the_prior_pools_own_arithmetic(exe):
    args = []
    for k in range(len(NP.CASES)):
        c = NP.case(k)
        middle, tris, skipped, want = NP.expected(k)
        rows, cols = c["raw"].shape
        args += ["prior", cols, rows, c["W"], c["H"], len(tris), want["rows"]]
    assert _run(exe, *args) > _run(exe)


def test_a_malformed_request_is_refused(exe):
    r = subprocess.run([exe, "labels", "12"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout
