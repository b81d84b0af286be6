"""The plane-cache plan of the split strong update (dvp_strong.hpp: strong_reuse_plan, what dvp_strong_plan runs per pixel) on the
host: tests/reuse_host builds it with g++ into a stand-alone program that draws seeded random old records (0-17 valid places,
matching and stale epoch / radius) and new slot sets (missing slots, repeated planes, planes that differ only in the sign of a
zero or in a NaN payload) and checks, against a brute-force model: (a) every present slot ends at a place whose key is its plane's
bits, (b) a plane of a live record is not evaluated and keeps its place, (c) the evaluation mask holds exactly one slot per
distinct plane that missed, (d) distinct planes never share a place, (e) a stale epoch or radius makes the mask equal to `uniq`.
The same program built with -fsanitize=address,undefined runs as a plain executable."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.hostbox

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reuse_host")


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", _HERE])
    return _HERE


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout
    return r.stdout


def test_plan_properties_on_random_records(built):
    out = _run(os.path.join(built, "reuse_host"), 300000)
    assert "300000 cases ok" in out


def test_plan_properties_with_another_seed(built):
    _run(os.path.join(built, "reuse_host"), 200000, "0x1234567")


def test_plan_under_address_and_undefined_behaviour_sanitizers(built):
    out = _run(os.path.join(built, "reuse_host_san"), 300000)
    assert "300000 cases ok" in out
