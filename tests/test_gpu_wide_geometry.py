"""Wide-baseline and degenerate-hypothesis geometry on the GPU: the HIP engine through the C ABI against the CPU oracle, bit for
bit, on the classes and the state of tests/wide_geometry.py.  Every other GPU parity test draws its cameras from synth.make_rig,
where the projective denominator of every homography is 1 +- 0.1; here patches straddle a source camera's principal plane, taps
land 1e6 pixels outside or at inf / NaN coordinates, forward points lie behind a source camera and plane records are degenerate —
the operands at which the device-only branches of dvp_dev.hpp / dvp_wave.hpp (clampf_nan_lo, floor_to_int, the 24-bit multiplies of
the offsets, the binary16 converts, the uniform loads) could differ from the host text that tests/emul runs.
tests/test_wide_geometry_host.py holds the CPU twin of every test here: a failure here next to a green twin points at such a
branch.  All at 96 x 64, the smallest size at which the rig keeps the epipole and all six sources in view."""
import pytest

from conftest import pkg
from oracle import oracle as O
import test_wide_geometry_host as T

pytestmark = pytest.mark.gpu


def capi():
    return pkg("capi")


def _pair(scene, params, state, seed=1234, sampler=0, depths=None):
    a = O.from_scene(scene, params, seed=seed, sampler=sampler, depths=depths)
    b = capi().from_scene(scene, params, seed=seed, sampler=sampler, depths=depths)
    a.upload_state(**state)
    b.upload_state(**state)
    return a, b


@pytest.mark.parametrize("sampler", [0, 1])
@pytest.mark.parametrize("name", ["C0", "C1", "C2", "C4"])
def test_cost_vectors_kat(name, sampler):
    """dvp_eval_cost_vectors == the oracle on 4096 members of a class, all six views of each; C1: every member is evaluated in the
    forward camera (as many costs below 2 as the classifier counted)"""
    T.kat_case(_pair, name, sampler)


@pytest.mark.parametrize("sampler", [0, 1])
def test_first_pass_stage_by_stage(sampler):
    """FIRST_INIT from first_pass_state: random planes over the depth range [0.3, 60], every CHECKED buffer after every stage"""
    T.first_pass_case(_pair, T.run_and_compare, sampler)


@pytest.mark.parametrize("images", ["int", "box", "scaled"])
def test_refine_pass_stage_by_stage(images, monkeypatch):
    """REFINE_ITER with the geometric term on arbitrary_state + the shallow C3 planes in a 16 x 16 block, on byte tiles, binary16
    tiles and float planes (formats 1, 2, 0): every CHECKED buffer after every stage"""
    T.refine_pass_case(_pair, T.run_and_compare, images, monkeypatch)


@pytest.mark.parametrize("form", list(T.FORMS))
def test_forms_in_the_regime(form, monkeypatch):
    """dvp_run_patchmatch of that pass with each launch site in its other forms (T.FORMS) == one shared oracle run.  The case pins
    the environment and asserts what the launch-site rule decides under it (strong, weak and sweep kernel, runs and groups);
    the strong update's form is also read back from the engine (the C ABI reports no other)."""
    g = T.forms_case(lambda sc, p, depths: capi().from_scene(sc, p, depths=depths), form, monkeypatch)
    # the strong update really took the form asked for: the decision bracket of S = 5, the streaming kernel, or a monolithic kernel
    assert g.strong_update_form() == {"strong_monolithic": 0, "strong_streaming_decide": 32}.get(form, 6)
    assert g.weak_count() > 700 and g.timings()["stage_launches"]["weak_update"] > 0
