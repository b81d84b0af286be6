"""dvp_plane_prior on the device against the numpy model of np_prior.py (the source's overwriting sweep, typed arithmetic): the
owner map, the rate map, the working-size metric depth (dvp_plane_prior_stage) and the context's planes, bitwise on all pixels
(NaN == NaN) of every case; status 1 and what it leaves alone; scratch that grows and is reused; the error before any camera
upload; and a FIRST_INIT pass that starts from the device's planes against one that starts from the model's."""
import numpy as np
import pytest

import np_prior as N
from conftest import pkg, synth

pytestmark = pytest.mark.gpu


def context(W, H, cam=None, num_images=2):
    capi = pkg().get_capi()
    c = capi.Context(W, H, num_images)
    cams = np.zeros(num_images, synth.CAMERA_DTYPE)
    cams[:] = N.camera() if cam is None else cam
    c.set_cameras(cams)
    return c


def check(c, k):
    capi = pkg().get_capi()
    case = N.case(k)
    middle, tris, skipped, want = N.expected(k)
    assert c.plane_prior(case["raw"], case["xy"], case["xyz"], N.camera()) == 0
    owner = c.plane_prior_stage(capi.PRIOR_STAGE_OWNER)
    assert np.array_equal(owner, want["owner"]), (N.CASES[k], "owner", int((owner != want["owner"]).sum()))
    got = dict(rate=c.plane_prior_stage(capi.PRIOR_STAGE_RATE), depth=c.plane_prior_stage(capi.PRIOR_STAGE_DEPTH),
               planes=c.get("planes").reshape(case["H"], case["W"], 4))
    for stage in ("rate", "depth", "planes"):
        assert N.same_bits(got[stage], want[stage]), (N.CASES[k], stage, N.differing(got[stage], want[stage]))
    t = c.plane_prior_timings()
    assert t["triangles"] == len(tris) and t["sweep_rows"] == want["rows"]


@pytest.mark.parametrize("k", range(len(N.CASES)), ids=N.CASES)
def test_every_stage_equals_the_model(k):
    case = N.case(k)
    c = context(case["W"], case["H"])
    check(c, k)
    c.close()


def test_status_1_leaves_the_planes_untouched():
    c = context(96, 72)
    before = np.random.default_rng(5).standard_normal((96 * 72, 4)).astype(np.float32)
    c.set("planes", before)
    for case in N.unusable_cases():
        assert c.plane_prior(case["raw"], case["xy"], case["xyz"], N.camera()) == 1, case["name"]
        assert N.same_bits(c.get("planes"), before), case["name"]
    with pytest.raises(pkg().get_capi().DvpError):       # nothing to read back: no run with status 0 has finished
        c.plane_prior_stage(0)
    c.close()


def test_one_context_a_larger_map_then_a_smaller_one():
    """the scratch grows for the larger map; the smaller one after it must not see the larger one's owners"""
    c = context(96, 72)
    for k in (0, 2, 1, 0):          # 96 x 72, 191 x 143, 200 x 100, 96 x 72 again
        assert (N.case(k)["W"], N.case(k)["H"]) == (96, 72)
        check(c, k)
    # ... and an unusable input in between leaves the last result readable and the planes as they are
    want = N.expected(0)[3]
    bad = N.unusable_cases()[0]
    assert c.plane_prior(bad["raw"], bad["xy"], bad["xyz"], N.camera()) == 1
    assert N.same_bits(c.get("planes").reshape(72, 96, 4), want["planes"])
    assert N.same_bits(c.plane_prior_stage(pkg().get_capi().PRIOR_STAGE_RATE), want["rate"])
    c.close()


def test_a_call_before_any_camera_upload_is_an_error():
    capi = pkg().get_capi()
    c = capi.Context(96, 72, 2)
    case = N.case(0)
    with pytest.raises(capi.DvpError, match="cameras"):
        c.plane_prior(case["raw"], case["xy"], case["xyz"], N.camera())
    c.close()


def test_first_init_pass_from_the_device_planes_equals_one_from_the_models():
    capi = pkg().get_capi()
    W, H, S = 96, 72, 3
    sc = synth.make_scene(W, H, S)
    cam = sc["cameras"][0]
    case = N.case(0)
    status, middle, tris, skipped = N.serial_triangles(case, cam)
    assert status == 0
    want = N.model(case["raw"], tris, middle, W, H, cam)["planes"].reshape(-1, 4)
    p = synth.default_params(S + 1, max_iterations=1, state=synth.FIRST_INIT, use_APD=0)
    p["depth_min"] = np.float32(2.5) * np.float32(0.6)
    p["depth_max"] = np.float32(6.5) * np.float32(1.2)
    inside = (want[:, 3] >= p["depth_min"]) & (want[:, 3] <= p["depth_max"])
    assert inside.mean() > 0.9          # the pass keeps the prior's planes (APD.cu:1289-1291): it does depend on them
    rest = dict(edge=sc["edge"], label=sc["label"], radius=np.full(H * W, 5, np.int32))
    out = {}
    for tag in ("device", "model"):
        g = capi.from_scene(sc, p, device=0)
        if tag == "device":
            assert g.plane_prior(case["raw"], case["xy"], case["xyz"], cam) == 0
            g.upload_state(planes=None, **rest)
            assert N.same_bits(g.get("planes"), want)
        else:
            g.upload_state(planes=want, **rest)
        g.run_patchmatch()
        out[tag] = {n: g.get(n) for n in ("planes", "costs", "selected_views", "weak_info", "radius")}
        g.close()
    assert N.same_bits(out["device"]["planes"], out["model"]["planes"]) and N.same_bits(out["device"]["costs"], out["model"]["costs"])
    for n in ("selected_views", "weak_info", "radius"):
        assert np.array_equal(out["device"][n], out["model"][n]), n
    assert not N.same_bits(out["device"]["planes"], want)       # the pass did something
