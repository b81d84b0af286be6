"""The upload probe of the image formats at tile seams and plane corners (test_half_planes.py: check_probe, spoiled_weak_pass)
on the host emulation of the kernels: the format the emulation reports for one spoiler texel at every residue of the tile grids,
and weak passes over spoiled sets against the oracle bit for bit."""
import pytest

from oracle import oracle as O
from tests.emul import emul as E
from test_half_planes import PROBE_SIZES, PROBE_S, check_probe, spoiled_weak_pass


@pytest.mark.parametrize("i", range(len(PROBE_SIZES)), ids=lambda i: "%dx%d" % PROBE_SIZES[i])
def test_probe_finds_spoilers_at_tile_seams_emulated(i, monkeypatch):
    for k in ("DVP_NO_IMAGES8", "DVP_NO_IMAGES16"):
        monkeypatch.delenv(k, raising=False)
    W, H = PROBE_SIZES[i]
    e = E.Emul(W, H, PROBE_S + 1)

    def formats(imgs):
        e.set_images(imgs)
        return (e.image_format(),)
    try:
        check_probe(i, formats)
    finally:
        e.close()


@pytest.mark.parametrize("fmt", [2, 0])
@pytest.mark.parametrize("i", range(len(PROBE_SIZES)), ids=lambda i: "%dx%d" % PROBE_SIZES[i])
def test_weak_pass_with_spoilers_emulated(i, fmt, monkeypatch):
    for k in ("DVP_NO_IMAGES8", "DVP_NO_IMAGES16"):
        monkeypatch.delenv(k, raising=False)
    spoiled_weak_pass(i, fmt, lambda sc, p, seed, smp: O.from_scene(sc, p, seed=seed, sampler=smp, depths=sc["depth_gt"], cls=E.Emul))
