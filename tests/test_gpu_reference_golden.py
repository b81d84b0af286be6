"""The engine against recordings of the reference's own device text (tests/golden/reference_*.npz, made by
tests/golden/make_reference_golden.py from the library oracle/make_ref.py builds; tests/test_reference_pin.py pins the
oracle to that text on the host).  These tests read the recordings only — inputs are regenerated from synth seeds — and
never skip.

The engine equals the oracle's contract numerics bit for bit, so what the recordings predict is known: cost vectors within
the |oracle contract - reference| maximum stored beside them (the factor 2 covers that figure's sampling, nothing else), and
the integer outputs of the RNG-free launch sites equal wherever the oracle's contract equalled the reference when the
recording was made (a stored mask, allowed to leave out at most 1 % of a buffer; at this scene it leaves out nothing)."""
import os

import numpy as np
import pytest

import ref_pin as P
from conftest import pkg, synth, stage_sequence

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT_PAIRS = 400
SITE_SHAPE = (64, 48, 3, 0, 4)      # W, H, S, sampler, weak_peak_radius: as make_reference_golden.py


def capi():
    return pkg("capi")


@pytest.mark.parametrize("sampler", [0, 1])
def test_cost_vectors_against_the_recorded_reference(sampler):
    """dvp_eval_cost_vectors on the KAT scene (rotated rig with skew, radius prior 5 / 10 / 15, the four corner pixels, planes
    that project outside the source images) within 2 x the stored maximum of the recorded reference costs"""
    W, H, S, sc, p, st = P.kat_scene()
    px, planes = P.kat_inputs(W, H, sc, KAT_PAIRS)
    with np.load(os.path.join(GOLDEN, "reference_kat.npz")) as z:
        want, bound = z["costs_s%d" % sampler], float(z["costs_maxdiff_s%d" % sampler])
    assert want.shape == (KAT_PAIRS, S) and 0 < bound < 1e-3
    g = capi().from_scene(sc, p, sampler=sampler)
    g.upload_state(**st)
    got = g.eval_cost_vectors(px, planes)
    g.close()
    d = np.abs(got.astype(np.float64) - want)
    print("\nsampler %d: max |engine - reference| = %.3g (recorded contract distance %.3g)" % (sampler, d.max(), bound))
    assert np.isfinite(got).all()
    assert ((got == 2.0) == (want == 2.0)).mean() > 0.995      # the same patches are evaluated / rejected
    assert d.max() <= 2 * bound


def test_rng_free_sites_against_the_recorded_reference():
    """64x48, S = 3, FIRST_INIT then REFINE_ITER with > 50 WEAK pixels, launch by launch: after every RNG-free launch site the
    integer buffers it changes are the reference text's recording wherever the oracle's contract agreed with it."""
    W, H, S, sampler, wpr = SITE_SHAPE
    sc = synth.make_scene(W, H, S)
    p1, p2 = P.pass_params(S, wpr)
    with np.load(os.path.join(GOLDEN, "reference_sites.npz")) as z:
        rec = {k: z[k] for k in z.files}
    names = sorted(k for k in rec if not k.endswith("_mask"))
    assert len(names) >= 6
    used = set()
    state, depths = P.first_state(sc), None
    for ps, params in ((1, p1), (2, p2)):
        g = capi().from_scene(sc, params, sampler=sampler, depths=depths)
        g.upload_state(**state)
        for idx, (st, it, col) in enumerate(stage_sequence(P.ITERS)):
            g.run_stage(st, it, col)
            if st not in P.RNG_FREE:
                continue
            for key in names:
                n = key[len(P.site_key(ps, idx, st, col, "")):]
                if not key.startswith(P.site_key(ps, idx, st, col, "")):
                    continue
                want = rec[key]
                mask = np.unpackbits(rec[key + "_mask"])[:want.size].astype(bool).reshape(want.shape)
                assert mask.mean() >= 0.99, key
                got = g.get(n)
                assert got.shape == want.shape, key
                nd = int(((got != want) & mask).sum())
                assert nd == 0, "%s: %d entries differ from the recorded reference after %s(colour=%d) of pass %d" % (n, nd, st, col, ps)
                used.add(key)
        if ps == 1:
            state, depths = P.second_state(g, sc), sc["depth_gt"]
            assert (state["weak"] == synth.WEAK).sum() > 50
        g.close()
    assert used == set(names)
