"""Records what the reference's own device text (oracle/_ref/libdvp_ref.so, built by oracle/make_ref.py) gives, for the GPU
tests that cannot have the reference beside them (tests/test_gpu_reference_golden.py):

  reference_kat.npz    ComputeMultiViewCostVectorOld of the reference text on 400 (pixel, plane) pairs of the KAT scene
                       (ref_pin.kat_scene / kat_inputs: four corner pixels, planes that project outside, radius 5 / 10 / 15),
                       both samplers, and per sampler the maximum |oracle contract - reference| measured when this was made.
  reference_sites.npz  on the 64x48 S = 3 two-pass scene, for every RNG-free launch site of both passes: each integer buffer
                       the launch changes, as the reference text leaves it when started from the oracle-contract's
                       pre-launch state, and the mask of entries where the oracle's contract agreed (decided here, from
                       reference and oracle alone).  A mask may leave out at most 1 % of a buffer.  `candidate` is not
                       recorded: a record of a pixel closer than weak_radius to the border always has an empty sector,
                       which the reference reads uninitialised (APD.cu:3783) — a third of the records at this size, on any scene.
  reference_contract_distance.json  per launch site, the distance between the reference text and the oracle's contract numerics
                       (tests/test_reference_pin.py::test_launch_site_contract_distance gates at twice these).

Inputs are regenerated from synth seeds, never stored.      python tests/golden/make_reference_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for d in (os.path.dirname(TESTS), TESTS):
    if d not in sys.path:
        sys.path.insert(0, d)

KAT_PAIRS = 400
SITE_SHAPE = (64, 48, 3, 0, 4)      # W, H, S, sampler, weak_peak_radius


def kat_golden():
    import ref_pin as P
    from ref_pin import O, R
    out = {}
    W, H, S, sc, p, st = P.kat_scene()
    px, planes = P.kat_inputs(W, H, sc, KAT_PAIRS)
    for sampler in (0, 1):
        o = O.from_scene(sc, p, sampler=sampler)
        o.set_numerics(0)
        o.upload_state(**st)
        r = R.from_scene(sc, p, sampler=sampler)
        r.upload_state(**st)
        cr, co = r.eval_cost_vectors(px, planes), o.eval_cost_vectors(px, planes)
        assert np.isfinite(cr).all() and (cr < 2.0).mean() > 0.3
        out["costs_s%d" % sampler] = cr
        out["costs_maxdiff_s%d" % sampler] = np.array(np.abs(cr.astype(np.float64) - co).max())
        o.close()
        r.close()
    return out


def sites_golden():
    import ref_pin as P
    from ref_pin import O, R, synth
    W, H, S, sampler, wpr = SITE_SHAPE
    sc = synth.make_scene(W, H, S)
    p1, p2 = P.pass_params(S, wpr)
    ints = [n for n in P.CHECKED if n not in P.FLOATS and n != "candidate"]
    out = {}
    state, depths = P.first_state(sc), None
    for ps, params in ((1, p1), (2, p2)):
        o = O.from_scene(sc, params, sampler=sampler, depths=depths)
        o.set_numerics(0)
        o.upload_state(**state)
        r = R.from_scene(sc, params, sampler=sampler, depths=depths)
        for idx, (st, it, col, pre, post) in enumerate(P.walk(o, dict(ref=r))):
            if st not in P.RNG_FREE:
                continue
            for n in ints:
                a, b = post["ref"][n], post["oracle"][n]
                if not ((a != pre[n]).any() or (b != pre[n]).any()):
                    continue
                same = (a == b)
                assert same.mean() >= 0.99, (ps, st, col, n, float(same.mean()))
                out[P.site_key(ps, idx, st, col, n)] = a
                out[P.site_key(ps, idx, st, col, n) + "_mask"] = np.packbits(same.reshape(-1))
        r.close()
        if ps == 1:
            state, depths = P.second_state(o, sc), sc["depth_gt"]
            assert (state["weak"] == synth.WEAK).sum() > 50
        o.close()
    return out


def distance_table():
    import test_reference_pin as T
    sites = {}
    for shape in T.SHAPES[1:3]:
        walks = T.walked(shape)
        for site in T.SITES:
            sites[T._distance_key(shape, site)] = walks[site[0]][site[1]][4]
    return dict(_comment="reference text vs the oracle's contract numerics, per launch site, each launch started from the literal "
                         "oracle's state: int_share = share of pixels with a differing integer output; w / cost: plane offset "
                         "(depth after get_depth_normal) and cost, share of pixels moved by more than 1e-3 relative and mean "
                         "relative movement.  Written by tests/golden/make_reference_golden.py.", sites=sites)


def make_all(distance=True):
    out = {"reference_kat.npz": kat_golden(), "reference_sites.npz": sites_golden()}
    if distance:
        out["reference_contract_distance.json"] = distance_table()
    return out


if __name__ == "__main__":
    for fname, content in make_all().items():
        path = os.path.join(HERE, fname)
        if fname.endswith(".json"):
            with open(path, "w") as f:
                json.dump(content, f, indent=1, sort_keys=True)
                f.write("\n")
        else:
            np.savez_compressed(path, **content)
        print("%s: %d bytes" % (fname, os.path.getsize(path)))
