"""Shared by tests/test_reference_pin.py and tests/golden/make_reference_golden.py: scenes of the reference pin and the
launch-by-launch walk that runs one launch in the oracle and in the reference's own device text (oracle/reference.py)
from the same pre-launch state."""
import numpy as np

from conftest import synth, make_params, count_diff, stage_sequence, CHECKED, first_pass_state, second_pass_inputs
from oracle import oracle as O
from oracle import reference as R

ITERS = 2
WEAK_IDX = ("neighbours", "complex", "label_boundary")     # indexed by neighbours_map, not by pixel
FLOATS = ("planes", "costs", "fit_planes", "complex")
RNG_FREE = ("gen_edge_inform", "find_nearest_strong", "neighbour_update", "get_depth_normal", "filter_strong",
            "depth_to_weak", "local_refine")


def pass_params(S, weak_peak_radius=4):
    """FIRST_INIT then REFINE_ITER with geometric consistency, every prior on (as test_gpu_strong_reuse._params)"""
    p1 = make_params(S + 1, max_iterations=ITERS, state=synth.FIRST_INIT, use_APD=0)
    p2 = make_params(S + 1, max_iterations=ITERS, state=synth.REFINE_ITER, use_APD=1, geom_consistency=1,
                     weak_peak_radius=weak_peak_radius, rotate_time=2, ransac_threshold=0.01)
    return p1, p2


def first_state(sc):
    st = first_pass_state(sc)
    W, H = sc["width"], sc["height"]
    st["radius"] = (5 + np.arange(W * H) % 3 * 5).astype(np.int32)   # radius prior: 5 / 10 / 15
    return st


def second_state(o1, sc):
    """the second pass's inputs from the first pass's oracle, the flat regions made WEAK (as test_gpu_strong_reuse.reference)"""
    W, H = sc["width"], sc["height"]
    st2 = second_pass_inputs(o1, sc)
    weak = st2["weak"].reshape(H, W).copy()
    weak[sc["flat"] & (weak == synth.STRONG)] = synth.WEAK
    st2["weak"] = weak.reshape(-1)
    return st2


def load_state(eng, pre, weak0):
    """every buffer of `pre` into `eng`.  The WEAK-indexed ones are sized by upload_state from the pass's INPUT weak map
    `weak0` (APD.cpp:1182-1193): DepthToWeak changes weak_info, never the WEAK list."""
    eng.upload_state(planes=pre["planes"], views=pre["selected_views"], weak=weak0, edge=pre["edge"],
                     label=pre["label"], radius=pre["radius"])
    for n in O.BUFFERS:
        eng.set(n, pre[n])


def walk(o, engines, iters=ITERS, sequence=None):
    """For every launch of the pass, in conftest.stage_sequence order: copy the oracle `o`'s pre-launch buffers into every
    engine of `engines` (a dict name -> Oracle-like), run the launch in each and in `o`, yield
    (stage, iter, colour, pre, post) with post[name] = {buffer: array} (o's under the key "oracle").  The next launch starts
    from o's state again, so one difference does not hide the next."""
    weak0 = o.get("weak_info")
    for st, it, col in (sequence or stage_sequence(iters)):
        pre = {n: o.get(n) for n in O.BUFFERS}
        post = {}
        for name, e in engines.items():
            load_state(e, pre, weak0)
            assert e.weak_count() == o.weak_count()
            e.run_stage(st, it, col)
            post[name] = {n: e.get(n) for n in CHECKED}
        o.run_stage(st, it, col)
        post["oracle"] = {n: o.get(n) for n in CHECKED}
        yield st, it, col, pre, post


def _sector_of(i, j):
    """GenEdgeInform's sector of offset (i, j): the angle of atan2(j, i) in degrees, rounded to binary32 (APD.cu:3759)"""
    deg = np.degrees(np.arctan2(float(j), float(i)))
    if deg < 0:
        deg += 360.0
    return int(np.float32(deg) // 30.0)


def full_sector_rows(views, W, H, S, radius):
    """[L, S] bool: all 12 sectors of (pixel, view) have at least one in-image offset whose pixel selected the view"""
    out = np.zeros((H * W, S), bool)
    v = views.reshape(H, W)
    for s in range(S):
        sel = np.zeros((H + 2 * radius, W + 2 * radius), bool)
        sel[radius:radius + H, radius:radius + W] = (v >> s) & 1 == 1
        has = np.zeros((12, H, W), bool)
        for i in range(-radius, radius + 1):
            for j in range(-radius, radius + 1):
                if i == 0 and j == 0:
                    continue
                has[_sector_of(i, j)] |= sel[radius + j:radius + j + H, radius + i:radius + i + W]
        out[:, s] = has.all(axis=0).reshape(-1)
    return out


def kat_inputs(W, H, sc, n, seed=7):
    """the (pixel, plane) pairs of test_gpu_parity.test_cost_vectors_kat: the four corner pixels first, planes of which many
    project outside the source images"""
    rng = np.random.default_rng(seed)
    px = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int32)
    px[:64] = [[0, 0], [W - 1, H - 1], [0, H - 1], [W - 1, 0]] * 16
    depth = rng.uniform(1.5, 7.8, n).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm[:, 2] = -np.abs(nrm[:, 2]) - 0.3
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    K = sc["cameras"][0]["K"]
    X = depth * (px[:, 0] - K[2]) / K[0]
    Y = depth * (px[:, 1] - K[5]) / K[4]
    d = -(nrm[:, 0] * X + nrm[:, 1] * Y + nrm[:, 2] * depth)
    return px, np.concatenate([nrm, d[:, None]], 1).astype(np.float32)


def kat_scene():
    """the rotated rig with skew of the KATs, radius prior 5 / 10 / 15, the flat regions WEAK with anchors from a
    gen_neighbours launch (for ComputeBilateralNCCNew), the ground-truth depth maps for the geometric term.  Four sources, not
    the five of test_cost_vectors_kat: ComputeBilateralNCCNew reads candidate records, whose stride in the reference is four
    views (main.h:41)"""
    W, H, S = 160, 120, 4
    sc = synth.make_scene(W, H, S, skew=0.6)
    assert sc["cameras"][0]["K"][1] != 0        # skew, as tests/test_numpy_kat.py's geometric-term scene
    p = make_params(S + 1, state=synth.REFINE_ITER, use_APD=1, geom_consistency=1)
    L = W * H
    gt = sc["depth_gt"][0].reshape(-1)
    st = first_pass_state(sc)
    st["planes"] = np.concatenate([np.tile(sc["normal_gt"], (L, 1)), gt[:, None]], 1).astype(np.float32)
    st["views"] = np.full(L, (1 << S) - 1, np.uint32)
    st["weak"] = np.where(sc["flat"].reshape(-1), synth.WEAK, synth.STRONG).astype(np.uint8)
    st["radius"] = (5 + np.arange(L) % 3 * 5).astype(np.int32)
    return W, H, S, sc, p, st


def site_key(ps, idx, st, col, name):
    """key of a recorded buffer in tests/golden/reference_sites.npz"""
    return "p%d_%02d_%s_c%d_%s" % (ps, idx, st, col, name)

