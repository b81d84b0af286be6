"""The device label prior's arithmetic without a GPU: csrc/dvp_labels.hpp, built for the host in tests/labels_host and run one
launch after the other, one pixel after the other (tile by tile where the device uses tiles), against the host mirror's
LabelSegment(scale, image, &stages) in the same library, and scipy's connected components.  Every comparison is exact: the
quarter-size grey image, the texture map, the texture map with the Hough lines, the resized and the cleaned level map, and the
labels with their values — not only the partition.  The region map the host middle reads must induce scipy's partition of the
flat pixels, name every large region by its smallest pixel index and mark nothing else."""
import numpy as np
import pytest

import np_labels as N

pytestmark = pytest.mark.hostbox


@pytest.mark.parametrize("case", N.CASES, ids=N.case_id)
def test_every_stage_equals_the_host_mirror(case):
    content, W, H, scale = case
    want = N.expected(case)
    rc, got = N.serial(N.image(content, W, H, scale), scale)
    assert rc == 0
    N.check_against_mirror(got, want, N.sizes(W, H, scale)["weak_tex_num"])


def test_sizes_follow_labels_cpp():
    assert N.sizes(258, 130, 2) == dict(quarter=(32, 64), level=(33, 65), weak_tex_num=2, unit=1)     # 64.5 and 32.5 round away from zero
    assert N.sizes(480, 360, 0) == dict(quarter=(90, 120), level=(360, 480), weak_tex_num=168, unit=3)
    assert N.sizes(480, 360, 1)["weak_tex_num"] == 42 and N.sizes(13, 15, 2)["level"] == (4, 3)


def test_pitch_is_honoured():
    img = N.image("picture", 63, 65, 1)
    wide = np.zeros((65, 80), np.uint8)
    wide[:, :63] = img
    rc, got = N.serial(wide[:, :63], 1)
    assert rc == 0 and wide[:, :63].strides[0] == 80
    assert np.array_equal(got["labels"], N.expected(("picture", 63, 65, 1))["labels"])


@pytest.mark.parametrize("W,H,scale", [(11, 40, 0), (40, 11, 0), (12, 12, 3), (4, 4, 0)])
def test_small_maps_are_an_error(W, H, scale):
    rc, _ = N.serial(np.zeros((H, W), np.uint8), scale)
    assert rc != 0


def test_cases_say_what_they_claim():
    """what the pictures were built for does occur, by the host mirror's own maps"""
    # the Hough transform fires and adds white pixels; the final map holds numbered regions, small ones and texture
    e = N.expected(("picture", 480, 360, 0))
    assert N.sizes(480, 360, 0)["unit"] == 3 and (e["lines"] != e["texture"]).sum() > 0
    assert (e["labels"] > 0).any() and (e["labels"] == -1).any() and (e["labels"] == 0).any()
    assert (N.expected(("serpentine", 480, 360, 0))["lines"] != N.expected(("serpentine", 480, 360, 0))["texture"]).sum() > 100
    # constant: one region, every pixel inside the frame; noise: none; the 4 x 4 checkerboard: its diagonals agree, so Roberts sees nothing
    e = N.expected(("constant", 257, 131, 0))
    assert (e["texture"][1:-1, 1:-1] == 0).all() and set(np.unique(e["labels"])) == {0, 1}
    assert (N.expected(("noise", 257, 131, 0))["labels"] <= 0).all()
    assert (N.expected(("checker", 480, 360, 0))["texture"][1:-1, 1:-1] == 0).all()
    # corridors: one flat region over many 64 x 16 tiles, at quarter and at level size
    for content in ("serpentine", "spiral"):
        for scale in N.SCALES:
            e = N.expected((content, 480, 360, scale))
            for name in ("texture", "cleaned"):
                lab, size = N.components(e[name] == 0)
                ys, xs = np.nonzero(lab == size[1:].argmax() + 1)
                assert len(set(zip(ys // 16, xs // 64))) >= 2, (content, scale, name)
    e = N.expected(("serpentine", 480, 360, 0))
    lab, size = N.components(e["texture"] == 0)
    ys, xs = np.nonzero(lab == size[1:].argmax() + 1)
    assert len(set(xs // 64)) == 2 and len(set(ys // 16)) >= 5
    # the threshold pictures hold weak_tex_num - 1, weak_tex_num, weak_tex_num + 1 at quarter size wherever the halvings are exact
    for scale in N.SCALES:
        weak = N.sizes(480, 360, scale)["weak_tex_num"]
        _, size = N.components(N.expected(("threshold", 480, 360, scale))["texture"] == 0)
        assert sorted(size[1:]) == [weak - 1, weak, weak + 1]
    # ... and over all cases both comparisons meet all three sizes, at quarter size (`<`) and at level size (`<=`): the Hough
    # lines cut into most level regions that were built for it, the noise and the corridors supply the rest
    seen = {("texture", d): 0 for d in (-1, 0, 1)}
    seen.update({("cleaned", d): 0 for d in (-1, 0, 1)})
    for case in N.CASES:
        weak = N.sizes(case[1], case[2], case[3])["weak_tex_num"]
        if weak < 2:
            continue
        for name in ("texture", "cleaned"):
            _, size = N.components(N.expected(case)[name] == 0)
            for d in (-1, 0, 1):
                seen[(name, d)] += int((size[1:] == weak + d).any())
    assert min(seen.values()) >= 2, seen
    # Roberts roots 4, 5, 255, 256, 260, 261 all occur; 256 ... 260 are black
    e = N.expected(("roberts", 480, 360, 0))
    q = e["quarter"].astype(np.int64)
    t1, t2 = q[1:-1, 1:-1] - q[2:, 2:], q[2:, 1:-1] - q[1:-1, 2:]
    root = np.floor(np.sqrt((t1 * t1 + t2 * t2).astype(np.float64))).astype(np.int64)
    assert set(N.ROBERTS_ROOTS) <= set(np.unique(root))
    inner = e["texture"][1:-1, 1:-1]
    for r, white in zip(N.ROBERTS_ROOTS, (False, True, True, False, False, True)):
        assert ((inner[root == r] == 255) == white).all(), r
    # the frame clean-up changes pixels, all four corners among them
    corners = 0
    for content in ("frame", "constant"):
        for (W, H) in N.SIZES:
            e = N.expected((content, W, H, 2))
            ch = e["resized"] != e["cleaned"]
            corners += int(ch[0, 0] and ch[0, -1] and ch[-1, 0] and ch[-1, -1])
    e = N.expected(("frame", 480, 360, 2))
    assert corners >= 2 and (e["resized"] != e["cleaned"]).sum() > 100
    # 258 x 130 at scale 2: the quarter map is 64 wide, the level 65: a real resize
    assert N.expected(("picture", 258, 130, 2))["lines"].shape == (32, 64) and N.expected(("picture", 258, 130, 2))["resized"].shape == (33, 65)
