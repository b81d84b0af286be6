"""The mesher without a GPU: the serial text of csrc/dvp_mesh.hpp (tests/mesh_host) equals the numpy restatement of tests/np_mesh.py bit
for bit - block set, SF, W, colour sums, vertices, colours, faces - over the case table; the case table holds what it says; the closed
cases are closed, consistently oriented manifolds of Euler characteristic 2 and positive volume, as close to the true sphere as twice
what a binary64 model of the same definition manages; every refusal carries its message."""
import numpy as np
import pytest

import np_mesh as M

pytestmark = pytest.mark.hostbox

CASES = M.cases()


@pytest.fixture(scope="module", autouse=True)
def built():
    M.build_program()


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


@pytest.mark.parametrize("case", list(CASES))
def test_serial_text_equals_numpy(serial_of, case):
    c = CASES[case]
    assert M.same(serial_of(case), M.model(c["views"], c["s"], c["tau"], c["min_weight"])) == ""


def test_the_case_table_holds_what_it_says(serial_of):
    for n in (1, 63, 64, 65):
        got = serial_of("blocks_%d" % n)
        assert len(got["keys"]) == n and len(got["faces"]) == 8 * n
    assert len(serial_of("nothing_masked")["keys"]) == 0 and len(serial_of("nothing_masked")["vertices"]) == 0
    above = serial_of("min_weight_above_views")
    assert len(above["keys"]) > 0 and 0 < above["w"].max() < CASES["min_weight_above_views"]["min_weight"] and len(above["vertices"]) == 0 and len(above["faces"]) == 0
    origin = M.key_blocks(serial_of("sphere_at_origin")["keys"])
    around = {(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)}
    assert around <= set(map(tuple, origin.tolist())) and origin.min() < 0        # negative block coordinates, eight blocks meet at the centre
    layer = serial_of("plane_on_layer")
    zero = (layer["w"] > 0) & (layer["sf"] == 0)
    assert zero.any() and len(layer["faces"]) > 0                                  # F == 0 exactly on lattice layer 10, which is outside
    assert np.all(layer["vertices"][:, 2] == np.float32(0.625))                    # ... so every crossing sits on that layer
    two = serial_of("two_views_disagree")
    z = np.sort(np.unique(np.round(two["vertices"][:, 2] / CASES["two_views_disagree"]["s"])))
    assert z[0] > 18                                                               # the far view sees through the near sheet and carves it away
    assert len(CASES["views_33"]["views"]) == 33 and serial_of("views_33")["w"].max() > 6
    half = serial_of("zero_depths_half_mask")
    assert 0 < len(half["vertices"]) < len(serial_of("plane_one_view")["vertices"])
    open_mesh = M.edge_use(serial_of("plane_one_view")["faces"])
    assert open_mesh[0] == 0 and open_mesh[1] > 0                                  # an open mesh: boundary edges, none used twice one way


def test_samples_behind_a_camera_are_skipped(serial_of):
    c, got = CASES["behind_a_camera"], serial_of("behind_a_camera")
    at = M.key_blocks(got["keys"])
    l = np.arange(512)
    z = (at[:, None, 2] * 8 + (l & 7)[None]) * c["s"]
    behind = z < 8.0 * c["s"] - 1e-6                                               # behind the second camera, which stands at z = 8 s
    assert behind.any() and got["w"][behind].max() <= 1 and got["w"][~behind].max() == 2


@pytest.mark.parametrize("case", [n for n, c in CASES.items() if c["closed"]])
def test_closed_cases_are_closed_oriented_manifolds(serial_of, case):
    got = serial_of(case)
    twice_one_way, not_twice, euler = M.edge_use(got["faces"])
    assert (twice_one_way, not_twice, euler) == (0, 0, 2)
    assert len(np.unique(got["faces"])) == len(got["vertices"])
    assert M.signed_volume(got["vertices"], got["faces"]) > 0


@pytest.mark.parametrize("case", ["sphere", "sphere_at_origin"])
def test_the_sphere_is_as_close_as_twice_the_binary64_model(serial_of, case):
    """Vertex distance to the true sphere and the relative error of the enclosed volume, binary32 serial text against twice what the
    binary64 model of the same definition gives (measured in this test; recorded here from the run that wrote it):
      sphere            binary64: 0.701926 voxels, 0.090003   binary32: 0.701930 voxels, 0.091509
      sphere_at_origin  binary64: 0.701008 voxels, 0.079145   binary32: 0.701621 voxels, 0.092932
    (The surface bulges where a view meets it at a grazing angle: a sample just outside the limb lies behind that view's nearest
    pixel by less than tau and counts as inside for it.  The binary64 model shows the same: it is the definition's, not rounding's.)"""
    c = CASES[case]

    def figures(vertices, faces):
        v = np.asarray(vertices, np.float64)
        true = 4.0 / 3.0 * np.pi * (6 * c["s"]) ** 3
        return (np.abs(np.linalg.norm(v - np.asarray(c["centre"]), axis=1) - 6 * c["s"]).max() / c["s"],
                abs(M.signed_volume(v, faces) - true) / true)

    wide = M.model(c["views"], c["s"], c["tau"], c["min_weight"], np.float64)
    want, got = figures(wide["vertices"], wide["faces"]), figures(serial_of(case)["vertices"], serial_of(case)["faces"])
    print("%s: binary64 %.6f voxels, %.6f; binary32 %.6f voxels, %.6f" % ((case,) + want + got))
    assert got[0] <= 2 * want[0] and got[1] <= 2 * want[1]


@pytest.mark.parametrize("args, message", [
    (("0", "1", 1), "the voxel edge must be finite and positive"),
    (("-0.5", "1", 1), "the voxel edge must be finite and positive"),
    (("nan", "1", 1), "the voxel edge must be finite and positive"),
    (("inf", "inf", 1), "the voxel edge must be finite and positive"),
    (("0.05", "0.04", 1), "must be finite and at least the voxel edge"),
    (("0.05", "inf", 1), "must be finite and at least the voxel edge"),
    (("0.05", "nan", 1), "must be finite and at least the voxel edge"),
    (("0.05", "3.3", 1), "spans more than 64 voxels"),
    (("0.05", "0.2", 0), "min_weight must be at least 1"),
    (("0.0000001", "0.0000004", 1), "a lattice index beyond 21 bits (view 0)"),
])
def test_refusals_carry_their_messages(tmp_path, args, message):
    scene = str(tmp_path / "scene.bin")
    M.write_scene(CASES["plane_one_view"]["views"], scene)
    out = M.run_program("build", scene, *args, str(tmp_path / "out"))
    assert out.returncode == 3 and message in out.stderr, (out.returncode, out.stderr)


def test_a_depth_that_is_not_finite_is_refused(tmp_path):
    cam, depth, mask, bgr = CASES["plane_one_view"]["views"][0]
    depth = depth.copy()
    depth[3, 4] = np.inf
    rc, err, _ = M.serial([CASES["plane_one_view"]["views"][0], (cam, depth, mask, bgr)], 0.05, 0.2, 1, tmp_path)
    assert rc == 3 and "a lattice index beyond 21 bits (view 1)" in err
    with pytest.raises(M.Refused, match="view 1"):
        M.blocks([CASES["plane_one_view"]["views"][0], (cam, depth, mask, bgr)], 0.05, 0.2)


def test_more_vertices_than_an_int_holds_are_refused():
    assert M.run_program("vertices", 2147483647).returncode == 0
    out = M.run_program("vertices", 2147483648)
    assert out.returncode == 3 and "2147483648 vertices; an int face index holds at most 2147483647" in out.stderr


def test_negative_zero_is_outside():
    """F >= 0 is outside, -0.0 included (integration cannot produce it - the sums start at +0.0 - so it is pinned here on hand-made
    values): a cell of -0.0 and positive corners has no sign change, -0.0 against a negative corner is a crossing at the -0.0 corner"""
    cell = lambda *F: M.run_program("cell", *F).stdout.split()
    edge = lambda a, b: M.run_program("edge", a, b).stdout.strip()
    assert cell("-0.0", 1, 1, 1, 1, 1, 1, 1) == ["inactive"]
    assert cell("-0.0", "-0.0", "-0.0", "-0.0", "0.0", "0.0", "0.0", "0.0") == ["inactive"]
    assert cell("nan", -1, 1, 1, 1, 1, 1, 1) == ["inactive"]
    assert cell("-0.0", "-0.0", "-0.0", "-0.0", -1, -1, -1, -1) == ["active", "0", "0.5", "0.5"]     # the crossings sit on the -0.0 layer
    assert cell(-1, -1, -1, -1, "-0.0", "-0.0", "-0.0", "-0.0") == ["active", "1", "0.5", "0.5"]
    assert cell(-1, -1, -1, -1, 1, 1, 1, 1) == ["active", "0.5", "0.5", "0.5"]
    assert (edge("-0.0", 1), edge("-0.0", "0.0"), edge(-1, "-0.0"), edge("-0.0", -1), edge("nan", -1), edge(-1, 1), edge(1, -1)) == ("0", "0", "1", "2", "0", "1", "2")
