"""The mesher without a GPU: the serial text of csrc/dvp_mesh.hpp (tests/mesh_host) equals the numpy restatement of tests/np_mesh.py bit
for bit - block set, SF, W, colour sums, vertices, colours, faces - over the case table; the case table holds what it says; the closed
cases are closed, consistently oriented manifolds of Euler characteristic 2 and positive volume, as close to the true sphere as twice
what a binary64 model of the same definition manages; every refusal carries its message.  The device's view cull (view_misses_block and
what it stands on, run here through `mesh_host cull`) is sound - a skipped (block, view) pair has no sample that view contributes to,
without exception - over the case table and a seeded sweep of cameras, and skips every pair its own margins say it must."""
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
    for n in (511, 512, 513, 968):                                                 # mesh_scan's chunks of 512: one short, exact, one over, nearly two
        assert len(serial_of("blocks_%d" % n)["keys"]) == n
    assert len(serial_of("blocks_968")["faces"]) > 50000
    for cam, depth, mask, _ in CASES["oblique_sphere"]["views"]:                    # the picture border cuts the sphere
        assert depth.shape == (28, 40) and (mask[0].any() or mask[-1].any() or mask[:, 0].any() or mask[:, -1].any())
        K = cam["K"]
        assert K[0] != K[4] and K[2] != K[5] and np.count_nonzero(np.abs(cam["R"]) > 1e-3) >= 8
    assert M.edge_use(serial_of("oblique_sphere")["faces"])[1] > 0                 # ... so the mesh is open
    for k, kind in M.UNCULLABLE.items():                                            # a cull applied with these K would drop the right and bottom halves
        cam, depth, mask, _ = CASES["uncullable_views"]["views"][k]
        assert mask[:, 20:].sum() >= 40 and mask[14:].sum() >= 40
        assert {"skew": cam["K"][1] != 0, "k2": cam["K"][8] == 2, "r": abs(np.linalg.norm(cam["R"][:3]) - 1) > 4e-4}[kind]


def test_the_cull_knows_which_cameras_it_may_judge(tmp_path):
    for name, c in CASES.items():
        cullable, _ = M.cull(c["views"], c["s"], c["tau"], tmp_path)
        want = [k not in M.UNCULLABLE for k in range(len(c["views"]))] if name == "uncullable_views" else [True] * len(c["views"])
        assert cullable.tolist() == want, name


# ---- the view cull ----------------------------------------------------------------------------------------------------------------

FACES = ("left", "right", "top", "bottom", "behind", "too far")


def view_frame(view):
    """(K (3, 3), R (3, 3), t, cols, rows, largest masked depth) in binary64 from the record's binary32 values"""
    cam, depth, mask, _ = view
    m = (mask != 0) & (depth > 0)
    return (cam["K"].astype(np.float64).reshape(3, 3), cam["R"].astype(np.float64).reshape(3, 3), cam["t"].astype(np.float64), depth.shape[1], depth.shape[0],
            float(depth[m].max()) if m.any() else 0.0)


def face_forms(view, T, tau):
    """per face a form over the camera-frame points T (..., 3) that is negative exactly where the point lies beyond that face of the
    region a contributing sample lives in (z > 0, -1.5 < px < cols - 0.5, -1.5 < py < rows - 0.5, z <= depth_max + tau); with the
    form's gradient norm and, for the four sides, (focal, pixels from the true face to the cull's plane).  K without skew, K[8] == 1"""
    K, _, _, cols, rows, dmax = view_frame(view)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = T[..., 0], T[..., 1], T[..., 2]
    side = lambda f, u, a, h: (f * u + a * z, np.hypot(f, a), (abs(f), h))
    return dict(zip(FACES, (side(fx, x, cx + 1.5, 0.5), side(-fx, x, cols - 0.5 - cx, 1.5), side(fy, y, cy + 1.5, 0.5), side(-fy, y, rows - 0.5 - cy, 1.5),
                            (z, 1.0, None), (float(np.float32(dmax) + np.float32(tau)) - z, 1.0, None))))


def block_samples(at, s):
    """the binary32 sample positions (B, 512, 3) of the blocks `at` (B, 3), as binary64"""
    l = np.arange(512)
    idx = np.asarray(at)[:, None, :] * 8 + np.stack([l >> 6, (l >> 3) & 7, l & 7], -1)[None]
    return M.lattice(idx, np.float32(s), np.float32).astype(np.float64)


def must_skip(view, at, s, tau):
    """The completeness condition of the cull, from its own margins; at (B, 3) block coordinates, answer (B,) bool.
    view_misses_block tests a sphere of r = 1.25 radius + 1e-3 (distance + radius) around the block centre C, radius = 6.0622 s + 1e-6
    |C|_1.  Closer than 500 radii, r < 1.25 radius + 0.501 radius < 2 radius, and the quarter radius left over is far above what the
    binary32 roundings inside the function can move a bound relative to the distance (a few 1e-7 of it); what they move it
    relative to the coordinates is bounded by e = 1e-6 (|C|_1 + |t|_1) (three products and three sums per coordinate, 2^-24 each).
      behind / too far: the function skips when tz + r <= 0, or tz - r > depth_max + tau: so it must when the centre lies more than
        2 radius + e beyond z = 0 or z = depth_max + tau.
      the four sides: the function's plane is n' = (f, a + h) against the true face's n = (f, a), h = 0.5 pixels at the left and top (-2
        against -1.5) and 1.5 at the right and bottom (cols + 1 against cols - 0.5).  n'.T = n.T + h tz and |n'| <= |n| + h, so n'.T <
        -r |n'| follows from n.T / |n| < -(r + h (tz + r) / |n|), and |n| >= f: the centre must lie beyond the true face by more than
        2 radius + h max(tz + 2 radius, 0) / f + e: h pixels' footprint at the depth of the block's far end, not of its centre (the
        difference shows where f is a fraction of a pixel, and at the right and bottom one pixel is not enough: the plane is 1.5 away).
    A view without a masked pixel must always be skipped; a camera that is not cullable never has to be."""
    K, R, t, cols, rows, dmax = view_frame(view)
    s = float(np.float32(s))
    C = (np.asarray(at, np.float64) * 8.0 + 3.5) * s
    radius = 6.0622 * s + 1e-6 * np.abs(C).sum(-1)
    T = C @ R.T + t
    e = 1e-6 * (np.abs(C).sum(-1) + np.abs(t).sum())
    must = np.zeros(len(C), bool)
    for name, (g, norm, side) in face_forms(view, T, tau).items():
        margin = 2 * radius + e
        if side:
            margin = margin + side[1] * np.maximum(T[:, 2] + 2 * radius, 0) / side[0]
        must |= g / norm < -margin
    must &= np.linalg.norm(T, axis=-1) < 500 * radius
    return must if dmax > 0 else np.ones(len(C), bool)


def contributes(view, keys, s, tau):
    """(B,) bool: the view alone gives some sample of the block a weight, under the binary32 definition"""
    return (M.integrate([view], keys, s, tau)[1] > 0).any(1)


def sweep():
    """(views, pairs): 400 seeded cameras - a random orthonormal R (reflections included), 1 ... 80 columns and rows drawn apart, fx
    0.3 ... 30 picture widths, fy / fx 0.5 ... 2, the principal point -0.5 ... 1.5 of the picture, s 10^-2.5 ... 1, tau 1 ... 8 voxels, a
    random depth map of 5 to 500 voxels with one pixel in seven unmasked - and for each 9 blocks near each of the six faces: the
    block of a point on the face (inside the other faces or up to 30 % outside) moved up to 4 block radii off it, either way"""
    rng = np.random.default_rng(77)
    views, pairs = [], []
    for n in range(400):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        R = q * np.sign(np.diag(r)) * rng.choice([-1.0, 1.0])                       # det +1 or -1
        cols, rows = (int(v) for v in rng.integers(1, 81, 2))
        fx = cols * 10 ** rng.uniform(np.log10(0.3), np.log10(30.0))
        fy = fx * 2 ** rng.uniform(-1, 1)
        cx, cy = cols * rng.uniform(-0.5, 1.5), rows * rng.uniform(-0.5, 1.5)
        s = 10 ** rng.uniform(-2.5, 0)
        tau = s * rng.uniform(1, 8)
        eye = rng.uniform(-1, 1, 3) * s * 10 ** rng.uniform(0, 3.5)
        scale = s * 10 ** rng.uniform(1, 2.7)
        cam = np.zeros((), M.CAMERA_DTYPE)
        cam["K"], cam["R"], cam["t"], cam["c"], cam["height"], cam["width"] = [fx, 0, cx, 0, fy, cy, 0, 0, 1], R.reshape(-1), -R @ eye, eye, rows, cols
        depth = (scale * rng.uniform(0.5, 1.0, (rows, cols))).astype(np.float32)
        mask = (rng.uniform(size=(rows, cols)) > 1 / 7).astype(np.uint8)
        view = (cam, depth, mask, np.zeros((rows, cols, 3), np.uint8))
        views.append(view)
        K, R, t, _, _, dmax = view_frame(view)
        if dmax == 0:
            dmax = scale
        Ki = np.linalg.inv(K)
        for face in range(6):
            for _ in range(9):
                px, py = -1.5 + (cols + 1) * rng.uniform(-0.3, 1.3), -1.5 + (rows + 1) * rng.uniform(-0.3, 1.3)
                z = (dmax + tau) * rng.uniform(0.02, 1.1)
                if face < 4:
                    px, py = (-1.5, py) if face == 0 else (cols - 0.5, py) if face == 1 else (px, -1.5) if face == 2 else (px, rows - 0.5)
                    normal = np.array([[fx, 0, cx + 1.5], [-fx, 0, cols - 0.5 - cx], [0, fy, cy + 1.5], [0, -fy, rows - 0.5 - cy]][face])
                else:
                    z, normal = (0.0 if face == 4 else dmax + tau), np.array([0.0, 0.0, 1.0])
                point = z * (Ki @ [px, py, 1.0]) if face != 4 else np.append(rng.uniform(-1, 1, 2) * scale, 0.0)
                point = point + normal / np.linalg.norm(normal) * rng.uniform(-4, 4) * 6.0622 * s
                X = np.linalg.solve(R, point - t)
                pairs.append((n, s, tau, np.floor(X / float(np.float32(s)) / 8.0).astype(np.int64)))
    return views, np.array([(n, s, tau, at) for n, s, tau, at in pairs], M.PAIR_DTYPE)


def cull_of(name, tmp):
    """(label, skipped, contributing, must be skipped), each over the (block, view) pairs of a case or of the sweep"""
    if name != "sweep":
        c = CASES[name]
        keys = M.blocks(c["views"], c["s"], c["tau"])
        cullable, skipped = M.cull(c["views"], c["s"], c["tau"], tmp)
        assert skipped.shape == (len(keys), len(c["views"]))
        at = M.key_blocks(keys)
        con = np.stack([contributes(v, keys, c["s"], c["tau"]) for v in c["views"]], 1)
        must = np.stack([must_skip(v, at, c["s"], c["tau"]) if ok else np.zeros(len(at), bool) for v, ok in zip(c["views"], cullable)], 1)
        return skipped, con, must
    views, pairs = sweep()
    skipped = M.cull_pairs(views, pairs, tmp)
    assert len(pairs) >= 20000 and skipped.shape == (len(pairs),)
    con, must = np.zeros(len(pairs), bool), np.zeros(len(pairs), bool)
    for n, view in enumerate(views):
        mine = np.nonzero(pairs["view"] == n)[0]
        s, tau, at = pairs["s"][mine[0]], pairs["tau"][mine[0]], pairs["at"][mine]
        con[mine] = contributes(view, M.block_keys(at), s, tau)
        must[mine] = must_skip(view, at, s, tau)
    return skipped, con, must


@pytest.mark.parametrize("name", list(CASES) + ["sweep"])
def test_the_cull_is_sound_and_skips_what_its_margins_promise(tmp_path, name):
    """Soundness, exact: no skipped pair has a sample with W > 0 from that view alone.  Completeness: every pair must_skip() names is
    skipped (see there for the derivation).  Printed: the share of the contribution-less pairs that the cull skips (Mesh;
    profiles/mesh_cull.txt)."""
    skipped, con, must = cull_of(name, tmp_path)
    idle = ~con
    print("%-24s pairs %6d  without a contribution %6d  skipped %6d (%5.1f %%)  promised by the margins %6d" %
          (name, con.size, idle.sum(), skipped.sum(), 100.0 * skipped.sum() / max(idle.sum(), 1), must.sum()))
    assert not (skipped & con).any(), "%d skipped pairs have a contribution" % (skipped & con).sum()
    assert not (must & ~skipped).any(), "%d pairs the margins promise are not skipped" % (must & ~skipped).sum()
    if name == "sweep":
        assert idle.sum() > 5000 and con.sum() > 5000 and must.sum() > 2000 and (skipped & ~must).sum() > 500


def test_cull_faces_puts_blocks_beyond_and_across_every_face():
    """binary64 geometry, not the cull: per face of the contributing region, the (block, view) pairs of cull_faces whose 512 samples
    all lie beyond it, and those with samples on both sides"""
    c = CASES["cull_faces"]
    P = block_samples(M.key_blocks(M.blocks(c["views"], c["s"], c["tau"])), c["s"])
    beyond, across = dict.fromkeys(FACES, 0), dict.fromkeys(FACES, 0)
    for view in c["views"]:
        _, R, t, _, _, _ = view_frame(view)
        for name, (g, _, _) in face_forms(view, P @ R.T + t, c["tau"]).items():
            out = g < 0 if name != "behind" else g <= 0
            beyond[name] += int(out.all(1).sum())
            across[name] += int((out.any(1) & ~out.all(1)).sum())
    print("beyond", beyond, "across", across)
    assert min(beyond.values()) >= 8 and min(across.values()) >= 8, (beyond, across)


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
