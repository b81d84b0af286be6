"""TEST INFRASTRUCTURE — a wide-baseline rig and degenerate plane hypotheses (tests only; synth.make_rig stays the rig of
bench.py and of every other test).

synth.make_rig keeps baseline / depth at 0.1, rolls of 5-20 degrees and one focal length +-8 %: the projective denominator
Z = H6 x + H7 y + H8 of every homography it produces is 1 +- 0.1 over a patch.  Here: baseline / depth up to 0.6, rolls of 90 and
180 degrees (portrait next to landscape), focal lengths x2 and x0.5, and a camera 1.4 units AHEAD of the reference one whose epipole
lies inside the reference image.  With this rig a random or perturbed hypothesis can put a patch across the source camera's
principal plane (Z changes sign among the 36 taps), send taps to 1e6 pixels or to inf / NaN coordinates, put the forward point of
the geometric term behind a source camera, and the plane records themselves may be degenerate.

rig / scene            the cameras of the table below and the scene rendered from them (dict shape of synth.make_scene)
hypotheses_ordinary    C0  unrestricted unit normals, depth = ground truth x exp(N(0, 0.5)), centre inside the targeted source
hypotheses_straddling  C1  planes through a point just in front of the forward camera's centre: Z takes both signs over the patch
hypotheses_far_outside C2  a tap whose source coordinate lies more than 1e4 pixels outside the image (centre inside)
hypotheses_behind      C3  the forward point of the geometric term lies behind a selected source camera
hypotheses_special     C4  w in {+-0, NaN, +-inf, subnormal, 1e-38, 3e38}, normals {0, NaN component, length 1e20}, border pixels
arbitrary_state        a REFINE_ITER input state made of such hypotheses

Every class is a deterministic generator of (px, planes) for eval_cost_vectors — planes as the kernels hold them: normal in the
reference camera's frame, offset w with n.X + w = 0 — together with the source view it targets, and a float64 numpy classifier
(`classify`) that reads cameras only, never an engine's output: H = K2 (Rrel - trel n^T / w) K^-1 from the float32 cameras, the
centre's projection and Z at the 36 taps of the radius-5, increment-2 patch.  A class function asserts its own guard (how many
members the classifier confirms) before it returns.

How C2 is built.  A tap leaves the image by 1e4 pixels only when its 3-D point comes within ~1e-2 of the source camera's principal
plane in relative terms (coordinate = f X / Z); a plane that merely grazes the tap's viewing ray (n.K^-1 p -> 0) sends the point to
infinity, whose image is the ray's vanishing point: a few hundred pixels out with this rig, whose cameras all look at one target.
So C2 takes planes through a point of a TAP's viewing ray that lies within 1e-7 ... 1e-3 (relative, either side) of the source's
principal plane.  Only cameras ahead of the reference one have their principal plane in front of it: the forward camera (source 6,
at depth ~1.4) and source 3 (at depth ~0.12).  No camera had to be moved.

C3 draws depths in [0.3, 1.5] with views {forward camera, source 3} selected.  Source 3's principal plane crosses the reference
rays at depth ~0.12, below that range: the members are behind the forward camera (all of them) and in front of source 3, so both
outcomes are met in one pixel's view loop.  No camera had to be moved.
"""
import numpy as np

from conftest import synth

TARGET = np.array([0.0, 0.0, 4.2])
DEPTH_MIN, DEPTH_MAX = 0.3, 60.0
# centre, roll (degrees), focal scale: the reference view, then sources 1..6
CAMERAS = [((0.05, -0.04, 0.0), 0.0, 1.0),
           ((1.6, 0.0, 0.3), 90.0, 1.0),
           ((-1.4, 0.5, -0.8), 180.0, 1.0),
           ((0.0, 1.8, 1.2), -90.0, 2.0),
           ((0.9, -1.2, -1.5), 35.0, 0.5),
           ((2.4, 0.3, 0.0), 10.0, 1.0),
           ((0.15, -0.1, 1.4), 15.0, 1.0)]
FORWARD, SOURCE3 = 6, 3          # numbers of the table
# the look-at is perturbed by (about x, about y) degrees and the principal point shifted by (x, y) pixels, per view
_TILT = [(0.6, -0.4), (-1.1, 0.8), (0.9, 1.2), (-0.7, -0.9), (1.3, 0.5), (-0.5, 1.0), (0.8, -0.7)]
_SHIFT = [(1.5, -1.0), (-2.5, 1.5), (2.0, 2.5), (-1.5, -2.0), (3.0, 1.0), (-2.0, -1.5), (2.5, -2.5)]
# scene(W, H, S) takes the first S of these table numbers as its source views 1..S: the forward camera and source 3 (classes C1,
# C3) are in every scene, the two quarter-turn cameras next
SCENE_ORDER = (6, 3, 1, 2, 4, 5)
TAPS = np.array([-5, -3, -1, 1, 3, 5])


def rig(W, H):
    """[7] CAMERA_DTYPE in table order: index 0 the reference view, 1..6 the sources."""
    cams = np.zeros(len(CAMERAS), dtype=synth.CAMERA_DTYPE)
    deg = np.pi / 180.0
    for i, (c, roll, fs) in enumerate(CAMERAS):
        v = TARGET - np.asarray(c, np.float64)
        ay = -np.arctan2(v[0], v[2]) + deg * _TILT[i][1]
        ax = np.arctan2(v[1], np.hypot(v[0], v[2])) + deg * _TILT[i][0]
        f = 0.9 * W * fs
        K = [f, 0, W / 2.0 + _SHIFT[i][0], 0, 1.01 * f, H / 2.0 + _SHIFT[i][1], 0, 0, 1]
        cams[i] = synth.make_camera(W, H, c, depth_min=DEPTH_MIN, depth_max=DEPTH_MAX, R=synth._rot(ax, ay, deg * roll), K=K)
    return cams


def view_of(number, S):
    """image index (1-based source view) of table camera `number` in scene(W, H, S)"""
    assert number in SCENE_ORDER[:S], (number, S)
    return 1 + SCENE_ORDER.index(number)


_SCENES = {}


def scene(W, H, S):
    """dict of synth.make_scene's shape (images, cameras, depth_gt, normal_gt, edge, label, flat, width, height) with the first S
    sources of SCENE_ORDER.  Cached: callers copy what they change."""
    assert 1 <= S <= len(SCENE_ORDER)
    if (W, H, S) in _SCENES:
        return dict(_SCENES[(W, H, S)])
    all_cams = rig(W, H)
    cams = np.zeros(S + 1, dtype=synth.CAMERA_DTYPE)
    cams[0] = all_cams[0]
    for k in range(S):
        cams[k + 1] = all_cams[SCENE_ORDER[k]]
    px_world = 4.0 / (0.9 * W)
    images, depths = [], []
    sid0 = flat0 = None
    for i in range(S + 1):
        img, dep, sid, fm = synth.render_view(W, H, cams[i], px_world)
        images.append(img)
        depths.append(dep)
        if i == 0:
            sid0, flat0 = sid, fm
    edge = np.zeros((H, W), np.uint8)
    edge[:, 1:] |= (sid0[:, 1:] != sid0[:, :-1]).astype(np.uint8)
    edge[1:, :] |= (sid0[1:, :] != sid0[:-1, :]).astype(np.uint8)
    label = sid0.astype(np.int32) + 1
    label[edge > 0] = -1
    n = np.array([0.25, 0.1, -1.0])
    n /= np.linalg.norm(n)
    sc = dict(images=np.stack(images), cameras=cams, depth_gt=np.stack(depths), normal_gt=n.astype(np.float32),
              edge=edge, label=label, flat=flat0, width=W, height=H)
    _SCENES[(W, H, S)] = sc
    return dict(sc)


def wide_params(make_params, num_images, **kw):
    return make_params(num_images, depth_min=np.float32(DEPTH_MIN), depth_max=np.float32(DEPTH_MAX), **kw)


# ---- float64 reference geometry -------------------------------------------------------------------------------------------------
def _cam(cam):
    K = cam["K"].astype(np.float64).reshape(3, 3)
    R = cam["R"].astype(np.float64).reshape(3, 3)
    t = cam["t"].astype(np.float64)
    return K, R, t, -R.T @ t


def epipole(ref, src):
    """projection of src's centre into ref (pixels)"""
    K, R, t, _ = _cam(ref)
    q = K @ (R @ _cam(src)[3] + t)
    return q[:2] / q[2]


def homographies(ref, src, planes):
    """[n, 3, 3] float64: K2 (Rrel - trel n^T / w) K^-1 for planes [n, 4] (float32 records, read as float64)"""
    Kr, Rr, tr, Cr = _cam(ref)
    Ks, Rs, ts, Cs = _cam(src)
    Rrel = Rs @ Rr.T
    trel = Rs @ (Cr - Cs)
    pl = np.asarray(planes, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        M = Rrel[None] - trel[None, :, None] * pl[:, None, :3] / pl[:, 3, None, None]
        return Ks[None] @ M @ np.linalg.inv(Kr)[None]


def classify(sc, view, px, planes):
    """Reference geometry of hypotheses (px [n, 2], planes [n, 4]) against source view `view` [n] (or one int) of scene `sc`:
    dict(centre [n, 2] the centre's projection, inside [n] it lies in [0, W) x [0, H), Z [n, 36] the denominators at the taps,
    straddles [n] both signs among them, cond [n] min|Z| / max|Z|, far [n] the largest distance of a tap's coordinate from
    the image in pixels (inf for a tap at Z = 0 or a non-finite coordinate), zc_rel [n] the centre's |Z| over the sum of the
    magnitudes of its three terms: how much of them cancels)."""
    W, H = sc["width"], sc["height"]
    px = np.asarray(px, np.float64).reshape(-1, 2)
    n = len(px)
    view = np.broadcast_to(np.asarray(view), (n,))
    Hm = np.zeros((n, 3, 3))
    for v in np.unique(view):
        m = view == v
        Hm[m] = homographies(sc["cameras"][0], sc["cameras"][int(v)], np.asarray(planes)[m])
    dx, dy = np.meshgrid(TAPS, TAPS)
    tx = px[:, 0, None] + dx.reshape(1, -1)
    ty = px[:, 1, None] + dy.reshape(1, -1)
    with np.errstate(all="ignore"):
        def proj(x, y):
            X = Hm[:, 0, 0, None] * x + Hm[:, 0, 1, None] * y + Hm[:, 0, 2, None]
            Y = Hm[:, 1, 0, None] * x + Hm[:, 1, 1, None] * y + Hm[:, 1, 2, None]
            Z = Hm[:, 2, 0, None] * x + Hm[:, 2, 1, None] * y + Hm[:, 2, 2, None]
            return X / Z, Y / Z, Z
        cx, cy, _ = proj(px[:, 0, None], px[:, 1, None])
        qx, qy, Z = proj(tx, ty)
        centre = np.concatenate([cx, cy], 1)
        inside = (centre[:, 0] >= 0) & (centre[:, 0] < W) & (centre[:, 1] >= 0) & (centre[:, 1] < H)
        out = np.maximum(np.maximum(-qx, qx - (W - 1)), np.maximum(-qy, qy - (H - 1)))
        out = np.where(np.isfinite(out), np.maximum(out, 0.0), np.inf)
        aZ = np.abs(Z)
        cond = aZ.min(1) / aZ.max(1)
        x0, y0 = px[:, 0], px[:, 1]
        zc = Hm[:, 2, 0] * x0 + Hm[:, 2, 1] * y0 + Hm[:, 2, 2]
        zc_rel = np.abs(zc) / (np.abs(Hm[:, 2, 0] * x0) + np.abs(Hm[:, 2, 1] * y0) + np.abs(Hm[:, 2, 2]))
    return dict(centre=centre, inside=inside, Z=Z, straddles=(Z.min(1) < 0) & (Z.max(1) > 0), cond=np.nan_to_num(cond),
                far=out.max(1), zc_rel=np.nan_to_num(zc_rel))


def well_inside(c, W, H):
    """the centre's projection keeps a margin from the source's border, so that the float32 centre test of the kernels and the
    float64 one of the classifier agree and "evaluated" can be counted (C1 only: the other classes assert no count and keep every member): a quarter pixel, plus what some 30 binary32 roundings
    (2e-6 of the terms of Z) can move a coordinate of up to max(W, H) pixels when Z is what is left of those terms after cancellation"""
    x, y = c["centre"][:, 0], c["centre"][:, 1]
    with np.errstate(all="ignore"):
        margin = 0.25 + max(W, H) * 2e-6 / c["zc_rel"]
        return (x >= margin) & (x < W - margin) & (y >= margin) & (y < H - margin)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(cam, px):
    """K^-1 (x, y, 1) without the skew, as Get3DPoint (APD.cu:372-377): [n, 3] with z = 1"""
    K = cam["K"].astype(np.float64)
    px = np.asarray(px, np.float64).reshape(-1, 2)
    return np.stack([(px[:, 0] - K[2]) / K[0], (px[:, 1] - K[5]) / K[4], np.ones(len(px))], 1)


def _planes_through(n_cam, X_cam):
    """plane records (n, w) with n.X + w = 0, float32"""
    w = -(n_cam * X_cam).sum(1)
    return np.concatenate([n_cam, w[:, None]], 1).astype(np.float32)


def _keep(px, planes, view, mask, count, guard, name):
    """the first `count` members the classifier confirmed; the guard is the class's own assertion"""
    idx = np.flatnonzero(mask)
    assert len(idx) >= guard, "%s: %d of %d draws are members, the guard asks for %d" % (name, len(idx), len(mask), guard)
    assert count is None or len(idx) >= count, "%s: %d members, %d wanted" % (name, len(idx), count)
    idx = idx[:count]
    return px[idx].astype(np.int32), planes[idx], np.asarray(view)[idx].astype(np.int32)


# ---- the classes ------------------------------------------------------------------------------------------------------------------
def hypotheses_ordinary(sc, count=4096, seed=100):
    """C0: -> (px, planes, view).  Unrestricted unit normals (camera frame), depth = ground truth x exp(N(0, 0.5)), any pixel; the
    targeted view cycles over the scene's sources; members: the centre projects inside it."""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    rng = np.random.default_rng(seed)
    n = 6 * (count or 4096)
    px = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    depth = sc["depth_gt"][0][px[:, 1], px[:, 0]].astype(np.float64) * np.exp(rng.normal(0, 0.5, n))
    planes = _planes_through(_unit(rng, n), _rays(sc["cameras"][0], px) * depth[:, None])
    view = 1 + np.arange(n) % S
    c = classify(sc, view, px, planes)
    return _keep(px, planes, view, c["inside"], count, 500, "C0 ordinary")


def hypotheses_straddling(sc, count=4096, seed=101):
    """C1: -> (px, planes, view).  Planes with a random normal through A = C_src + eps * dir, src the forward camera, eps log-uniform
    in [1e-4, 0.3], dir inside its viewing cone; the pixel is the rounded projection of A into the reference view.  Members: the
    centre projects inside the forward camera, the 36 denominators take both signs, and the plane keeps 1e-3 from the reference
    camera's own centre (|w| >= 1e-3: a plane through that centre maps the whole patch onto the epipole — no variance, cost 2 from
    the variance floor and nothing evaluated; 1 of 7300 draws)."""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    v = view_of(FORWARD, S)
    rng = np.random.default_rng(seed)
    n = 5 * (count or 4096)
    Kr, Rr, tr, Cr = _cam(sc["cameras"][0])
    Ks, Rs, ts, Cs = _cam(sc["cameras"][v])
    q = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    d = _rays(sc["cameras"][v], q)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    eps = np.exp(rng.uniform(np.log(1e-4), np.log(0.3), n))
    A = Cs[None] + eps[:, None] * (d @ Rs)          # R^T d, row-wise
    Ac = (A - Cr[None]) @ Rr.T                      # in the reference camera's frame
    p = Ac @ Kr.T
    px = np.rint(p[:, :2] / p[:, 2:3]).astype(np.int64)
    planes = _planes_through(_unit(rng, n), Ac)
    ok = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
    px = np.clip(px, 0, [W - 1, H - 1])
    c = classify(sc, v, px, planes)
    return _keep(px, planes, np.full(n, v), ok & c["inside"] & well_inside(c, W, H) & c["straddles"] & (np.abs(planes[:, 3]) >= 1e-3), count, 500, "C1 straddling")


def hypotheses_far_outside(sc, count=4096, seed=102):
    """C2: -> (px, planes, view).  Planes with a random normal through the point of a TAP's viewing ray at (1 + e) times the depth
    at which that ray meets the targeted source's principal plane, |e| log-uniform in [1e-7, 1e-3] with either sign, every
    eighth draw e = 0 (module docstring).  Members: the centre projects inside the source and a tap's coordinate lies more than 1e4 pixels outside it."""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    rng = np.random.default_rng(seed)
    n = 48 * (count or 4096)
    targets = [view_of(FORWARD, S)] * 3 + ([view_of(SOURCE3, S)] if SOURCE3 in SCENE_ORDER[:S] else [])
    view = np.array(targets)[np.arange(n) % len(targets)]
    px = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    tap = np.stack([TAPS[rng.integers(0, 6, n)], TAPS[rng.integers(0, 6, n)]], 1)
    r = _rays(sc["cameras"][0], px + tap)
    Kr, Rr, tr, Cr = _cam(sc["cameras"][0])
    s = np.zeros(n)
    for v in np.unique(view):
        Ks, Rs, ts, Cs = _cam(sc["cameras"][int(v)])
        Rrel, trel = Rs @ Rr.T, Rs @ (Cr - Cs)
        m = view == v
        s[m] = -trel[2] / (r[m] @ Rrel[2])          # (Rrel s r + trel).z = 0
    e = np.exp(rng.uniform(np.log(1e-7), np.log(1e-3), n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    e[::8] = 0.0      # on the principal plane to float64 rounding: Z ~ 1e-16, which binary32 may round to 0 (inf / NaN coordinates)
    planes = _planes_through(_unit(rng, n), r * (s * (1 + e))[:, None])
    c = classify(sc, view, px, planes)
    return _keep(px, planes, view, (s > 0) & c["inside"] & (c["far"] > 1e4), count, 500, "C2 far outside")


def forward_point_depth(sc, view, px, planes):
    """sd of ProjectonCamera_cu (APD.cu:489-499) for the forward point of the geometric term (APD.cu:1218-1230), float64: the
    depth in source `view` of the point where the pixel's viewing ray meets the plane"""
    ref = sc["cameras"][0]
    K = ref["K"].astype(np.float64)
    pl = np.asarray(planes, np.float32).astype(np.float64)
    px = np.asarray(px, np.float64)
    with np.errstate(all="ignore"):
        z = -pl[:, 3] * K[0] / ((px[:, 0] - K[2]) * pl[:, 0] + (K[0] / K[4]) * (px[:, 1] - K[5]) * pl[:, 1] + K[0] * pl[:, 2])
        Kr, Rr, tr, Cr = _cam(ref)
        Xw = (_rays(ref, px) * z[:, None]) @ Rr + Cr[None]
        Ks, Rs, ts, Cs = _cam(sc["cameras"][int(view)])
        return (Xw @ Rs.T + ts[None])[:, 2]


def hypotheses_behind(sc, count=1024, seed=103):
    """C3: -> (px, planes, views) with `views` the selected-view WORD (forward camera | source 3).  Unrestricted normals, depth
    uniform in [0.3, 1.5].  Members: the forward point has sd <= 0 in at least one selected source, and a finite positive depth
    along the pixel's ray (the plane record reproduces the drawn depth)."""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    vf, v3 = view_of(FORWARD, S), view_of(SOURCE3, S)
    rng = np.random.default_rng(seed)
    n = 3 * (count or 1024)
    px = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
    depth = rng.uniform(0.3, 1.5, n)
    planes = _planes_through(_unit(rng, n), _rays(sc["cameras"][0], px) * depth[:, None])
    sd_f, sd_3 = forward_point_depth(sc, vf, px, planes), forward_point_depth(sc, v3, px, planes)
    with np.errstate(invalid="ignore"):
        member = ((sd_f <= 0) | (sd_3 <= 0)) & np.isfinite(sd_f) & np.isfinite(sd_3)
    word = (1 << (vf - 1)) | (1 << (v3 - 1))
    return _keep(px, planes, np.full(n, word), member, count, 200, "C3 behind")


SPECIAL_W = [0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, 1e-38, 3e38]


def hypotheses_special(sc, count=4096, seed=104):
    """C4: -> (px, planes, view).  Every combination of w in SPECIAL_W + {an ordinary offset} with a normal in {ordinary, the zero
    vector, one NaN component, length 1e20} (the all-ordinary one left out), at the four corners and at every second pixel of
    the four borders, the borders taken in turn (top, bottom, left, right, top, ...) so that the first `count` records span all
    four.  No classifier: the class is its list.  An operand at which a device primitive is found to differ from
    its host text is added to this list."""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    rng = np.random.default_rng(seed)
    pix = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    borders = [[(x, 0) for x in range(2, W - 1, 2)], [(x, H - 1) for x in range(2, W - 1, 2)],
               [(0, y) for y in range(2, H - 1, 2)], [(W - 1, y) for y in range(2, H - 1, 2)]]
    for k in range(max(len(b) for b in borders)):
        pix += [b[k] for b in borders if k < len(b)]
    recs, pxs = [], []
    for (x, y) in pix:
        z = float(sc["depth_gt"][0][y, x])
        nrm = _unit(rng, 1)[0]
        ordinary_w = float(-(nrm * (_rays(sc["cameras"][0], [(x, y)])[0] * z)).sum())
        k = int(rng.integers(0, 3))
        nan_n = nrm.copy()
        nan_n[k] = np.nan
        for wi, w in enumerate(SPECIAL_W + [ordinary_w]):
            for kind, nv in enumerate((nrm, np.zeros(3), nan_n, nrm * 1e20)):
                if kind == 0 and wi == len(SPECIAL_W):
                    continue
                recs.append([nv[0], nv[1], nv[2], w])
                pxs.append((x, y))
    planes = np.array(recs, np.float64).astype(np.float32)
    px = np.array(pxs, np.int32)
    assert count is None or len(px) >= count, len(px)
    view = 1 + np.arange(len(px)) % S
    w = planes[:count, 3]
    assert ((w > 0) & (w < np.finfo(np.float32).tiny)).any()      # the subnormal offset survives the conversion to binary32
    return px[:count], planes[:count], view[:count].astype(np.int32)


# ---- a REFINE_ITER input state ------------------------------------------------------------------------------------------------------
def arbitrary_state(sc, rng):
    """upload_state arguments for a REFINE_ITER pass: planes are (WORLD normal, depth) as a pass leaves them on disk.  Half of the
    pixels: unrestricted unit normals, depth = ground truth x exp(N(0, 0.6)); the other half: the ground-truth normal and depth
    with 1 % noise.  selected views: any word in [0, 2^S); a 20 x 40 WEAK block in the middle; 2 % of the pixels UNKNOWN."""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    L = W * H
    gt = sc["depth_gt"][0].reshape(-1).astype(np.float64)
    wild = rng.random(L) < 0.5
    n = np.where(wild[:, None], _unit(rng, L), np.tile(sc["normal_gt"].astype(np.float64), (L, 1)) + rng.normal(0, 0.01, (L, 3)))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    depth = np.where(wild, gt * np.exp(rng.normal(0, 0.6, L)), gt * (1 + rng.normal(0, 0.01, L)))
    planes = np.concatenate([n, depth[:, None]], 1).astype(np.float32)
    views = rng.integers(0, 1 << S, L).astype(np.uint32)
    weak = np.full((H, W), synth.STRONG, np.uint8)
    weak[H // 2 - 10:H // 2 + 10, W // 2 - 20:W // 2 + 20] = synth.WEAK
    weak[rng.random((H, W)) < 0.02] = synth.UNKNOWN
    return dict(planes=planes, views=views, weak=weak.reshape(-1), edge=sc["edge"], label=sc["label"],
                radius=np.full(L, 5, np.int32))


def write_behind_block(sc, state, x0=8, y0=8, size=16, seed=105):
    """the shallow C3 planes in a size x size block of `state` (in place): world normals, depths in [0.3, 1.5], the forward camera
    and source 3 selected, STRONG.  -> how many of the block's pixels the classifier confirms as C3 members."""
    W, H, S = sc["width"], sc["height"], len(sc["cameras"]) - 1
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[y0:y0 + size, x0:x0 + size]
    px = np.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    n = len(px)
    depth = rng.uniform(0.3, 1.5, n)
    nc = _unit(rng, n)
    Rr = _cam(sc["cameras"][0])[1]
    idx = px[:, 1] * W + px[:, 0]
    state["planes"][idx] = np.concatenate([nc @ Rr, depth[:, None]], 1).astype(np.float32)     # R^T n: camera -> world
    vf, v3 = view_of(FORWARD, S), view_of(SOURCE3, S)
    state["views"][idx] = (1 << (vf - 1)) | (1 << (v3 - 1))
    state["weak"][idx] = synth.STRONG
    planes_cam = _planes_through(nc, _rays(sc["cameras"][0], px) * depth[:, None])
    sd = forward_point_depth(sc, vf, px, planes_cam)
    return int((sd <= 0).sum())
