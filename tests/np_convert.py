"""An independent numpy reading of what `apd --convert-from` computes (the reference's colmap2mvsnet.py; csrc/dvp_pairs.hpp,
host/colmap.cpp): the view-selection scores straight from calc_score's definition - intersect two lists, sort the angles, look at
the element at int(S * 0.75) - without the count matrices the project's text uses; OpenCV's nearest-neighbour index rule; the
layout of pair.txt; readers for both COLMAP model formats.  Also the models the score tests share, and the glue that runs
tests/convert_host/convert_host (the project's text, serially, on the host)."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "convert_host", "convert_host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "convert")


# ---- the scores ---------------------------------------------------------------------------------------------------------------
def angles_deg(ci, cj, pts):
    """(180 / pi) * arccos(dot / |u| / |v|) per point, binary64, the reference's operand order; the cosine clamped to [-1, 1]"""
    u, v = ci[None, :] - pts, cj[None, :] - pts
    dot = u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]
    nu = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
    nv = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        c = dot / nu / nv
    c = np.where(c > 1.0, 1.0, np.where(c < -1.0, -1.0, c))
    return (180 / np.pi) * np.arccos(c)


def pair_angles(m, i, j):
    """the angles of calc_score for the pair (i, j), i's list order; NaN (a point at a centre) kept"""
    off, ids = m["offsets"], m["ids"]
    a, b = ids[off[i]:off[i + 1]], ids[off[j]:off[j + 1]]
    a = a[a != -1]
    a = a[np.isin(a, b)]
    order = np.argsort(m["point_ids"], kind="stable")
    at = order[np.searchsorted(m["point_ids"][order], a)]
    return angles_deg(m["centres"][i], m["centres"][j], m["xyz"][at])


def scores(m):
    """(N, N) uint32: S, or 0 when the element at int(S * 0.75) of the sorted angles is below 1 (NaN sorts last)"""
    N = len(m["offsets"]) - 1
    out = np.zeros((N, N), np.uint32)
    for i in range(N):
        for j in range(i + 1, N):
            th = np.sort(pair_angles(m, i, j))
            S = th.size
            s = S
            if S > 0 and th[int(S * 0.75)] < 1:
                s = 0
            out[i, j] = out[j, i] = s
    return out


def pair_text(score):
    """pair.txt (colmap2mvsnet.py:442-448): min(20, n - 1) entries per view, by descending score, ties by descending index"""
    n = score.shape[0]
    k = min(20, n - 1)
    text = "%d\n" % n
    for i in range(n):
        order = sorted(range(n), key=lambda v: (int(score[i, v]), v), reverse=True)[:k]
        text += "%d\n%d " % (i, k) + "".join("%d %d " % (v, int(score[i, v])) for v in order) + "\n"
    return text


# ---- the written image --------------------------------------------------------------------------------------------------------
def nearest_index(dst_n, src_n):
    """cv::resize(INTER_NEAREST): sx = min(floor(x * (1.0 / (dst_n / src_n))), src_n - 1), in double"""
    f = 1.0 / (float(dst_n) / float(src_n))
    return np.minimum(np.floor(np.arange(dst_n, dtype=np.float64) * f).astype(np.int64), src_n - 1)


def convert_image(bgr, pad_w, pad_h, out_w, out_h):
    h, w = bgr.shape[:2]
    padded = np.zeros((pad_h, pad_w, 3), np.uint8)
    padded[:h, :w] = bgr
    return np.ascontiguousarray(padded[nearest_index(out_h, pad_h)][:, nearest_index(out_w, pad_w)])


def picture(w, h, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


# (w, h, pad_w, pad_h, scale factor): identity, halving, a factor that is no integer, padding
IMAGE_CASES = [(13, 7, 13, 7, 1.0), (13, 7, 13, 7, 2.0), (17, 9, 17, 9, 1.5), (9, 5, 13, 7, 1.0), (9, 5, 13, 7, 2.0), (300, 5, 301, 6, 1.0)]


def out_size(pad_w, pad_h, F):
    return int(pad_w / F), int(pad_h / F)


# ---- models for the score tests -----------------------------------------------------------------------------------------------
def model(lists, centres, point_ids, xyz):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    ids = np.concatenate([np.asarray(l, np.int64) for l in lists]) if off[-1] else np.zeros(0, np.int64)
    return dict(offsets=off, ids=ids, centres=np.ascontiguousarray(centres, np.float64), point_ids=np.asarray(point_ids, np.int64),
                xyz=np.ascontiguousarray(xyz, np.float64).reshape(-1, 3))


def random_model(N, tracks, seed, baseline=1.0):
    """N centres on a line `baseline` apart; one point per entry of `tracks` = (length, multiplicity), seen by `length` random
    images, `multiplicity` times by the first of them; -1 entries in between; the point ids are no 0 .. P-1 and not sorted"""
    rng = np.random.default_rng(seed)
    centres = np.stack([np.arange(N) * baseline, rng.normal(0, 0.01, N), rng.normal(0, 0.01, N)], 1)
    P = len(tracks)
    point_ids = rng.permutation(P) * 7 + 3
    xyz = np.stack([rng.uniform(-1, N * baseline + 1, P), rng.uniform(-2, 2, P), rng.uniform(3, 9, P)], 1)
    lists = [[] for _ in range(N)]
    for k, (length, mult) in enumerate(tracks):
        seen = np.sort(rng.choice(N, length, replace=False))
        for n, i in enumerate(seen):
            lists[i] += [point_ids[k]] * (mult if n == 0 else 1)
    for i in range(N):
        l = lists[i] + [-1] * int(rng.integers(0, 4))
        lists[i] = list(rng.permutation(np.asarray(l, np.int64))) if l else []
    return model(lists, centres, point_ids, xyz)


def threshold_model(S, L):
    """two images that share S points of which exactly L are seen under less than 1 degree (far points), the others under about
    11 (near points); a third image shares nothing with them (S = 0 pairs)"""
    centres = np.array([[0.0, 0, 0], [1.0, 0, 0], [50.0, 0, 0]])
    xyz = np.array([[0.5, 0.0, 200.0 + k] if k < L else [0.5, 0.1 * k, 5.0] for k in range(S)] + [[50.0, 0, 5.0]])
    ids = np.arange(S + 1) + 10
    return model([list(ids[:S]), list(ids[:S][::-1]), [ids[S], -1]], centres, ids, xyz)


def score_cases():
    c = {}
    c["n2"] = random_model(2, [(2, 1)] * 9 + [(1, 1)] * 3 + [(2, 3)], 1)
    c["n3"] = random_model(3, [(3, 1)] * 5 + [(2, 2)] * 6 + [(1, 1)] * 2, 2)
    for length in (63, 64, 65, 130):      # one below a wave, a wave, one past it, past two
        c["track%d" % length] = random_model(length + 3, [(length, 1), (length, 2), (2, 3), (1, 1)] + [(5, 1)] * 20, 10 + length)
    c["mult"] = random_model(5, [(2, 1), (2, 2), (2, 3), (5, 3), (3, 2), (1, 3)] * 4, 5)
    c["close"] = random_model(6, [(6, 1)] * 10 + [(3, 2)] * 10, 6, baseline=0.02)      # every pair under 1 degree: zeroed
    for S, L in ((1, 0), (1, 1), (4, 3), (4, 4), (8, 6), (8, 7)):      # L at (3 * S) >> 2 and one above
        c["s%d_l%d" % (S, L)] = threshold_model(S, L)
    m = random_model(4, [(3, 1)] * 6 + [(2, 1)] * 5, 7)      # an image whose list is all -1: its points leave the others' lists too
    lo, hi = m["offsets"][2], m["offsets"][3]
    m["ids"][lo:hi] = -1
    c["all_minus_one"] = m
    # a point whose cosine rounds above 1: on the line through both centres, far out (the reference gets NaN here; clamped: 0 degrees)
    centres = np.array([[0.1, 0.2, 0.3], [0.4, 0.8, 1.2], [3.0, 0.1, 0.7]])
    d = centres[1] - centres[0]
    ts = np.arange(2, 400) * 0.37
    pts = centres[0][None, :] + ts[:, None] * d[None, :]
    cos = [float((np.dot(centres[0] - p, centres[1] - p) / np.sqrt(np.dot(centres[0] - p, centres[0] - p))) / np.sqrt(np.dot(centres[1] - p, centres[1] - p))) for p in pts]
    over = [k for k, v in enumerate(cos) if v > 1.0][:3]
    c["cosine_above_one"] = model([[5, 6, 7], [7, 6, 5], [5, -1]], centres, [5, 6, 7], pts[over] if len(over) == 3 else pts[:3])
    c["cosine_above_one"]["over"] = len(over)
    # a point at a camera centre: 0 / 0, counted in S and never below 1
    c["point_at_centre"] = model([[1, 2], [2, 1]], [[0.0, 0, 0], [1.0, 0, 0]], [1, 2], [[0.0, 0, 0], [0.5, 0, 4.0]])
    return c


def big_model(N=40, P=2000, seed=3):
    """many items for one matrix entry: every point is seen by every image once, one of them twice"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 0.45, N)      # neighbours about a degree apart as the points see them: some pairs are zeroed
    centres = np.stack([4 * np.sin(ang), rng.normal(0, 0.05, N), 4 - 4 * np.cos(ang)], 1)
    xyz = np.stack([rng.uniform(-1, 1, P), rng.uniform(-1, 1, P), rng.uniform(3.5, 5, P)], 1)
    ids = np.arange(P, dtype=np.int64) + 1
    return model([list(rng.permutation(np.concatenate([ids, ids[i:i + 1], [-1, -1]]))) for i in range(N)], centres, ids, xyz)


# ---- the project's text on the host -------------------------------------------------------------------------------------------
def run_program(*args):
    return subprocess.run([PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def serial_scores(m, tmp):
    """(return code, stderr, (N, N) uint32 or None) of convert_host scores"""
    src, dst = os.path.join(str(tmp), "scores.in"), os.path.join(str(tmp), "scores.out")
    N, E, P = len(m["offsets"]) - 1, len(m["ids"]), len(m["point_ids"])
    with open(src, "wb") as f:
        f.write(np.array([N, E, P], np.int64).tobytes() + m["offsets"].astype(np.int64).tobytes() + m["ids"].astype(np.int64).tobytes() + m["centres"].tobytes() +
                m["point_ids"].astype(np.int64).tobytes() + m["xyz"].tobytes())
    out = run_program("scores", src, dst)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    return 0, out.stderr, np.fromfile(dst, np.uint32).reshape(N, N)


def serial_image(bgr, pad_w, pad_h, out_w, out_h, tmp):
    src, dst = os.path.join(str(tmp), "nn.in"), os.path.join(str(tmp), "nn.out")
    np.ascontiguousarray(bgr).tofile(src)
    out = run_program("nn", bgr.shape[1], bgr.shape[0], pad_w, pad_h, out_w, out_h, src, dst)
    if out.returncode != 0:
        return out.returncode, out.stderr, None
    return 0, out.stderr, np.fromfile(dst, np.uint8).reshape(out_h, out_w, 3)


# ---- COLMAP models ------------------------------------------------------------------------------------------------------------
MODEL_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 6: 12, 7: 5, 8: 4, 9: 5, 10: 12}
MODEL_NAMES = {0: "SIMPLE_PINHOLE", 1: "PINHOLE", 2: "SIMPLE_RADIAL", 3: "RADIAL", 4: "OPENCV", 5: "OPENCV_FISHEYE", 6: "FULL_OPENCV", 7: "FOV",
               8: "SIMPLE_RADIAL_FISHEYE", 9: "RADIAL_FISHEYE", 10: "THIN_PRISM_FISHEYE"}


def _records(file):
    return [l.split() for l in open(file) if l.strip() and not l.strip().startswith("#")]


def read_model(folder, ext):
    """cameras {id: (model name, params)}, images [(id, q, t, camera id, name, xy (n, 2), point ids)] by id, points {id: (xyz, rgb)}"""
    cameras, images, points = {}, [], {}
    if ext == ".txt":
        for e in _records(os.path.join(folder, "cameras.txt")):
            cameras[int(e[0])] = (e[1], [float(v) for v in e[4:]])
        lines = open(os.path.join(folder, "images.txt")).read().split("\n")
        k = 0
        while k < len(lines):
            e = lines[k].split()
            k += 1
            if not e or e[0].startswith("#"):
                continue
            o = lines[k].split() if k < len(lines) else []
            k += 1
            images.append((int(e[0]), [float(v) for v in e[1:5]], [float(v) for v in e[5:8]], int(e[8]), e[9],
                           np.array([float(v) for v in o], np.float64).reshape(-1, 3)[:, :2], np.array([int(v) for v in o[2::3]], np.int64)))
        for e in _records(os.path.join(folder, "points3D.txt")):
            points[int(e[0])] = ([float(v) for v in e[1:4]], [int(v) for v in e[4:7]])
    else:
        b = open(os.path.join(folder, "cameras.bin"), "rb").read()
        at = 8
        for _ in range(struct.unpack_from("<Q", b, 0)[0]):
            cid, mid, w, h = struct.unpack_from("<iiQQ", b, at)
            at += 24
            cameras[cid] = (MODEL_NAMES[mid], list(struct.unpack_from("<%dd" % MODEL_PARAMS[mid], b, at)))
            at += 8 * MODEL_PARAMS[mid]
        b = open(os.path.join(folder, "images.bin"), "rb").read()
        at = 8
        for _ in range(struct.unpack_from("<Q", b, 0)[0]):
            v = struct.unpack_from("<idddddddi", b, at)
            at += 64
            end = b.index(b"\0", at)
            name = b[at:end].decode()
            n = struct.unpack_from("<Q", b, end + 1)[0]
            at = end + 9
            obs = np.frombuffer(b, np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")]), n, at)
            at += 24 * n
            images.append((v[0], list(v[1:5]), list(v[5:8]), v[8], name, np.stack([obs["x"], obs["y"]], 1).reshape(-1, 2), obs["id"].astype(np.int64)))
        b = open(os.path.join(folder, "points3D.bin"), "rb").read()
        at = 8
        for _ in range(struct.unpack_from("<Q", b, 0)[0]):
            v = struct.unpack_from("<QdddBBBd", b, at)
            n = struct.unpack_from("<Q", b, at + 43)[0]
            at += 51 + 8 * n
            points[v[0]] = (list(v[1:4]), list(v[4:7]))
    images.sort(key=lambda im: im[0])
    return cameras, images, points


def rotation(q):
    """qvec2rotmat, in Python floats"""
    return [[1 - 2 * q[2] * q[2] - 2 * q[3] * q[3], 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[3] * q[1] + 2 * q[0] * q[2]],
            [2 * q[1] * q[2] + 2 * q[0] * q[3], 1 - 2 * q[1] * q[1] - 2 * q[3] * q[3], 2 * q[2] * q[3] - 2 * q[0] * q[1]],
            [2 * q[3] * q[1] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], 1 - 2 * q[1] * q[1] - 2 * q[2] * q[2]]]


def score_inputs(images, points):
    """the arrays dvp_view_scores takes, from a model as read_model returns it"""
    centres = []
    for im in images:
        R, t = rotation(im[1]), im[2]
        centres.append([-(R[0][c] * t[0] + R[1][c] * t[1] + R[2][c] * t[2]) for c in range(3)])
    pid = sorted(points)
    return model([list(im[6]) for im in images], centres, pid, [points[k][0] for k in pid])


def parse_cam(text):
    """(extrinsic 4 x 4 strings, intrinsic 3 x 3 strings, the last line) of a cam file"""
    lines = text.split("\n")
    assert lines[0] == "extrinsic" and lines[5] == "" and lines[6] == "intrinsic" and lines[10] == "" and lines[12] == "" and len(lines) == 13, lines
    return [l.split(" ") for l in lines[1:5]], [l.split(" ") for l in lines[7:10]], lines[11]
