"""An INDEPENDENT float64 numpy reading of the reference's depth-map fusion, written from the source text of the
reference's APD.cpp (not from oracle/ or host/): Get3DPointonWorld (:501-524), ProjectCamera (:536-546),
RescaleImageAndCamera (:1750-1771), RescaleMatToTargetSize (:1773-1795), GetAngle (:1797-1806), RunFusion (:1809-1960),
RunFusion_TAT_Intermediate (:1962-2130) and RunFusion_TAT_advanced (:2132-2279).

TEST INFRASTRUCTURE.  It shares no code with the engine or the oracle and uses none of the numerics contract: float64
throughout, math.acos / math.exp.  Views may have maps and images of any size, each its own.

Comparing a float64 model with binary32 code.  Near a threshold the two may legitimately decide differently, and a claim
carries such a difference into later pixels and views.  So every decision is CERTAIN or UNCERTAIN.  It is uncertain when
int(v + 0.5) lies within EPS_PX of a rounding boundary, when a threshold test (reprojection, relative depth, angle, the vote
or the graded k rules) lies within its margin, or when it reads a witness whose claimed state is uncertain; an uncertain
pixel makes every pixel it could claim uncertain.  Certain decisions must match the engine exactly.

The margins bound the binary32 error of the engine's arithmetic on the scenes the tests build: world coordinates |X| <= 6.5,
depths z >= 4 (gross depth outliers go beyond both and miss every threshold by far more than a margin), focal lengths at
the maps' size f <= 160 px, pixel coordinates <= 170 (u = 2^-24, each rounding at most u times the largest magnitude it
can see)."""
import math

import numpy as np

# lift (8 roundings) then rotate + translate (6) put <= 14 u |X| = 5.4e-6 on a camera-frame coordinate; f / z turns that into
# 2.2e-4 px, and the 3 roundings of K . / z on coordinates <= 170 px add 3e-5 px
EPS_PX = 2.5e-4
# z_seen carries the same 14 u |X| = 5.4e-6; over z >= 4 that is 1.4e-6 of relative depth difference (+ 2 roundings of it)
EPS_REL = 1.5e-6
# a dot product of unit binary32 normals: 3 products + 2 sums of terms <= 1, each <= u; acos moves by that over sin(angle)
# (bounded per pair in get_angle), plus the contract's 1 ulp
EPS_DOT = 3e-7
# exp(-s) in binary32 (1 ulp) and the sum of the votes: <= 2 u per vote and addition
EPS_EXP = 1.2e-7

WEAK = 0                                           # main.h:80-84
FLT_MAX = float(np.finfo(np.float32).max)


class View:
    """One problem's inputs as RunFusion holds them after loading (APD.cpp:1836-1871): the camera with K rescaled to the
    depth map, the colour image resized to it, the weak map rescaled to it."""

    def __init__(self, K, R, t, depth, normal, weak=None, image_bgr=None, block=None):
        self.depth = np.asarray(depth, np.float64)
        self.rows, self.cols = self.depth.shape
        self.normal = np.asarray(normal, np.float64).reshape(self.rows, self.cols, 3)
        K = np.asarray(K, np.float64).reshape(9).copy()
        self.R = np.asarray(R, np.float64).reshape(9)
        self.t = np.asarray(t, np.float64).reshape(3)
        if image_bgr is None:
            image_bgr = np.zeros((self.rows, self.cols, 3), np.uint8)
        self.image_exact = image_bgr.shape[:2] == (self.rows, self.cols)
        self.image, self.K = rescale_image_and_camera(image_bgr, self.cols, self.rows, K)
        if weak is None:
            weak = np.full((self.rows, self.cols), 1, np.uint8)
        self.weak = rescale_mat_to_target_size(weak, self.cols, self.rows)
        self.block = block
        R_ = self.R
        # C = -R^T t (APD.cpp:515-518)
        self.C = np.array([-(R_[0 + k] * self.t[0] + R_[3 + k] * self.t[1] + R_[6 + k] * self.t[2]) for k in range(3)])


def rescale_image_and_camera(img, cols, rows, K):
    """APD.cpp:1750-1771: cv::resize(INTER_LINEAR) to the depth map's size; K[0], K[2] scale by cols / img.cols and K[4], K[5]
    by rows / img.rows."""
    if img.shape[1] == cols and img.shape[0] == rows:
        return img.copy(), K
    sx, sy = cols / img.shape[1], rows / img.shape[0]
    K = K.copy()
    K[0] *= sx
    K[2] *= sx
    K[4] *= sy
    K[5] *= sy
    return resize_linear(img, cols, rows), K


def _taps(n_dst, n_src):
    # cv::resize INTER_LINEAR: pixel centres aligned, src = (dst + 0.5) * n_src / n_dst - 0.5, border replicated
    s = (np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5
    i0 = np.floor(s).astype(np.int64)
    a = s - i0
    a = np.where(i0 < 0, 0.0, a)
    i0 = np.clip(i0, 0, n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, a


def resize_linear(img, cols, rows):
    """Bilinear resize of an 8-bit image in float64, rounded half up (the rounding OpenCV's fixed-point path uses)."""
    x0, x1, ax = _taps(cols, img.shape[1])
    y0, y1, ay = _taps(rows, img.shape[0])
    f = img.astype(np.float64)
    h = f[:, x0] * (1 - ax)[None, :, None] + f[:, x1] * ax[None, :, None]
    v = h[y0] * (1 - ay)[:, None, None] + h[y1] * ay[:, None, None]
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def rescale_mat_to_target_size(src, tw, th):
    """APD.cpp:1773-1795, with its swapped factors: the ROW index is divided by scale_x = tw / src.cols and the COLUMN index by
    scale_y = th / src.rows.  Target pixels whose source index falls outside are left unwritten by the reference (uninitialised
    memory); here, as in the port, they are 0."""
    if src.shape[1] == tw and src.shape[0] == th:
        return src.copy()
    scale_x = np.float32(tw) / np.float32(src.shape[1])
    scale_y = np.float32(th) / np.float32(src.shape[0])
    o_r = (np.arange(th, dtype=np.float32) / scale_x).astype(np.int64)
    o_c = (np.arange(tw, dtype=np.float32) / scale_y).astype(np.int64)
    dst = np.zeros((th, tw) + src.shape[2:], src.dtype)
    rr, cc = o_r < src.shape[0], o_c < src.shape[1]
    dst[np.ix_(rr, cc)] = src[np.ix_(o_r[rr], o_c[cc])]
    return dst


def lift(v, x, y, z):
    """Get3DPointonWorld (APD.cpp:501-524): x, y, z arrays -> [..., 3] world points."""
    K, R = v.K, v.R
    px = z * (x - K[2]) / K[0]
    py = z * (y - K[5]) / K[4]
    return np.stack([R[0] * px + R[3] * py + R[6] * z + v.C[0],
                     R[1] * px + R[4] * py + R[7] * z + v.C[1],
                     R[2] * px + R[5] * py + R[8] * z + v.C[2]], -1)


def project(v, X):
    """ProjectCamera (APD.cpp:536-546): -> (u, v, depth)."""
    R, t, K = v.R, v.t, v.K
    a = R[0] * X[..., 0] + R[1] * X[..., 1] + R[2] * X[..., 2] + t[0]
    b = R[3] * X[..., 0] + R[4] * X[..., 1] + R[5] * X[..., 2] + t[1]
    c = R[6] * X[..., 0] + R[7] * X[..., 1] + R[8] * X[..., 2] + t[2]
    d = K[6] * a + K[7] * b + K[8] * c
    with np.errstate(divide="ignore", invalid="ignore"):
        return (K[0] * a + K[1] * b + K[2] * c) / d, (K[3] * a + K[4] * b + K[5] * c) / d, d


def _trunc(t):
    # int(...) of a float: truncation toward zero; a value no int holds lands outside every image
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(t) & (np.abs(t) < 2.0 ** 30)
        return np.where(ok, np.trunc(np.where(ok, t, 0.0)), -1).astype(np.int64)


def get_angle(n1, n2):
    """GetAngle (APD.cpp:1797-1806): acos of the dot product, NaN (|dot| > 1) -> 0.  Also returns the margin of the binary32
    engine's value: how far acos moves when the dot product moves by EPS_DOT."""
    dot = np.sum(n1 * n2, -1)
    with np.errstate(invalid="ignore"):
        ang = np.where(np.abs(dot) <= 1, np.arccos(np.clip(dot, -1, 1)), 0.0)
        lo = np.where(dot + EPS_DOT < 1, np.arccos(np.clip(dot + EPS_DOT, -1, 1)), 0.0)
        hi = np.where(dot - EPS_DOT > -1, np.arccos(np.clip(dot - EPS_DOT, -1, 1)), math.pi)
    eps = np.maximum(hi - ang, ang - lo) + 2e-7
    return ang, eps


class Pair:
    """Every ref pixel of R against source S, vectorised (APD.cpp:1894-1925 / 2062-2090): the nearest source pixel, the three
    residuals and their margins, and whether the rounding to a pixel is certain."""

    def __init__(self, R, S, ys, xs):
        z = R.depth[ys, xs]
        X = lift(R, xs, ys, z)
        u, v, _ = project(S, X)
        tu, tv = u + 0.5, v + 0.5
        self.sx, self.sy = _trunc(tu), _trunc(tv)
        lo_x, hi_x, lo_y, hi_y = _trunc(tu - EPS_PX), _trunc(tu + EPS_PX), _trunc(tv - EPS_PX), _trunc(tv + EPS_PX)
        self.alts = [(ax, ay) for ax in (lo_x, hi_x) for ay in (lo_y, hi_y)]
        inside = lambda a, b: (a >= 0) & (a < S.cols) & (b >= 0) & (b < S.rows)
        self.inb = inside(self.sx, self.sy)
        self.round_unc = ((lo_x != hi_x) | (lo_y != hi_y)) & np.any([inside(a, b) for a, b in self.alts], 0)
        sxc, syc = np.where(self.inb, self.sx, 0), np.where(self.inb, self.sy, 0)
        self.sp = np.where(self.inb, syc * S.cols + sxc, -1)
        zs = S.depth[syc, sxc]
        self.zs_pos = self.inb & (zs > 0)
        Y = lift(S, sxc, syc, zs)
        bu, bv, zseen = project(R, Y)
        self.err = np.sqrt((xs - bu) ** 2 + (ys - bv) ** 2)
        self.rel = np.abs(zseen - z) / z
        self.ang, self.ang_eps = get_angle(R.normal[ys, xs], S.normal[syc, sxc])
        self.S = S
        self.scols, self.srows = S.cols, S.rows

    def alt_pixels(self, i):
        out = []
        for ax, ay in self.alts:
            if 0 <= ax[i] < self.scols and 0 <= ay[i] < self.srows:
                out.append(int(ay[i]) * self.scols + int(ax[i]))
        return out


def _test(value, eps, limit):
    """value < limit: 1 certainly, 0 certainly not, -1 within the margin"""
    if value < limit - eps:
        return 1
    if value >= limit + eps:
        return 0
    return -1


class State:
    """masks (APD.cpp:1868-1869 / 2022): claimed flags per view, and which of them are uncertain"""

    def __init__(self, views):
        self.claimed = [None if v is None else np.zeros(v.rows * v.cols, bool) for v in views]
        self.unc = [None if v is None else np.zeros(v.rows * v.cols, bool) for v in views]


def _ref_pixels(R):
    ys, xs = np.mgrid[0:R.rows, 0:R.cols]
    ok = R.depth > 0                                   # (APD.cpp:1889-1891: ref_depth <= 0.0 -> continue)
    if R.block is not None:
        ok &= ~(R.block < 128)                         # APD.cpp:1880-1882
    return ys[ok], xs[ok], np.flatnonzero(ok.reshape(-1))


def _new_stats():
    return dict(ref_pixels=0, uncertain=0, accepted=0, rej_reproj=0, rej_depth=0, rej_angle=0, rej_claimed=0, rej_vote=0)


def run_fusion(views, sources):
    """RunFusion (APD.cpp:1809-1960).  views: View or None (no maps) per slot in pair.txt order; sources: per slot, the slots of
    its listed sources (a slot may be the view itself).  Returns (records, stats): per fused or uncertain pixel, in the
    reference's output order, dict(view, pixel, certain, X, colour) — colour as the integer mean the PLY stores, None where
    not known exactly."""
    st = State(views)
    recs, stats = [], _new_stats()
    for i, R in enumerate(views):
        if R is None:
            continue
        ys, xs, pix = _ref_pixels(R)
        stats["ref_pixels"] += len(pix)
        src = [s for s in sources[i] if views[s] is not None]    # a source without maps never projects inside (cols = 0)
        pairs = [Pair(R, views[s], ys, xs) for s in src]
        for n in range(len(pix)):
            p = int(pix[n])
            y, x = int(ys[n]), int(xs[n])
            if st.claimed[i][p] and not st.unc[i][p]:
                continue                               # APD.cpp:1885-1887
            maybe_claimed = bool(st.unc[i][p])         # skipped or processed: the same when processing certainly rejects it
            unknown = False
            votes = votes_eps = 0.0
            wit = []
            rej = dict(rej_reproj=0, rej_depth=0, rej_angle=0, rej_claimed=0)
            for j, s in enumerate(src):
                P = pairs[j]
                if P.round_unc[n]:
                    unknown = True
                    continue
                if not P.inb[n]:
                    continue
                sp = int(P.sp[n])
                g = [_test(P.err[n], EPS_PX, 2.0), _test(P.rel[n], EPS_REL, 0.01), _test(P.ang[n], P.ang_eps[n], 0.174533)]
                could = P.zs_pos[n] and 0 not in g       # would be a witness if unclaimed
                if st.unc[s][sp]:
                    unknown = unknown or could
                    continue
                if st.claimed[s][sp]:                  # APD.cpp:1901-1902
                    rej["rej_claimed"] += int(bool(could))
                    continue
                if not P.zs_pos[n]:
                    continue
                if -1 in g and 0 not in g:
                    unknown = True
                    continue
                if 0 in g:
                    rej["rej_reproj"] += g[0] == 0
                    rej["rej_depth"] += g[1] == 0
                    rej["rej_angle"] += g[2] == 0
                    continue
                e = P.err[n] + 200 * P.rel[n] + 10 * P.ang[n]
                vote = math.exp(-e)
                votes += vote
                votes_eps += vote * (EPS_PX + 200 * EPS_REL + 10 * P.ang_eps[n]) + EPS_EXP * (len(src) + 1)
                wit.append((s, sp))
            factor = 0.45 if R.weak[y, x] == WEAK else 0.3
            nw = len(wit)
            if not unknown and nw >= 1 and abs(votes - factor * nw) <= votes_eps:
                unknown = True
            if maybe_claimed and (unknown or (nw >= 1 and votes > factor * nw)):
                unknown = True
            elif maybe_claimed:
                continue
            if unknown:
                stats["uncertain"] += 1
                recs.append(dict(view=i, pixel=p, certain=False, X=lift(R, x, y, R.depth[y, x])))
                for j, s in enumerate(src):            # whatever this pixel could claim
                    P = pairs[j]
                    if P.round_unc[n]:
                        cand = P.alt_pixels(n)
                    elif P.inb[n] and P.zs_pos[n] and 0 not in [_test(P.err[n], EPS_PX, 2.0), _test(P.rel[n], EPS_REL, 0.01), _test(P.ang[n], P.ang_eps[n], 0.174533)]:
                        cand = [int(P.sp[n])]
                    else:
                        cand = []
                    for q in cand:
                        if not st.claimed[s][q]:
                            st.unc[s][q] = True
                continue
            for k in rej:
                stats[k] += rej[k]
            if not (nw >= 1 and votes > factor * nw):
                stats["rej_vote"] += int(nw >= 1)
                continue
            stats["accepted"] += 1
            total = R.image[y, x].astype(np.int64).copy()
            for s, sp in wit:
                st.claimed[s][sp] = True                   # APD.cpp:1935-1940
                S = views[s]
                total += S.image[sp // S.cols, sp % S.cols]
            exact = R.image_exact and all(views[s].image_exact for s, _ in wit)
            recs.append(dict(view=i, pixel=p, certain=True, X=lift(R, x, y, R.depth[y, x]), colour=total // (nw + 1), colour_exact=exact))
    return recs, stats


def run_fusion_tat(views, sources, advanced):
    """RunFusion_TAT_Intermediate (advanced=False, APD.cpp:1962-2130) / RunFusion_TAT_advanced (True, :2132-2279).  The
    per-source residual records `diff` live for the whole view and are only overwritten when a source yields a comparison
    (APD.cpp:2051, 2082-2089): a source that drops out keeps voting with the residuals of the last pixel it was compared for."""
    dist_base = 0.25
    depth_base = 1.0 / 3000.0 if advanced else 1.0 / 3500.0
    angle_base, angle_grad = 0.06981317007977318, 0.05235987755982988
    st = State(views)
    recs, stats = [], _new_stats()
    for i, R in enumerate(views):
        if R is None:
            continue
        ys, xs, pix = _ref_pixels(R)
        stats["ref_pixels"] += len(pix)
        src = sources[i]                               # num_ngb counts every listed source (APD.cpp:2048)
        pairs = [None if views[s] is None else Pair(R, views[s], ys, xs) for s in src]
        ns = len(src)
        # diff[j]: the values the record may hold, each (err, rel, ang, ang_eps, source pixel); None: anything
        diff = [[(FLT_MAX, FLT_MAX, FLT_MAX, 0.0, -1)] for _ in range(ns)]
        for n in range(len(pix)):
            p = int(pix[n])
            y, x = int(ys[n]), int(xs[n])
            rej = dict(rej_reproj=0, rej_depth=0, rej_angle=0, rej_claimed=0)
            for j, s in enumerate(src):
                P = pairs[j]
                if P is None:
                    continue
                if P.round_unc[n]:
                    diff[j] = [None]                   # overwritten or not, and from which pixel
                    continue
                if not P.inb[n]:
                    continue
                sp = int(P.sp[n])
                fresh = (P.err[n], P.rel[n], P.ang[n], P.ang_eps[n], sp)
                if st.unc[s][sp]:
                    if P.zs_pos[n] and None not in diff[j]:   # overwritten or not
                        diff[j] = diff[j] + [fresh] if len(diff[j]) < 4 else [None]
                    continue
                if st.claimed[s][sp]:                  # APD.cpp:2073-2074
                    rej["rej_claimed"] += int(bool(P.zs_pos[n]))
                    continue
                if not P.zs_pos[n]:
                    continue
                diff[j] = [fresh]
                rej["rej_reproj"] += P.err[n] >= 2 * dist_base + EPS_PX
                rej["rej_depth"] += P.rel[n] >= 2 * depth_base + EPS_REL
                rej["rej_angle"] += (not advanced) and P.ang[n] >= 2 * angle_grad + angle_base + P.ang_eps[n]
            decision, use = 0, None                    # 0 reject, 1 accept, -1 uncertain
            for k in range(2, ns + 1):
                yes, unk = [], 0
                for j in range(ns):
                    out = set()
                    for d in diff[j]:
                        if d is None:
                            out.add(-1)
                            continue
                        g = [_test(d[0], EPS_PX, k * dist_base), _test(d[1], EPS_REL, k * depth_base)]
                        if not advanced:
                            g.append(_test(d[2], d[3], k * angle_grad + angle_base))
                        out.add(0 if 0 in g else (-1 if -1 in g else 1))
                    if out == {1}:
                        yes.append(j)
                    elif out != {0}:
                        unk += 1
                if len(yes) >= k:
                    decision, use = 1, (yes if unk == 0 and all(len(diff[j]) == 1 for j in yes) else None)
                    break
                if len(yes) + unk >= k:
                    decision = -1
                    break
            if decision == -1:
                stats["uncertain"] += 1
                st.unc[i][p] = True
                recs.append(dict(view=i, pixel=p, certain=False, X=lift(R, x, y, R.depth[y, x])))
                continue
            for k in rej:
                stats[k] += rej[k]
            if decision == 0:
                stats["rej_vote"] += 1
                continue
            stats["accepted"] += 1
            st.claimed[i][p] = True                    # APD.cpp:2118 / 2270: the pixel claims itself
            total = R.image[y, x].astype(np.int64).copy()
            exact = R.image_exact
            colour = total
            if not advanced:
                if use is None:
                    colour, exact = None, False
                else:
                    for j in use:
                        S = views[src[j]]
                        sp = diff[j][0][4]
                        total += S.image[sp // S.cols, sp % S.cols]
                        exact = exact and S.image_exact
                    colour = total // (len(use) + 1)
            recs.append(dict(view=i, pixel=p, certain=True, X=lift(R, x, y, R.depth[y, x]), colour=colour, colour_exact=exact))
    return recs, stats


def match(recs, xyz, bgr, scale, rel_tol=1e-5):
    """Walk the engine's point list (xyz [n, 3], bgr [n, 3] as the PLY stores them) against the model's records in output order:
    every certain record must be the next engine point, an uncertain one may be.  Coordinates must match to rel_tol * scale;
    colours exactly where the model knows them exactly (same-size maps and images), else within 1 per channel.
    Returns a list of problems (empty = agreement)."""
    bad = []
    tol = rel_tol * scale
    k = 0
    n = len(xyz)
    for r in recs:
        hit = k < n and np.abs(xyz[k].astype(np.float64) - r["X"]).max() <= tol
        if not hit:
            if r["certain"]:
                bad.append("view %d pixel %d: model keeps it, engine point %d is %s (model %s)" % (r["view"], r["pixel"], k, xyz[k] if k < n else None, r["X"]))
                if len(bad) > 10:
                    return bad
            continue
        if r["certain"] and r.get("colour") is not None:
            d = np.abs(bgr[k].astype(np.int64) - r["colour"])
            if d.max() > (0 if r["colour_exact"] else 1):
                bad.append("view %d pixel %d: colour %s, model %s" % (r["view"], r["pixel"], bgr[k], r["colour"]))
        k += 1
    if k != n:
        bad.append("engine has %d points after the model's last record (%d matched)" % (n - k, k))
    return bad
