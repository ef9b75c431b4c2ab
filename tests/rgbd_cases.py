"""The RGB-D frame path as a pure-Python / numpy-float32 restatement written from the reference
lines, and built cases that reach its edges on purpose (test_rgbd.py on the CPU, test_gpu_rgbd.py
against the kernels):

* `restated_stereo`  Frame::ComputeStereoFromRGBD (Frame.cc:759-780) on the raw depth image with
  the `convertTo(CV_32F, mDepthMapFactor)` of Tracking::GrabImageRGBD (Tracking.cc:367-368; the
  `if` in front of it ends in a semicolon, so the conversion always runs) applied per pixel: the
  literal lookup loop;
* `restated_close`   the literal sort-and-walk of Tracking::UpdateLastFrame (Tracking.cc:1059-1111)
  and CreateNewKeyFrame (1333-1392) with its nPoints counter, StereoInitialization's take-all
  (764-779), the counters of NeedNewKeyFrame (1256-1265), Frame::UnprojectStereo (Frame.cc:782-796)
  and the distances of the Frame-form MapPoint constructor (MapPoint.cc:298-305);
* `closed_prefix`    the closed form of the visited prefix the kernel uses in place of the walk.

Both restatements count the branches they take into an optional `stats` dict and take `mutant=`,
which flips exactly one decision (used only by the discrimination test).  Where the reference
reads out of bounds they report ORBFE_ERR_UNSUPPORTED and go on, as the library does.
"""
from __future__ import annotations

import math

import numpy as np

from orbslam_mapsave_amd.abi import KEYPOINT_DTYPE, ORBFE_ERR_UNSUPPORTED, ORBFE_OK

F32 = np.float32
CLOSE_SORTED, CLOSE_ALL = 0, 1
MIN_POINTS = 100  # the literal of Tracking.cc:1109 / 1389

STEREO_MUTANTS = ("round", "swap_rc", "lookup_undist", "ur_dist_x", "d_ge0")
CLOSE_MUTANTS = ("th_ge", "npoints_ge", "break_before", "tie_larger", "counter_le",
                 "all_reads_has_point", "float_norm", "assoc", "min_scale0")

# mDepthMapFactor after Tracking.cc:236-240: 1.0f / DepthMapFactor in float (0 reads as 1)
FACTOR_1000 = F32(1.0) / F32(1000.0)
FACTOR_5000 = F32(1.0) / F32(5000.0)
FACTORS = (FACTOR_1000, FACTOR_5000, F32(1.0), F32(5.0))


def _bump(st, key, n=1):
    if st is not None and n:
        st[key] = st.get(key, 0) + int(n)


def below(v):
    return np.nextafter(F32(v), F32(-np.inf))


def above(v):
    return np.nextafter(F32(v), F32(np.inf))


def keys_at(xs, ys, octaves=0):
    k = np.zeros(len(xs), KEYPOINT_DTYPE)
    k["x"], k["y"] = np.asarray(xs, F32), np.asarray(ys, F32)
    k["octave"] = octaves
    k["size"], k["angle"] = 31.0, 0.0
    return k


# ---- the conversion ---------------------------------------------------------------------------

def convert(raw, factor):
    """One element of convertTo(CV_32F, alpha): src * alpha + 0 as a float multiply."""
    with np.errstate(all="ignore"):
        return F32(F32(raw) * F32(factor))


def conversion_readings(raw: np.ndarray, factor) -> dict:
    """The three ways a build may evaluate src * alpha + 0 for an array of raw values."""
    f = F32(factor)
    with np.errstate(all="ignore"):
        a = raw.astype(F32) * f                                            # float multiply
        b = (raw.astype(np.float64) * np.float64(f)).astype(F32)           # double, then rounded
        c = (raw.astype(np.float64) * np.float64(f) + 0.0).astype(F32)     # fma(src, alpha, 0)
    return {"float_mul": a, "double_mul": b, "fma0": c}


# ---- Frame::ComputeStereoFromRGBD -------------------------------------------------------------

def _trunc(v):
    """(int)float: toward zero; None where the value has no int (NaN, beyond int)."""
    v = float(v)
    if math.isnan(v) or math.isinf(v) or abs(v) >= 2.0 ** 31:
        return None
    return int(v)


def _round(v):
    v = float(v)
    if math.isnan(v) or math.isinf(v) or abs(v) >= 2.0 ** 31:
        return None
    return int(math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1))


def restated_stereo(im_depth, factor, keys, keys_un, bf, stats=None, mutant=None):
    """Returns (mvuRight, mvDepth, status).  im_depth: the raw (h, w) uint16 / float32 image."""
    st = stats
    h, w = im_depth.shape
    n = len(keys)
    ku = keys if keys_un is None else keys_un
    bf = F32(bf)
    ur = np.full(n, -1, F32)   # 761
    dp = np.full(n, -1, F32)   # 762
    status = ORBFE_OK
    to_int = _round if mutant == "round" else _trunc
    for i in range(n):
        kp, kpu = keys[i], ku[i]
        src = kpu if mutant == "lookup_undist" else kp
        v, u = src["y"], src["x"]                       # 769-770
        row, col = to_int(v), to_int(u)                 # at<float>(v, u): row = y, column = x
        if mutant == "swap_rc":
            row, col = col, row
        if row is None or col is None or not (0 <= row < h and 0 <= col < w):
            _bump(st, "oob")
            status = ORBFE_ERR_UNSUPPORTED
            continue
        _bump(st, "frac", float(u) != col or float(v) != row)
        _bump(st, "neg_frac", float(u) < 0 or float(v) < 0)
        d = convert(im_depth[row, col], factor)         # 772 on the converted image
        ok = d >= 0 if mutant == "d_ge0" else d > 0     # 774
        _bump(st, "nan_depth", math.isnan(float(d)))
        if ok:
            _bump(st, "d_pos")
            _bump(st, "denormal", 0 < float(d) < float(np.finfo(F32).tiny))
            _bump(st, "un_distinct", kpu["x"] != kp["x"])
            dp[i] = d
            x = kp["x"] if mutant == "ur_dist_x" else kpu["x"]
            with np.errstate(all="ignore"):
                ur[i] = F32(x - F32(bf / d))            # 777
        else:
            _bump(st, "d_nonpos")
    return ur, dp, status


# ---- the close points -------------------------------------------------------------------------

def closed_prefix(depth, th, min_points):
    """Visited prefix of the sorted walk as a function of the depths alone: with M depths > 0,
    c of them not beyond th, the break fires after the first visit j >= max(c, min_points)."""
    z = np.asarray(depth, F32)
    with np.errstate(invalid="ignore"):
        kept = z > 0
        m = int(kept.sum())
        c = int((kept & ~(z > F32(th))).sum())
    return min(m, max(c, int(min_points)) + 1)


def unproject(kpu, z, cam, pose, mutant=None):
    """Frame::UnprojectStereo (Frame.cc:784-792); mRwc * x3Dc + mOw in the small-gemm order."""
    fx, fy, cx, cy = (F32(c) for c in cam)
    invfx, invfy = F32(1.0) / fx, F32(1.0) / fy
    u, v, z = F32(kpu["x"]), F32(kpu["y"]), F32(z)
    with np.errstate(all="ignore"):
        if mutant == "assoc":
            x = F32(F32(u - cx) * invfx) * z
            y = F32(F32(v - cy) * invfy) * z
        else:
            x = F32(F32(u - cx) * z) * invfx
            y = F32(F32(v - cy) * z) * invfy
        R = np.asarray(pose, F32)
        out = np.zeros(3, F32)
        for r in range(3):
            out[r] = F32(F32(F32(R[3 * r] * x) + F32(R[3 * r + 1] * y)) + F32(R[3 * r + 2] * z)) + R[9 + r]
    return out


def distances(p, pose, octave, scale, stats=None, mutant=None):
    """mfMaxDistance / mfMinDistance (MapPoint.cc:298-305); None where the octave indexes
    mvScaleFactors out of range."""
    ow = np.asarray(pose, F32)[9:]
    with np.errstate(all="ignore"):
        d = [F32(p[k] - ow[k]) for k in range(3)]
        if mutant == "float_norm":
            dist = F32(np.sqrt(F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))))
        else:  # cv::norm of a CV_32F vector accumulates in double
            s = 0.0
            for k in range(3):
                s += float(d[k]) * float(d[k])
            dist = F32(math.sqrt(s))
        if not 0 <= int(octave) < len(scale):
            _bump(stats, "octave_oob")
            return None
        mx = F32(dist * F32(scale[int(octave)]))
        mn = F32(mx / F32(scale[0 if mutant == "min_scale0" else len(scale) - 1]))
    return mx, mn


def restated_close(mode, keys_un, depth, has_point, cam, pose, th, min_points, scale,
                   stats=None, mutant=None):
    """Returns a dict like ORBmatcher.ClosePoints: order, create, xyz, max_dist, min_dist,
    n_visited, n_total, n_map, status.  scale None leaves the distances out."""
    st = stats
    n = len(depth)
    th = F32(th)
    depth = np.asarray(depth, F32)
    hp = np.zeros(n, bool) if has_point is None else np.asarray(has_point).astype(bool)
    status = ORBFE_OK
    # NeedNewKeyFrame's counters (1256-1265)
    n_total = n_map = 0
    for i in range(n):
        z = depth[i]
        if z > 0 and (z <= th if mutant == "counter_le" else z < th):
            n_total += 1
            _bump(st, "near")
            if hp[i]:
                n_map += 1
                _bump(st, "near_map")
    v = []
    for i in range(n):                                   # 1063-1070
        z = depth[i]
        if z > 0:
            v.append((float(z), i))
        else:
            _bump(st, "dropped")
    order, create, xyz, mxd, mnd = [], [], [], [], []

    def visit(z, i, new):
        nonlocal status
        order.append(i)
        create.append(1 if new else 0)
        p, d = np.zeros(3, F32), (F32(0), F32(0))
        if new:
            _bump(st, "created")
            p = unproject(keys_un[i], z, cam, pose, mutant)
            if scale is not None:
                d = distances(p, pose, keys_un[i]["octave"], scale, st, mutant)
                if d is None:
                    status = ORBFE_ERR_UNSUPPORTED
                    d = (F32(-1), F32(-1))
        else:
            _bump(st, "has_point")
        xyz.append(p)
        mxd.append(d[0])
        mnd.append(d[1])

    if mode == CLOSE_ALL:                                # 764-779
        for z, i in v:
            visit(z, i, not hp[i] if mutant == "all_reads_has_point" else True)
    elif v:                                              # 1072
        v.sort(key=(lambda t: (t[0], -t[1])) if mutant == "tie_larger" else None)   # 1075
        _bump(st, "tie", sum(1 for a, b in zip(v, v[1:]) if a[0] == b[0]))
        n_points = 0
        fired = False
        for j in range(len(v)):                          # 1080
            z, i = v[j]
            beyond = z >= float(th) if mutant == "th_ge" else z > float(th)
            if mutant == "break_before":
                if beyond and n_points > min_points:
                    fired = True
                    break
            visit(z, i, not hp[i])                       # 1084-1107: nPoints++ on both branches
            n_points += 1
            _bump(st, "beyond_visited", beyond)
            if mutant != "break_before" and beyond and \
                    (n_points >= min_points if mutant == "npoints_ge" else n_points > min_points):  # 1109
                fired = True
                break
        _bump(st, "break_fired", fired)
        _bump(st, "ran_out", not fired)
    nv = len(order)
    return {"order": np.asarray(order, np.int32).reshape(nv),
            "create": np.asarray(create, np.uint8).reshape(nv),
            "xyz": np.asarray(xyz, F32).reshape(nv, 3),
            "max_dist": None if scale is None else np.asarray(mxd, F32).reshape(nv),
            "min_dist": None if scale is None else np.asarray(mnd, F32).reshape(nv),
            "n_visited": nv, "n_total": n_total, "n_map": n_map, "status": status}


# ---- built cases ------------------------------------------------------------------------------

SCALE = np.asarray([F32(1.2) ** l for l in range(8)], F32)
SCALE[0] = 1.0
CAM = (F32(517.306408), F32(516.469215), F32(318.643040), F32(255.313989))  # TUM1.yaml
BF = F32(40.0)
TH = F32(40.0) * BF / CAM[0]   # mThDepth = mbf * ThDepth / fx (Tracking.cc:226)
IDENTITY = np.asarray([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)


def seeded_pose(seed):
    """A rotation (QR of a seeded matrix, rounded to float) and a camera centre."""
    r = np.random.default_rng(seed)
    q, _ = np.linalg.qr(r.normal(size=(3, 3)))
    return np.concatenate([q.reshape(9), r.normal(size=3) * 2.0]).astype(F32)


def stereo_cases():
    """name -> (im_depth, factor, keys, keys_un, bf)."""
    r = np.random.default_rng(7)
    c = {}
    w, h = 640, 480
    img = r.integers(0, 65536, (h, w)).astype(np.uint16)
    img[r.random((h, w)) < 0.15] = 0

    def rand_keys(n, ww=w, hh=h):
        return keys_at(r.random(n).astype(F32) * F32(ww - 1), r.random(n).astype(F32) * F32(hh - 1),
                       r.integers(0, 8, n))

    for n in (0, 1, 63, 64, 65, 257):
        c[f"u16_n{n}"] = (img, FACTOR_5000, rand_keys(n), None, BF)
    k = rand_keys(65)
    ku = k.copy()
    ku["x"] += r.normal(size=65).astype(F32) * F32(3)
    ku["y"] += r.normal(size=65).astype(F32) * F32(3)
    c["keys_un_distinct"] = (img, FACTOR_1000, k, ku, BF)
    # truncation edges: 12.999 -> 12, (-1, 0) -> 0, w - 0.5 -> w - 1, and their out-of-image kin
    small = r.integers(1, 65536, (5, 7)).astype(np.uint16)
    xs = [F32(2.999), F32(-0.5), below(0), above(-1), F32(6.5), below(7), F32(3.5), F32(0.5), F32(1.25), F32(5.75)]
    ys = [F32(1.999), F32(1.5), F32(-0.25), above(-1), F32(2.5), F32(0), below(5), F32(4.5), F32(-0.75), F32(3.25)]
    c["edges_in"] = (small, F32(1.0), keys_at(xs, ys), None, BF)
    xs = [F32(3), F32(7), F32(2), F32(-1), F32(1), F32(np.nan), F32(1e10), F32(4), F32(-3e9), F32(2), F32(6.5)]
    ys = [F32(2), F32(1), F32(5), F32(1), F32(-1), F32(1), F32(1), F32(np.inf), F32(2), F32(np.nan), F32(4.5)]
    c["edges_out"] = (small, F32(1.0), keys_at(xs, ys), None, BF)
    # a non-square image read with row / column swapped leaves it; a square one reads the transpose
    sq = r.integers(1, 65536, (6, 6)).astype(np.uint16)
    c["square"] = (sq, FACTOR_1000, keys_at([0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 0.2], [5.5, 3.5, 4.5, 0.5, 2.5, 1.5, 3.3]),
                   None, BF)
    # values: 0, 65535, and a factor that makes the product a denormal (bf / d = inf)
    vals = np.asarray([[0, 65535, 1, 2, 0, 40000, 7, 0]], np.uint16)
    kx = np.arange(8, dtype=F32) + F32(0.5)
    c["values_u16"] = (vals, FACTOR_5000, keys_at(kx, np.zeros(8, F32)), None, BF)
    c["values_denormal"] = (vals, F32(1e-41), keys_at(kx, np.zeros(8, F32)), None, BF)
    fv = np.asarray([[np.nan, -0.0, np.inf, -1.5, 0.0, 2.5, -np.inf, 1e-40, 3.25, np.nan, -0.0, 0.0],
                     [1.0, np.nan, -2.0, 0.0, 4.0, -0.0, 6.0, np.inf, -np.inf, 9.0, 1e-42, -1e-42]], F32)
    kx = np.concatenate([np.arange(12), np.arange(12)]).astype(F32) + F32(0.25)
    ky = np.concatenate([np.zeros(12), np.ones(12)]).astype(F32) + F32(0.75)
    c["values_f32"] = (fv, F32(1.0), keys_at(kx, ky), None, BF)
    c["values_f32_x5"] = (fv, F32(5.0), keys_at(kx, ky), None, BF)
    fimg = (r.random((48, 64)).astype(F32) * F32(8)) * (r.random((48, 64)) > 0.2)
    c["f32_n257"] = (fimg.astype(F32), F32(1.0), rand_keys(257, 64, 48), None, BF)
    # plane geometry: padded rows, 1 x 1, 3 x 2
    wide = r.integers(0, 65536, (9, 16)).astype(np.uint16)
    c["padded_u16"] = (wide[:, :11], FACTOR_5000, rand_keys(65, 11, 9), None, BF)
    widef = r.random((9, 16)).astype(F32)
    c["padded_f32"] = (widef[:, :13], F32(5.0), rand_keys(65, 13, 9), None, BF)
    c["one_pixel"] = (np.asarray([[1234]], np.uint16), FACTOR_1000,
                      keys_at([0, 0.5, -0.5, 1, 0.25], [0, 0.9, -0.9, 0, 1]), None, BF)
    c["three_by_two"] = (np.asarray([[1, 2, 3], [4, 0, 6]], np.uint16), F32(1.0),
                         keys_at([0.5, 1.5, 2.5, 0.5, 1.5, 2.5, 2.99, 3.0], [0.5, 0.5, 0.5, 1.5, 1.5, 1.5, 1.99, 1.0]),
                         None, BF)
    return c


def _close_case(depth, has_point, seed, pose=None, th=TH, min_points=MIN_POINTS, octaves=None):
    r = np.random.default_rng(seed)
    n = len(depth)
    k = keys_at(r.random(n).astype(F32) * F32(639), r.random(n).astype(F32) * F32(479),
                r.integers(0, 8, n) if octaves is None else octaves)
    return {"keys_un": k, "depth": np.asarray(depth, F32),
            "has_point": np.asarray(has_point, np.uint8), "cam": CAM,
            "pose": IDENTITY if pose is None else pose, "th": F32(th), "min_points": min_points,
            "scale": SCALE}


def depths_mc(r, n, m, c, th=TH):
    """n depths in a seeded order: c in (0, th], m - c beyond th, the rest dropped (<= 0, NaN)."""
    near = (r.random(c).astype(F32) * F32(0.98) + F32(0.01)) * F32(th)
    far = F32(th) * (F32(1.01) + r.random(m - c).astype(F32) * F32(4))
    junk = r.choice(np.asarray([0.0, -0.0, -1.0, -3.5, np.nan, -np.inf], F32), n - m)
    d = np.concatenate([near, far, junk]).astype(F32)
    return d[r.permutation(n)]


def close_cases():
    """name -> dict(keys_un, depth, has_point, cam, pose, th, min_points, scale)."""
    r = np.random.default_rng(11)
    c = {}

    def hp(n, p=0.4):
        return r.random(n) < p

    # M around min_points with everything near, and c around min_points with M above and below
    for m in (0, 1, 99, 100, 101, 102):
        c[f"M{m}_near"] = _close_case(depths_mc(r, m + 9, m, m), hp(m + 9), 100 + m)
        c[f"M{m}_far"] = _close_case(depths_mc(r, m + 9, m, 0), hp(m + 9), 200 + m)
    for cc in (99, 100, 101):
        for m in (cc, cc + 1, cc + 2, cc + 30):
            c[f"c{cc}_M{m}"] = _close_case(depths_mc(r, m + 20, m, cc), hp(m + 20), 300 + cc * 7 + m,
                                           pose=seeded_pose(cc + m))
    # exactly th and its two float neighbours, with M on both sides of the cut
    for k, edge in enumerate((below(TH), TH, above(TH))):
        for cc in (99, 100):
            d = depths_mc(r, 130, 120, cc)
            d[np.flatnonzero(d > TH)[0]] = edge
            c[f"th_edge{k}_c{cc}"] = _close_case(d, hp(130), 400 + k * 10 + cc)
        d = np.concatenate([np.full(3, edge, F32), r.random(20).astype(F32) * TH * F32(0.5) + F32(0.1),
                            np.full(4, F32(2) * TH, F32)])
        c[f"th_edge{k}_counters"] = _close_case(d, hp(len(d)), 450 + k, min_points=5)
    # runs of equal depths across the cut (the index breaks the tie)
    # six equal depths just beyond th are the first far ones: sorted positions cc .. cc + 5, and the
    # last visit is position max(cc, 100) = 100; eight equal near ones sit at 96 .. 103 of c = 104
    for cc in (96, 98, 100):
        d = np.sort(depths_mc(r, 120, 120, cc))
        d[cc:cc + 6] = TH * F32(1.005)
        c[f"ties_far_c{cc}"] = _close_case(d[r.permutation(120)], hp(120), 500 + cc, pose=seeded_pose(cc))
    d = np.sort(depths_mc(r, 120, 120, 104))
    d[96:104] = TH * F32(0.995)
    c["ties_near_c104"] = _close_case(d[r.permutation(120)], hp(120), 510, pose=seeded_pose(104))
    d = np.concatenate([np.full(60, F32(1.5), F32), np.full(60, TH * F32(3), F32)])[r.permutation(120)]
    c["ties_two_values"] = _close_case(d, hp(120), 520, min_points=70)
    # +inf depths sort last and unproject to inf / NaN
    d = depths_mc(r, 120, 110, 50)
    d[np.flatnonzero(d > TH)[:7]] = np.inf
    c["inf_depths"] = _close_case(d, np.zeros(120, bool), 530)
    d = np.concatenate([r.random(30).astype(F32) + F32(0.5), np.full(5, np.inf, F32)])
    c["inf_all_visited"] = _close_case(d, hp(35), 531)
    # every has_point pattern on the three visits around the cut (c = 100: visits 99, 100, 101)
    for bits in range(8):
        d = np.sort(depths_mc(r, 110, 110, 100))
        h = np.zeros(110, bool)
        h[99:102] = [(bits >> b) & 1 for b in range(3)]
        c[f"cut_pattern{bits}"] = _close_case(d, h, 540 + bits)
    # min_points 0 and 1, and th below every depth
    for mp in (0, 1):
        c[f"min_points{mp}_mixed"] = _close_case(depths_mc(r, 40, 30, 12), hp(40), 560 + mp, min_points=mp)
        c[f"min_points{mp}_far"] = _close_case(depths_mc(r, 40, 30, 0), hp(40), 570 + mp, min_points=mp)
    c["th_below_all"] = _close_case(r.random(150).astype(F32) + F32(1), hp(150), 580, th=F32(0.5))
    c["th_below_all_few"] = _close_case(r.random(60).astype(F32) + F32(1), hp(60), 581, th=F32(0.5))
    # sizes around the wave and the block
    for n in (63, 64, 65, 1024, 1025):
        c[f"n{n}"] = _close_case(depths_mc(r, n, n - n // 5, n // 3), hp(n), 600 + n, pose=seeded_pose(n))
    # an octave outside the pyramid on created and on skipped visits
    d = depths_mc(r, 60, 50, 40)
    o = r.integers(0, 8, 60)
    o[::7] = 8
    o[3::11] = -1
    c["octave_out"] = _close_case(d, hp(60), 620, octaves=o)
    return c


def big_close_case(kept, n=None, seed=0):
    """`kept` depths > 0 among n (for the 8,192 / 8,193 seam), a fifth of them near."""
    r = np.random.default_rng(900 + seed)
    n = kept + 50 if n is None else n
    return _close_case(depths_mc(r, n, kept, kept // 5), r.random(n) < 0.3, 901 + seed,
                       pose=seeded_pose(5), min_points=kept // 4)


def run_close(case, mode=CLOSE_SORTED, stats=None, mutant=None, dists=True):
    return restated_close(mode, case["keys_un"], case["depth"], case["has_point"], case["cam"],
                          case["pose"], case["th"], case["min_points"],
                          case["scale"] if dists else None, stats, mutant)


def same_bits(a, b):
    """Two results agree on every bit (floats compared as their bit patterns)."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
