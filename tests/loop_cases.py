"""The three matchers LoopClosing::ComputeSim3 calls, as pure-Python restatements written from
the reference lines, with the seeded inputs that reach their decisions on purpose:

  loop_sbp   SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)   ORBmatcher.cc:293-406
  sim3       SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) ORBmatcher.cc:1105-1329
  bow_kk     SearchByBoW(pKF1, pKF2, vpMatches12)                     ORBmatcher.cc:525-658

Every float expression is evaluated with np.float32 scalars in the written order; cv::norm and
Mat::dot accumulate in Python floats (double).  Each restatement counts the branches it takes
into an optional `stats` dict and takes `mutant=`, which flips exactly one decision (used only by
the discrimination test).  Shared pieces are imported, not restated twice: the projection block of
the loop SearchByProjection is fuse_cases.project (the Sim3 overload of Fuse has the same lines),
KeyFrame::GetFeaturesInArea is oracle.features_in_area, the rotation bin, ComputeThreeMaxima and
the FeatureVector helpers are triangulation_cases'.
"""
from __future__ import annotations

import copy
import functools
import math

import numpy as np

import fuse_cases as FC
import oracle
import scenarios as S
import triangulation_cases as TC
from orbslam_mapsave_amd.abi import Frame

F32 = np.float32
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30        # ORBmatcher.cc:37-39
INT_MAX = 2 ** 31 - 1
LOG_SCALE = FC.LOG_SCALE
SCALE = FC.SCALE

SBP_MUTANTS = ("ignore_dynamic", "ignore_preheld", "th_lt", "tie_last", "image_le", "no_angle",
               "level_plus1")
SIM3_MUTANTS = ("world_dist", "src_bounds", "src_tables", "tgt_filter", "kp_desc", "th_lt",
                "one_way", "angle")
BOW_MUTANTS = ("th_le", "no_mp2", "no_matched2", "second_over_blocked")

_bump = TC._bump
hamming = TC.hamming


def flip_exact(d, rng, nbits):
    """A copy of descriptor d with exactly nbits distinct bits flipped."""
    out = np.array(d, np.uint8, copy=True)
    for bit in rng.choice(256, size=nbits, replace=False):
        out[bit // 8] ^= np.uint8(1 << (bit % 8))
    return out


# ==== SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) =====================================

def _relaxed_bounds(kf: Frame) -> Frame:
    """kf with max_x / max_y one ulp up: u < nextafter(max) <=> u <= max (the non-strict mutant)."""
    k = copy.copy(kf)
    k.max_x = float(np.nextafter(F32(kf.max_x), F32(np.inf)))
    k.max_y = float(np.nextafter(F32(kf.max_y), F32(np.inf)))
    return k


def _sbp_point(c, i, ow, th, variant):
    """Lines 317-368 for point i: the projection block (fuse_cases.project) and the candidates of
    KeyFrame::GetFeaturesInArea with their octaves and distances.  variant: None, or the mutant
    that changes this block ("image_le", "no_angle")."""
    cc = c
    if variant == "image_le":
        cc = dict(c, kf=_relaxed_bounds(c["kf"]))
    p = FC.project(cc, i, ow)
    if p["reject"] == "angle" and variant == "no_angle":
        # the same point with its normal along PO: every other line of the block unchanged
        po = c["xyz"][i].astype(np.float64) - np.array([float(x) for x in ow])
        nn = c["normal"].copy()
        nn[i] = (po / np.linalg.norm(po)).astype(F32)
        p = FC.project(dict(c, normal=nn), i, ow)
    if p["reject"] is not None:
        return dict(reject=p["reject"])
    kf = c["kf"]
    lvl = p["lvl"]
    if lvl is None or lvl < 0 or lvl >= len(kf.scale_factors):
        return dict(reject="unsupported")
    r = F32(int(th)) * kf.scale_factors[lvl]                       # 363: th is an int
    idx = oracle.features_in_area(kf, float(p["u"]), float(p["v"]), float(r))   # 365
    return dict(reject=None, lvl=lvl, idx=idx, octave=kf.keys["octave"][idx],
                dist=hamming(c["desc"][i], kf.desc[idx]) if len(idx) else np.zeros(0, np.int32))


def loop_sbp(c, th, stats=None, mutant=None, points=None):
    """-> (vpMatched after the call, nmatches, per-point decision (-1: none), unsupported).
    c: kf, tcw (the normalised [R|t]), cam, log_scale, xyz, normal, min_dist, max_dist, desc,
    skip, ids (None: the index), matched0.  points: the _sbp_point results, when cached."""
    n = len(c["xyz"])
    ow = FC.camera_center(c["tcw"].astype(F32))
    variant = mutant if mutant in ("image_le", "no_angle") else None
    matched0 = c["matched0"]
    matched = matched0.copy()
    taken = set()
    dec = np.full(n, -1, np.int32)
    nmatches, bad = 0, False
    for i in range(n):                                              # 315
        if c["skip"][i]:                                            # 320
            _bump(stats, "skip")
            continue
        pt = points[i] if points is not None else _sbp_point(c, i, ow, th, variant)
        if pt["reject"] == "unsupported":
            _bump(stats, "unsupported")
            bad = True
            continue
        if pt["reject"] is not None:                                # 330-358
            _bump(stats, pt["reject"])
            continue
        if len(pt["idx"]) == 0:                                     # 367
            _bump(stats, "no_candidates")
            continue
        lvl = pt["lvl"]
        hi = lvl + 1 if mutant == "level_plus1" else lvl
        best, bi = 256, -1                                          # 373-374
        for idx, octave, d in zip(pt["idx"], pt["octave"], pt["dist"]):
            idx, d = int(idx), int(d)
            if matched0[idx] >= 0 and mutant != "ignore_preheld":   # 378, held before the call
                _bump(stats, "blocked_preheld")
                continue
            if idx in taken and mutant != "ignore_dynamic":         # 378, taken at 399
                _bump(stats, "blocked_dynamic")
                continue
            if octave < lvl - 1 or octave > hi:                     # 383
                _bump(stats, "level_reject")
                continue
            if d == best and bi >= 0:
                _bump(stats, "tie")
            if d < best or (mutant == "tie_last" and d == best and bi >= 0):   # 390
                best, bi = d, idx
        if best == TH_LOW:
            _bump(stats, "best_at_50")
        if best <= TH_LOW and not (mutant == "th_lt" and best == TH_LOW):      # 397
            matched[bi] = c["ids"][i] if c["ids"] is not None else i
            taken.add(bi)
            dec[i] = bi
            nmatches += 1
            _bump(stats, "accept")
        else:
            _bump(stats, "reject_gt_th" if bi >= 0 else "all_blocked")
    return matched, nmatches, dec, bad


def sbp_points(c, th, variant=None):
    """The per-point block of every point, for restatement runs that share it."""
    ow = FC.camera_center(c["tcw"].astype(F32))
    return [None if c["skip"][i] else _sbp_point(c, i, ow, th, variant)
            for i in range(len(c["xyz"]))]


def independent(c, th, points=None):
    """The Fuse-style answer: every point's best candidate with no blocking at all."""
    blind = dict(c, matched0=np.full(c["kf"].n, -1, np.int32))
    return loop_sbp(blind, th, mutant="ignore_dynamic", points=points)[2]


@functools.lru_cache(maxsize=None)
def sbp_case(seed=0, th=10, preheld=0.25):
    """fuse_case(seed)'s keyframe and points, mono; a quarter of the points listed a second time;
    a quarter of the keypoints hold a point before the call; built on purpose: points whose best
    free candidate is at distance exactly 50, pairs of keypoints with one descriptor inside a
    point's window (ties), a point exactly on the image's upper bound."""
    rng = np.random.Generator(np.random.PCG64(seed + 211))
    base = FC.fuse_case(seed, stereo=False, skip_rate=0.08)
    n0 = len(base["xyz"])
    order = np.concatenate([np.arange(n0), rng.choice(n0, n0 // 4, replace=False)])
    order = order[rng.permutation(len(order))]
    c = FC.subset(base, order)
    kf = c["kf"]
    kf.desc = kf.desc.copy()
    c["ids"] = (order + 7000).astype(np.int32)       # a point listed twice keeps its id
    c["matched0"] = np.where(rng.uniform(size=kf.n) < preheld,
                             rng.integers(20000, 30000, kf.n), -1).astype(np.int32)
    # 30 of the held slots hold points of the list: spAlreadyFound (309-310, 320)
    held = rng.choice(np.flatnonzero(c["matched0"] >= 0), 30, replace=False)
    c["matched0"][held] = rng.choice(c["ids"], 30, replace=False)
    c["bad"] = c["skip"].copy()                      # isBad()
    c["skip"] = (c["bad"].astype(bool) | np.isin(c["ids"], c["matched0"])).astype(np.uint8)
    c["th"] = th
    # craft on the restatement's own candidate lists
    pts = sbp_points(c, th)
    _, _, dec, _ = loop_sbp(c, th, points=pts)
    used = set()
    acc = [i for i in np.flatnonzero(dec >= 0)]
    rng.shuffle(acc)
    n50 = nt = 0
    for i in acc:
        if order[i] in used:
            continue
        pt = pts[i]
        free = [int(k) for k, o in zip(pt["idx"], pt["octave"])
                if c["matched0"][k] < 0 and pt["lvl"] - 1 <= o <= pt["lvl"] and k != dec[i]]
        if n50 < 8:
            d = flip_exact(kf.desc[dec[i]], rng, TH_LOW)
            c["desc"][order == order[i]] = d       # every listing of the point
            n50 += 1
            used.add(order[i])
        elif nt < 12 and free:
            kf.desc[free[0]] = kf.desc[dec[i]]
            nt += 1
            used.add(order[i])
    # a point exactly on the upper bound: its own u becomes the keyframe's max_x
    ow = FC.camera_center(c["tcw"].astype(F32))
    # (its keypoint is moved 7 pixels to the left, inside the window and off the last half cell,
    # whose keypoints PosInGrid drops)
    edge = max((i for i in np.flatnonzero(dec >= 0) if order[i] not in used),
               key=lambda i: float(FC.project(c, i, ow)["u"]))
    u_edge = FC.project(c, edge, ow)["u"]
    kf.keys = kf.keys.copy()
    kf.keys["x"][dec[edge]] = u_edge - F32(7.0)
    others = [i for i in range(len(order)) if not c["skip"][i] and
              FC.project(c, i, ow).get("u", F32(0)) == u_edge]
    c["edge"] = others
    kf.max_x = float(u_edge)
    kf.grid_w_inv = F32(Frame.GRID_COLS) / F32(kf.max_x - kf.min_x)
    return c


@functools.lru_cache(maxsize=None)
def chain_case(length=5):
    """A built chain: slots s0..s(L-1) side by side at level 0, points P0..P(L-1) projecting onto
    them (identity pose).  P0 is s0's descriptor; Pj (j >= 1) is at distance 6 from s(j-1), 10
    from sj and 22 or more from every other slot: P0 takes s0, P1 falls to s1, which P2 wanted,
    so P2 falls to s2, ... — a dependency chain of the list's whole length."""
    rng = np.random.Generator(np.random.PCG64(977))
    base = rng.integers(0, 256, 32, dtype=np.uint8)

    def region(j, nbits):   # the first nbits of bits [16 j, 16 j + 8)
        d = np.zeros(32, np.uint8)
        for b in range(16 * j, 16 * j + nbits):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d
    slots = np.stack([base ^ region(j, 8) for j in range(length)])
    pdesc = np.stack([slots[0]] + [slots[j - 1] ^ region(j, 6) for j in range(1, length)])
    x = 300.0 + 0.5 * np.arange(length)
    y = np.full(length, 200.0)
    keys = TC._keys(x, y, np.zeros(length, np.int32), np.zeros(length, F32))
    kf = Frame(keys, slots, S.W, S.H, SCALE)
    z = 4.0
    xyz = np.stack([np.full(length, (301.0 - S.CX) / S.FX * z),
                    np.full(length, (200.0 - S.CY) / S.FY * z), np.full(length, z)], 1)
    dist = np.linalg.norm(xyz, axis=1)
    maxd = (0.97 * dist).astype(F32)
    return dict(kf=kf, tcw=np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F32), cam=S.camera(),
                log_scale=LOG_SCALE, xyz=xyz.astype(F32), normal=(xyz / dist[:, None]).astype(F32),
                min_dist=(maxd / SCALE[7]).astype(F32), max_dist=maxd, desc=pdesc,
                skip=np.zeros(length, np.uint8), ids=None,
                matched0=np.full(length, -1, np.int32), th=10)


def sbp_subset(c, idx):
    """The case restricted to the points idx (any index expression)."""
    out = FC.subset(c, idx)
    for k in ("ids", "bad"):
        if c.get(k) is not None:
            out[k] = np.ascontiguousarray(c[k][idx])
    return out


def sbp_dense_case(seed=0):
    """sbp_case with every keypoint at octave 7 and every point predicted at level 7: the radius
    is 10 * 1.2^7 = 35.8 pixels and every keypoint in it passes the level window, so many points
    have more than 16 candidates."""
    c = dict(sbp_case(seed))
    kf = copy.copy(c["kf"])
    kf.keys = kf.keys.copy()
    kf.keys["octave"] = 7
    ow = np.array([float(x) for x in FC.camera_center(c["tcw"].astype(F32))])
    dist = np.linalg.norm(c["xyz"].astype(np.float64) - ow, axis=1)
    c["max_dist"] = (0.97 * dist * float(SCALE[7])).astype(F32)
    c["min_dist"] = (c["max_dist"] / SCALE[7]).astype(F32)
    c["kf"] = kf
    return c


def sbp_unsupported_case(seed=0, n_bad=6):
    """sbp_case with mfMaxDistance of n_bad matched points blown up: PredictScale leaves the
    pyramid for them (and the 1.2 window still holds them)."""
    c = dict(sbp_case(seed))
    _, _, dec, _ = loop_sbp(c, c["th"])
    hit = np.flatnonzero(dec >= 0)[:n_bad]
    c["max_dist"] = c["max_dist"].copy()
    c["max_dist"][hit] *= F32(8.0)
    c["hit"] = hit
    return c


# ==== SearchBySim3 ==============================================================================

def sim3_mats(s12, R12, t12):
    """Lines 1122-1124 as the C++ adapter evaluates them -> the row-major 3 x 4
    [sR12|t12] and [sR21|t21]."""
    s12 = F32(s12)
    R12 = np.asarray(R12, F32).reshape(3, 3)
    t12 = np.asarray(t12, F32).reshape(3)
    S12 = np.zeros((3, 4), F32)
    S21 = np.zeros((3, 4), F32)
    inv = F32(1.0 / float(s12))
    for r in range(3):
        for k in range(3):
            S12[r, k] = s12 * R12[r, k]
            S21[r, k] = R12[k, r] * inv
        S12[r, 3] = t12[r]
    for r in range(3):
        S21[r, 3] = -((S21[r, 0] * t12[0] + S21[r, 1] * t12[1]) + S21[r, 2] * t12[2])
    return S12, S21


def _rigid(T, p):
    return [((T[r, 0] * p[0] + T[r, 1] * p[1]) + T[r, 2] * p[2]) + T[r, 3] for r in range(3)]


def _sim3_direction(c, a, b, Tsw, Sts, st, mutant, tgt_matched):
    """Lines 1151-1228 (a = 1, b = 2) or 1231-1308 (a = 2, b = 1): the points of keyframe a into
    keyframe b -> vnMatch of a, unsupported."""
    src, tgt = c["kf%d" % a], c["kf%d" % b]
    P = c["pts%d" % a]
    cam = c["cam1"]                                  # pKF1's intrinsics in both directions
    fx, fy, cx, cy = F32(cam.fx), F32(cam.fy), F32(cam.cx), F32(cam.cy)
    bounds_kf = src if mutant == "src_bounds" else tgt
    tab_kf, tab_log = (src, c["log%d" % a]) if mutant == "src_tables" else (tgt, c["log%d" % b])
    vn = np.full(src.n, -1, np.int32)
    bad = False
    Tsw = Tsw.astype(F32)
    ow_t = FC.camera_center(c["T%dw" % b].astype(F32))
    with np.errstate(all="ignore"):
        for i in range(src.n):
            if not c["search%d" % a][i]:             # 1155-1159
                _bump(st, "not_searched")
                continue
            Pw = P["xyz"][i]
            p1 = _rigid(Tsw, Pw)                     # 1162
            p2 = _rigid(Sts, p1)                     # 1163
            if p2[2] < F32(0.0):                     # 1166
                _bump(st, "depth")
                continue
            invz = F32(np.float64(1.0) / np.float64(p2[2]))   # 1169: a double divide
            x, y = p2[0] * invz, p2[1] * invz
            u, v = fx * x + cx, fy * y + cy
            k = bounds_kf
            if not (u >= F32(k.min_x) and u < F32(k.max_x) and v >= F32(k.min_y) and v < F32(k.max_y)):
                _bump(st, "image")                   # 1177
                continue
            d3 = F32(math.sqrt(sum(float(q) * float(q) for q in p2)))    # 1182
            if mutant == "world_dist":
                d3 = F32(math.sqrt(sum((float(Pw[j]) - float(ow_t[j])) ** 2 for j in range(3))))
            if d3 < F32(0.8) * P["min_dist"][i] or d3 > F32(1.2) * P["max_dist"][i]:   # 1185
                _bump(st, "distance")
                continue
            if mutant == "angle":
                po = [float(Pw[j]) - float(ow_t[j]) for j in range(3)]
                if sum(po[j] * float(P["normal"][i][j]) for j in range(3)) < 0.5 * math.sqrt(
                        sum(q * q for q in po)):
                    continue
            ratio = P["max_dist"][i] / d3            # MapPoint::PredictScale, no clamp (H8)
            lvl = int(math.ceil(F32(math.log(float(ratio))) / F32(tab_log)))
            if lvl < 0 or lvl >= len(tab_kf.scale_factors):
                _bump(st, "unsupported")
                bad = True
                continue
            r = F32(c["th"]) * tab_kf.scale_factors[lvl]       # 1192
            idx = oracle.features_in_area(tgt, float(u), float(v), float(r))
            if len(idx) == 0:                        # 1196
                _bump(st, "no_candidates")
                continue
            q = src.desc[i] if mutant == "kp_desc" else P["desc"][i]   # 1200
            dist = hamming(q, tgt.desc[idx])
            best, bi = INT_MAX, -1
            for j, octave, d in zip(idx, tgt.keys["octave"][idx], dist):
                if mutant == "tgt_filter" and tgt_matched[j]:
                    continue
                if octave < lvl - 1 or octave > lvl:           # 1210
                    _bump(st, "level_reject")
                    continue
                d = int(d)
                if d == best:
                    _bump(st, "tie")
                if d < best:                         # 1217
                    best, bi = d, int(j)
            if best == TH_HIGH:
                _bump(st, "best_at_100")
            if best <= TH_HIGH and not (mutant == "th_lt" and best == TH_HIGH):   # 1224
                vn[i] = bi
                _bump(st, "accept")
            else:
                _bump(st, "reject_gt_th")
    return vn, bad


def masks(c):
    """vbAlreadyMatched1 / 2 (1135-1145) and the two `search` masks the ABI takes."""
    n1, n2 = c["kf1"].n, c["kf2"].n
    am1 = c["matches12"] >= 0
    am2 = np.zeros(n2, bool)
    for i in np.flatnonzero(am1):
        idx2 = c["index_in_kf2"].get(int(c["matches12"][i]), -1)
        if 0 <= idx2 < n2:                           # 1142
            am2[idx2] = True
    s1 = (c["pts1"]["ids"] >= 0) & ~c["pts1"]["bad"].astype(bool) & ~am1
    s2 = (c["pts2"]["ids"] >= 0) & ~c["pts2"]["bad"].astype(bool) & ~am2
    return am1, am2, s1.astype(np.uint8), s2.astype(np.uint8)


def sim3(c, stats=None, mutant=None):
    """-> (match12 (idx2 per KF1 feature, -1), vnMatch1, vnMatch2, nFound, unsupported)."""
    am1, am2, s1, s2 = masks(c)
    c = dict(c, search1=s1, search2=s2)
    S12, S21 = sim3_mats(c["s12"], c["R12"], c["t12"])
    vn1, b1 = _sim3_direction(c, 1, 2, c["T1w"], S21, stats, mutant, am2)
    vn2, b2 = _sim3_direction(c, 2, 1, c["T2w"], S12, stats, mutant, am1)
    m12 = np.full(c["kf1"].n, -1, np.int32)
    for i1 in range(c["kf1"].n):                     # 1313-1326
        idx2 = vn1[i1]
        if idx2 >= 0:
            if vn2[idx2] == i1 or mutant == "one_way":
                m12[i1] = idx2
                _bump(stats, "agree")
            else:
                _bump(stats, "disagree")
    return m12, vn1, vn2, int((m12 >= 0).sum()), b1 or b2


def _inv_rigid(T):
    R, t = T[:, :3].astype(np.float64), T[:, 3].astype(np.float64)
    return R.T, -R.T @ t


def _points_for(kf, rng, T_w, depth_to_other, other_scale, other_nlevels):
    """The map points kf's features hold: along the feature's ray at depth U[2, 8] in kf's camera
    frame, 8 % clutter anywhere, mfMaxDistance from the distance in the OTHER camera
    (depth_to_other) so that the level predicted there is the feature's octave, clipped to the
    other keyframe's pyramid."""
    n = kf.n
    z = rng.uniform(2.0, 8.0, n)
    pc = np.stack([(kf.keys["x"] - S.CX) / S.FX * z, (kf.keys["y"] - S.CY) / S.FY * z, z], 1)
    clutter = rng.uniform(size=n) < 0.08
    pc[clutter] = np.stack([rng.uniform(-6, 6, clutter.sum()), rng.uniform(-5, 5, clutter.sum()),
                            rng.uniform(-2, 12, clutter.sum())], 1)
    Rwc, twc = _inv_rigid(T_w)
    xyz = pc @ Rwc.T + twc
    d_other = depth_to_other(pc)
    lvl = np.minimum(kf.keys["octave"], other_nlevels - 1)
    maxd = (0.97 * d_other * other_scale[lvl]).astype(F32)
    maxd[rng.uniform(size=n) < 0.03] *= F32(0.5)     # outside the 1.2 window
    normal = (xyz - twc) / np.linalg.norm(xyz - twc, axis=1, keepdims=True) + rng.normal(0, 0.5, (n, 3))
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    ids = np.where(rng.uniform(size=n) < 0.9, np.arange(n), -1).astype(np.int32)
    return dict(ids=ids, bad=(rng.uniform(size=n) < 0.04).astype(np.uint8),
                xyz=np.ascontiguousarray(xyz, F32), min_dist=(maxd / other_scale[-1]).astype(F32),
                max_dist=maxd, desc=S.flip_bits(kf.desc, rng, 0.06),
                normal=np.ascontiguousarray(normal, F32))


@functools.lru_cache(maxsize=None)
def sim3_case(seed=0, nfeatures=1000, mixed=False, th=7.5):
    """Two keyframes of one scene: KF2's image is KF1's shifted by (3, 2) pixels and the Sim3
    between the cameras is a rotation of about that shift with scale 1.3 (the scale moves the
    depth, not the projection).  mixed: KF2 has its own image bounds (600 x 440) and its own
    pyramid (6 levels of 1.25), so the source's bounds or tables give other answers.  Built on
    purpose: points at distance exactly 100 from their match, ids already in vpMatches12."""
    rng = np.random.Generator(np.random.PCG64(seed + 311))
    kf1 = S.extract_frame(seed, nfeatures)
    k2 = S.extract_frame(seed, nfeatures, shift=(2, 3))
    scale2, log2 = SCALE, LOG_SCALE
    if mixed:
        scale2 = (F32(1.25) ** np.arange(6, dtype=F32)).astype(F32)
        log2 = float(np.log(F32(1.25)).astype(F32))
        keys = k2.keys.copy()
        keys["octave"] = np.minimum(keys["octave"], 5)
        kf2 = Frame(keys, k2.desc, 600, 440, scale2)
    else:
        kf2 = Frame(k2.keys, k2.desc, S.W, S.H, scale2)
    kf1.desc, kf2.desc = kf1.desc.copy(), kf2.desc.copy()
    s12 = F32(1.3)
    ay, ax = 3.0 / S.FX, -2.0 / S.FY                # p2 = R21 p1 shifts u by +3, v by +2
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    R21 = Ry @ Rx
    R12 = R21.T.astype(F32)
    t12 = np.array([0.006, -0.004, 0.01], F32)
    T1w = S.pose(rng, 0.05, 0.3)
    T2w = S.pose(rng, 0.08, 0.5)
    S12, S21 = (m.astype(np.float64) for m in sim3_mats(s12, R12, t12))
    pts1 = _points_for(kf1, rng, T1w, lambda pc: np.linalg.norm(pc @ S21[:, :3].T + S21[:, 3], axis=1),
                       kf2.scale_factors, len(kf2.scale_factors))
    pts2 = _points_for(kf2, rng, T2w, lambda pc: np.linalg.norm(pc @ S12[:, :3].T + S12[:, 3], axis=1),
                       kf1.scale_factors, len(kf1.scale_factors))
    pts2["ids"] = np.where(pts2["ids"] >= 0, pts2["ids"] + 50000, -1).astype(np.int32)
    c = dict(kf1=kf1, kf2=kf2, cam1=S.camera(), T1w=T1w, T2w=T2w, s12=s12, R12=R12, t12=t12,
             log1=LOG_SCALE, log2=log2, pts1=pts1, pts2=pts2, th=th,
             matches12=np.full(kf1.n, -1, np.int32), index_in_kf2={})
    # craft on the restatement's own answers: distance exactly 100, then the prior matches
    m12, vn1, vn2, _, _ = sim3(c)
    agreed = np.flatnonzero(m12 >= 0)
    rng.shuffle(agreed)
    for i1 in agreed[:8]:
        pts1["desc"][i1] = flip_exact(kf2.desc[m12[i1]], rng, TH_HIGH)
    for i1 in agreed[8:8 + 40]:                     # already matched (by SearchByBoW) pairs
        c["matches12"][i1] = pts2["ids"][m12[i1]]
    c["index_in_kf2"] = {int(pts2["ids"][i]): int(i) for i in np.flatnonzero(pts2["ids"] >= 0)}
    c["index_in_kf2"][int(pts2["ids"][m12[agreed[9]]])] = kf2.n + 3      # outside [0, N2) (1142)
    c["index_in_kf2"][int(pts2["ids"][m12[agreed[10]]])] = -1            # not in pKF2
    return c


def sim3_unsupported_case(seed=0, n_bad=6):
    """sim3_case with mfMaxDistance of n_bad agreeing KF1 points blown up: PredictScale leaves
    KF2's pyramid for them (and the 1.2 window still holds them)."""
    c = dict(sim3_case(seed))
    hit = np.flatnonzero(sim3(c)[0] >= 0)[:n_bad]
    c["pts1"] = dict(c["pts1"], max_dist=c["pts1"]["max_dist"].copy())
    c["pts1"]["max_dist"][hit] *= F32(8.0)
    c["hit"] = hit
    return c


def sim3_subset(c, n1, n2):
    """The case cut to its first n1 / n2 features."""
    def cut(kf, n):
        f = Frame(kf.keys[:n], kf.desc[:n], 1, 1, kf.scale_factors)
        for k in ("min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv"):
            setattr(f, k, getattr(kf, k))
        return f
    out = dict(c, kf1=cut(c["kf1"], n1), kf2=cut(c["kf2"], n2),
               pts1={k: v[:n1] for k, v in c["pts1"].items()},
               pts2={k: v[:n2] for k, v in c["pts2"].items()},
               matches12=c["matches12"][:n1].copy())
    return out


# ==== SearchByBoW(pKF1, pKF2, vpMatches12) ======================================================

def bow_kk(c, nnratio=0.75, check_ori=True, stats=None, mutant=None):
    """-> (matches12 (idx2 per KF1 feature, -1), nmatches)."""
    d1, d2 = c["desc1"], c["desc2"]
    ok1, ok2 = c["ok1"], c["ok2"]
    ids1, off1, feat1 = c["fv1"]
    ids2, off2, feat2 = c["fv2"]
    m12 = np.full(len(d1), -1, np.int32)             # 537
    matched2 = np.zeros(len(d2), bool)               # 538
    hist = {}
    nmatches = 0
    i = j = 0
    while i < len(ids1) and j < len(ids2):           # 553
        if ids1[i] == ids2[j]:
            _bump(stats, "node_common")
            cand = feat2[off2[j]:off2[j + 1]]
            for idx1 in feat1[off1[i]:off1[i + 1]]:  # 557
                if not ok1[idx1]:                    # 561-565
                    _bump(stats, "kf1_no_mp")
                    continue
                dists = hamming(d1[idx1], d2[cand]) if len(cand) else []
                best1, bi, best2 = 256, -1, 256      # 569-571
                blocked_min = 256
                for r, idx2 in enumerate(cand):      # 573
                    d = int(dists[r])
                    if matched2[idx2] and mutant != "no_matched2":      # 579
                        _bump(stats, "c2_blocked")
                        blocked_min = min(blocked_min, d)
                        continue
                    if not ok2[idx2] and mutant != "no_mp2":            # 579-583
                        _bump(stats, "c2_no_mp")
                        continue
                    if d < best1:                    # 589
                        best2, best1, bi = best1, d, int(idx2)
                    elif d < best2:                  # 595
                        best2 = d
                if mutant == "second_over_blocked":  # a blocked candidate still sets bestDist2
                    best2 = min(best2, blocked_min)
                if best1 in (TH_LOW - 1, TH_LOW):
                    _bump(stats, "best_at_%d" % best1)
                if best1 < TH_LOW or (mutant == "th_le" and best1 == TH_LOW):   # 601
                    if F32(best1) < F32(nnratio) * F32(best2):                 # 603
                        m12[idx1] = bi
                        matched2[bi] = True
                        if check_ori:                # 608-618 (H15)
                            b = TC.rot_bin(c["angle1"][idx1], c["angle2"][bi], stats)
                            hist.setdefault(b, []).append(int(idx1))
                        nmatches += 1
                        _bump(stats, "match")
                    else:
                        _bump(stats, "ratio_reject")
                else:
                    _bump(stats, "th_reject")
            i += 1
            j += 1
        elif ids1[i] < ids2[j]:                      # 627-630
            _bump(stats, "node_skip1")
            i = TC._lower_bound(ids1, i, ids2[j])
        else:
            _bump(stats, "node_skip2")
            j = TC._lower_bound(ids2, j, ids1[i])
    if check_ori:                                    # 637-655
        top = TC.three_maxima([len(hist.get(b, ())) for b in range(HISTO_LENGTH)])
        for b in sorted(hist):
            if b in top:
                continue
            for idx1 in hist[b]:
                m12[idx1] = -1
                nmatches -= 1
                _bump(stats, "ori_dropped")
    return m12, nmatches


# angle differences and their shares: bins 2, 3 and 5 lead, bin 8 (240) is dropped; -300 wraps
ROT_CLASSES = ((60.0, 0.5), (90.0, 0.2), (150.0, 0.15), (-300.0, 0.05), (240.0, 0.1))


@functools.lru_cache(maxsize=None)
def bow_case(seed=0, nodes=70):
    """Built, never extracted (as triangulation_cases): quantised descriptors — a group's base
    with pk bits flipped in its first half for a KF2 feature and pq bits in its second half for a
    KF1 feature, so distance = pk + pq within a group and about 128 across.  Each node holds a few
    groups.  By construction: pairs at distance exactly 49 and 50, KF2 features without a live
    point that would be the best candidate, two KF1 features wanting one KF2 feature with a
    second clone behind it (close enough that a blocked clone's distance spoils the ratio test),
    KF1 features without a live point, nodes on one side only."""
    rng = np.random.Generator(np.random.PCG64(seed + 411))
    d1, d2, n1, n2, a1, a2, ok1, ok2 = [], [], [], [], [], [], [], []
    cls = np.array([r for r, _ in ROT_CLASSES])
    pr = np.array([p for _, p in ROT_CLASSES])

    def add1(base, pq, node, ang, ok=1):
        d1.append(TC._flip(base, rng, pq, 1)); n1.append(node); a1.append(ang); ok1.append(ok)

    def add2(base, pk, node, ang, ok=1):
        d2.append(TC._flip(base, rng, pk, 0)); n2.append(node); a2.append(ang); ok2.append(ok)
    for node in range(nodes):
        nid = 10 + 3 * node
        if node % 9 == 7:                            # a node KF2 does not have
            for _ in range(3):
                add1(TC._bases(rng, 1)[0], 3, nid, 10.0)
            continue
        if node % 9 == 8:                            # a node KF1 does not have
            for _ in range(3):
                add2(TC._bases(rng, 1)[0], 3, nid, 10.0)
            continue
        for g in range(int(rng.integers(2, 6))):
            base = TC._bases(rng, 1)[0]
            ang2 = float(rng.uniform(0, 360))
            rot = float(rng.choice(cls, p=pr))
            ang1 = ang2 + rot
            kind = (node * 5 + g) % 10
            if kind == 0:                            # distance exactly 49: matched
                add2(base, 20, nid, ang2); add1(base, 29, nid, ang1)
            elif kind == 1:                          # distance exactly 50: not matched (strict <)
                add2(base, 20, nid, ang2); add1(base, 30, nid, ang1)
            elif kind == 2:                          # the best KF2 clone holds no live point
                add2(base, 2, nid, ang2, ok=0); add2(base, 30, nid, ang2); add1(base, 4, nid, ang1)
            elif kind == 3:                          # contention: two KF1 features, clones 4 / 9
                add2(base, 4, nid, ang2); add2(base, 9, nid, ang2)
                add1(base, 3, nid, ang1); add1(base, 5, nid, ang1)
            elif kind == 4:                          # KF1 feature without a live point
                add2(base, 5, nid, ang2); add1(base, 5, nid, ang1, ok=0)
            elif kind == 5:                          # ratio test fails: clones 10 / 11
                add2(base, 10, nid, ang2); add2(base, 11, nid, ang2); add1(base, 6, nid, ang1)
            else:
                add2(base, int(rng.integers(2, 12)), nid, ang2)
                add1(base, int(rng.integers(2, 12)), nid, ang1)
    p1, p2 = rng.permutation(len(d1)), rng.permutation(len(d2))
    n1, n2 = np.array(n1)[p1], np.array(n2)[p2]
    return dict(desc1=np.stack(d1)[p1], desc2=np.stack(d2)[p2],
                angle1=np.array(a1, F32)[p1], angle2=np.array(a2, F32)[p2],
                ok1=np.array(ok1, np.uint8)[p1], ok2=np.array(ok2, np.uint8)[p2],
                fv1=TC.feature_vector(n1, len(n1)), fv2=TC.feature_vector(n2, len(n2)))


def bow_seam_case(ny, seed=0):
    """One common node holding ny KF2 features (the wave's 64-lane registers: 63 / 64 / 65 / 256,
    and 257 over the limit) and 12 KF1 features cloned from KF2 features spread over the node's
    ranks, the last rank included; a second, small node beside it."""
    rng = np.random.Generator(np.random.PCG64(seed + 511 + ny))
    d2 = TC._bases(rng, ny + 4)
    pick = np.unique(np.concatenate([[0, ny - 1], rng.integers(0, ny, 10)]))
    d1 = np.stack([TC._flip(d2[k], rng, int(rng.integers(1, 9)), 1) for k in pick] +
                  [TC._flip(d2[ny + 1], rng, 3, 1)])
    n2 = np.array([5] * ny + [9] * 4)
    n1 = np.array([5] * len(pick) + [9])
    ok2 = np.ones(ny + 4, np.uint8)
    ok2[pick[len(pick) // 2]] = 0
    return dict(desc1=d1, desc2=d2, angle1=np.zeros(len(d1), F32),
                angle2=np.zeros(ny + 4, F32), ok1=np.ones(len(d1), np.uint8), ok2=ok2,
                fv1=TC.feature_vector(n1, len(n1)), fv2=TC.feature_vector(n2, len(n2)))


def bow_item(c, side):
    """(desc, angle, ok, fv) of one side, the slot tuple of test_bow.pack_slots."""
    return c["desc%d" % side], c["angle%d" % side], c["ok%d" % side], c["fv%d" % side]


# ==== the case files of tests/cpp/loop_test.cpp =================================================

def _dump_frame(f, kf):
    np.array([kf.n, len(kf.scale_factors)], np.int32).tofile(f)
    np.array([kf.min_x, kf.max_x, kf.min_y, kf.max_y], F32).tofile(f)
    kf.scale_factors.astype(F32).tofile(f)
    kf.keys.tofile(f)
    kf.desc.tofile(f)


def _dump_points(f, p):
    p["ids"].astype(np.int32).tofile(f)
    p["bad"].astype(np.uint8).tofile(f)
    for k in ("xyz", "min_dist", "max_dist"):
        p[k].astype(F32).tofile(f)
    p["desc"].tofile(f)


def _dump_fv(f, fv):
    ids, off, feat = fv
    np.array([len(ids), len(feat)], np.int32).tofile(f)
    for a in fv:
        np.asarray(a, np.int32).tofile(f)


def dump_case(path, sbp, scw, s3, bow):
    """sbp: a loop_sbp case with scw its un-normalised 3 x 4 Sim3 (sbp["tcw"] =
    fuse_cases.sim3_normalise(scw)); its skip bytes are isBad() alone: the adapter builds
    spAlreadyFound itself.  s3: a sim3 case; bow: a bow_kk case."""
    with open(path, "wb") as f:
        cam = sbp["cam"]
        np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.bf, cam.b], F32).tofile(f)
        _dump_frame(f, sbp["kf"])
        np.array([len(sbp["xyz"]), sbp["th"]], np.int32).tofile(f)
        np.array([sbp["log_scale"]], F32).tofile(f)
        scw.astype(F32).tofile(f)
        for k in ("xyz", "normal", "min_dist", "max_dist"):
            sbp[k].astype(F32).tofile(f)
        sbp["desc"].tofile(f)
        sbp["bad"].astype(np.uint8).tofile(f)
        sbp["ids"].astype(np.int32).tofile(f)
        sbp["matched0"].astype(np.int32).tofile(f)
        # SearchBySim3
        _dump_frame(f, s3["kf1"])
        _dump_frame(f, s3["kf2"])
        _dump_points(f, s3["pts1"])
        _dump_points(f, s3["pts2"])
        for k in ("T1w", "T2w", "R12", "t12"):
            s3[k].astype(F32).tofile(f)
        np.array([s3["s12"], s3["th"], s3["log1"], s3["log2"]], F32).tofile(f)
        s3["matches12"].astype(np.int32).tofile(f)
        idx = np.array(sorted(s3["index_in_kf2"].items()), np.int32).reshape(-1, 2)
        np.array([len(idx)], np.int32).tofile(f)
        idx.tofile(f)
        # SearchByBoW
        for side in (1, 2):
            d = bow["desc%d" % side]
            np.array([len(d)], np.int32).tofile(f)
            d.tofile(f)
            bow["angle%d" % side].astype(F32).tofile(f)
            bow["ok%d" % side].astype(np.uint8).tofile(f)
            _dump_fv(f, bow["fv%d" % side])
