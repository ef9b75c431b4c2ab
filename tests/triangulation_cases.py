"""ORBmatcher::SearchForTriangulation (ORBmatcher.cc:660-826) with CheckDistEpipolarLine
(140-157) and ComputeThreeMaxima (1604-1645) as a pure-Python restatement written from those
lines, and seeded inputs that reach its decisions on purpose.

The restatement walks the two FeatureVectors as the reference does, serves each common node's
keyframe-1 features in order, computes its own Hamming distances and evaluates every float
expression with np.float32 scalars in the written order; the 3.84 test is a Python-float (double)
comparison.  `block` selects what vbMatched2 does: the reference declares it (680), reads it (728)
and never writes it, so block=False is the source as written and block=True its evident intent
(vbMatched2[bestIdx2] = true after 764, never released).  It counts the branches it takes into an
optional `stats` dict and takes `mutant=`, which flips exactly one decision (used only by the
discrimination test).

Inputs are built, never extracted.  Descriptors are quantised: a base pattern with `pk` bits
flipped in its first half for a keyframe-2 feature and `pq` bits flipped in its second half for a
keyframe-1 feature, so distance = pk + pq exactly whenever the two share a base, and about 128
otherwise.  Node ids are assigned directly from the base (any partition of the features is a valid
FeatureVector).  tri_case derives F12 and the epipole from a pose; band_case uses the F12 with
a = 0, b = 1, c = -y1 (the line test becomes (y2 - y1)^2 < 3.84 sigma2), which places every
candidate exactly.
"""
from __future__ import annotations

import functools
import math
import struct

import numpy as np

from orbslam_mapsave_amd.abi import KEYPOINT_DTYPE, Frame

F32 = np.float32
TH_LOW, HISTO_LENGTH = 50, 30                     # ORBmatcher.cc:38-39
W, H = 640, 480
FX, FY, CX, CY = F32(500.0), F32(500.0), F32(320.0), F32(240.0)
NLEVELS = 4
SCALE = (F32(1.2) ** np.arange(NLEVELS)).astype(F32)      # mvScaleFactors
SIGMA2 = (SCALE * SCALE).astype(F32)                      # mvLevelSigma2
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)

MUTANTS = ("tie_ge", "th_lt", "no_block", "block_released", "mp1_kept", "mp2_kept",
           "stereo1_kept", "stereo2_kept", "epipole_stereo", "epipole_le", "den0_accepted",
           "thr_float", "f12_transposed", "no_wrap", "bin30_kept", "all_nodes")


def _bump(st, key, n=1):
    if st is not None:
        st[key] = st.get(key, 0) + n


def hamming(d, D):
    """Hamming distances of descriptor d (32 bytes) to the rows of D."""
    return _POP[np.bitwise_xor(D, d)].sum(axis=1)


def rot_bin(a1, a2, st=None, mutant=None):
    """Lines 769-774.  Angles in [0, 360) give bin <= 12; bin == HISTO_LENGTH needs a difference
    of 885 or more, which only angles outside that range produce."""
    rot = F32(a1) - F32(a2)
    if rot < 0.0:
        if mutant != "no_wrap":
            rot = rot + F32(360.0)
        _bump(st, "rot_wrap")
    x = float(rot * (F32(1.0) / F32(HISTO_LENGTH)))
    b = int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))   # std::round
    if b == HISTO_LENGTH:
        _bump(st, "bin30")
        if mutant != "bin30_kept":
            b = 0
    return b


def three_maxima(sizes):
    """ComputeThreeMaxima (1604-1645) -> (ind1, ind2, ind3)."""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if m2 < F32(0.1) * F32(m1):
        i2 = i3 = -1
    elif m3 < F32(0.1) * F32(m1):
        i3 = -1
    return i1, i2, i3


def check_dist_epipolar_line(x1, y1, x2, y2, oct2, F, sigma2, st=None, mutant=None):
    """Lines 140-157; every operand an np.float32 scalar."""
    if mutant == "f12_transposed":
        F = F.T
    a = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]
    b = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
    c = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if den == 0:
        _bump(st, "den0")
        return mutant == "den0_accepted"
    dsqr = num * num / den
    assert dsqr.dtype == np.float32
    as_double = float(dsqr) < 3.84 * float(sigma2[oct2])
    as_float = bool(dsqr < F32(3.84) * sigma2[oct2])
    if as_double != as_float:
        _bump(st, "thr_double_differs")
    ok = as_float if mutant == "thr_float" else as_double
    _bump(st, "line_pass" if ok else "line_reject")
    return ok


def _lower_bound(ids, lo, v):
    hi = len(ids)
    while lo < hi:
        mid = (lo + hi) // 2
        if ids[mid] < v:
            lo = mid + 1
        else:
            hi = mid
    return lo


def restated(c, check_ori, block, only_stereo, stats=None, mutant=None, _no_block_for=()):
    """-> (vMatches12, nmatches, pairs (n, 2))."""
    if mutant == "no_block":
        block = False
    kf1, kf2 = c["kf1"], c["kf2"]
    k1, k2 = kf1.keys, kf2.keys
    ur1 = kf1.u_right if kf1.u_right is not None else np.full(kf1.n, -1, F32)
    ur2 = kf2.u_right if kf2.u_right is not None else np.full(kf2.n, -1, F32)
    mp1, mp2 = c["mp1"], c["mp2"]
    F, sigma2, scale = c["F12"], c["sigma2"], kf2.scale_factors
    ex, ey = F32(c["epipole"][0]), F32(c["epipole"][1])
    ids1, off1, feat1 = c["fv1"]
    ids2, off2, feat2 = c["fv2"]
    matched2 = np.zeros(kf2.n, bool)                     # vbMatched2 (680)
    m12 = np.full(kf1.n, -1, np.int32)                   # vMatches12 (681)
    nmatches = 0
    hist = {}                                            # rotHist (683)
    blocker = {}                                         # idx2 -> idx1 that matched it
    i, j = 0, 0
    with np.errstate(over="ignore", invalid="ignore"):
        while i < len(ids1) and j < len(ids2):           # 694
            common = ids1[i] == ids2[j]
            if not common and mutant == "all_nodes":
                common = True
            if common:
                _bump(stats, "node_common")
                cand = feat2[off2[j]:off2[j + 1]]
                for idx1 in feat1[off1[i]:off1[i + 1]]:  # 698
                    if mp1[idx1] and mutant != "mp1_kept":   # 705
                        _bump(stats, "kf1_has_mp")
                        continue
                    st1 = ur1[idx1] >= 0                 # 708
                    if only_stereo and not st1 and mutant != "stereo1_kept":
                        _bump(stats, "kf1_not_stereo")
                        continue
                    dists = hamming(kf1.desc[idx1], kf2.desc[cand]) if len(cand) else []
                    best_dist, best = TH_LOW, -1         # 718-719
                    for r, idx2 in enumerate(cand):      # 721
                        if matched2[idx2]:               # 728
                            _bump(stats, "c2_blocked")
                            continue
                        if mp2[idx2] and mutant != "mp2_kept":
                            _bump(stats, "c2_has_mp")
                            continue
                        st2 = ur2[idx2] >= 0             # 731
                        if only_stereo and not st2 and mutant != "stereo2_kept":
                            _bump(stats, "c2_not_stereo")
                            continue
                        dist = int(dists[r])
                        if dist == TH_LOW + 1:
                            _bump(stats, "dist_51")
                        if dist > TH_LOW or (mutant == "th_lt" and dist == TH_LOW):   # 741
                            _bump(stats, "dist_gt_th")
                            continue
                        if dist > best_dist or (mutant == "tie_ge" and dist == best_dist and best >= 0):
                            _bump(stats, "dist_gt_best")
                            continue
                        if (not st1 and not st2) or mutant == "epipole_stereo":   # 746
                            distex = ex - k2["x"][idx2]
                            distey = ey - k2["y"][idx2]
                            r2 = distex * distex + distey * distey
                            thr = 100 * scale[k2["octave"][idx2]]
                            assert r2.dtype == np.float32 and thr.dtype == np.float32
                            if r2 == thr:
                                _bump(stats, "epi_equal")
                            if r2 < thr or (mutant == "epipole_le" and r2 == thr):    # 750
                                _bump(stats, "epi_reject")
                                continue
                            _bump(stats, "epi_pass")
                            if r2 < F32(1.3) * thr:
                                _bump(stats, "epi_near_pass")
                        elif float((ex - k2["x"][idx2]) ** 2 + (ey - k2["y"][idx2]) ** 2) < float(
                                100 * scale[k2["octave"][idx2]]):
                            _bump(stats, "epi_stereo_inside")
                        if check_dist_epipolar_line(k1["x"][idx1], k1["y"][idx1], k2["x"][idx2],
                                                    k2["y"][idx2], k2["octave"][idx2], F, sigma2,
                                                    stats, mutant):       # 754
                            if best >= 0 and dist == best_dist:
                                _bump(stats, "tie_replace")
                            best, best_dist = int(idx2), dist
                    if best >= 0:                        # 761
                        _bump(stats, "match")
                        if best_dist == TH_LOW:
                            _bump(stats, "match_at_50")
                        if best in blocker:
                            _bump(stats, "rematched2")
                        blocker[best] = int(idx1)
                        m12[idx1] = best
                        nmatches += 1
                        if block and idx1 not in _no_block_for:
                            matched2[best] = True        # the intent; absent from the source
                        if check_ori:                    # 767-777
                            b = rot_bin(k1["angle"][idx1], k2["angle"][best], stats, mutant)
                            hist.setdefault(b, []).append(int(idx1))
                    else:
                        _bump(stats, "no_match")
                i += 1
                j += 1
            elif ids1[i] < ids2[j]:                      # 784-787
                _bump(stats, "node_skip1")
                i = _lower_bound(ids1, i, ids2[j])
            else:
                _bump(stats, "node_skip2")
                j = _lower_bound(ids2, j, ids1[i])
    dropped = set()
    if check_ori:                                        # 794-813
        top = three_maxima([len(hist.get(b, ())) for b in range(HISTO_LENGTH)])
        for b in sorted(hist):       # a mutant's bins outside [0, 30) are never among the maxima
            if b in top:
                continue
            for idx1 in hist[b]:
                m12[idx1] = -1
                nmatches -= 1
                dropped.add(idx1)
                _bump(stats, "ori_dropped")
        if mutant == "block_released" and dropped and not _no_block_for:
            return restated(c, check_ori, block, only_stereo, None, None, frozenset(dropped))
    i1 = np.flatnonzero(m12 >= 0)
    pairs = np.stack([i1, m12[i1]], axis=1).astype(np.int32).reshape(-1, 2)
    return m12, nmatches, pairs


# ---- inputs ------------------------------------------------------------------------------------

def _bases(rng, n):
    return rng.integers(0, 256, size=(n, 32), dtype=np.uint8)


def _flip(base, rng, nbits, half):
    """base with nbits distinct bits flipped in bytes [0, 16) (half 0) or [16, 32) (half 1)."""
    d = base.copy()
    for bit in rng.choice(128, size=nbits, replace=False):
        d[16 * half + bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


def feature_vector(nodes, n):
    """Per-feature node ids (-1: in no node) -> (node_ids, node_off, feat), ids ascending,
    features ascending within a node, as FeatureVector::addFeature builds it."""
    nodes = np.asarray(nodes)
    ids = np.unique(nodes[nodes >= 0])
    off, feat = [0], []
    for v in ids:
        f = np.flatnonzero(nodes == v)
        feat.extend(f.tolist())
        off.append(len(feat))
    return ids.astype(np.int32), np.asarray(off, np.int32), np.asarray(feat, np.int32)


def _keys(x, y, octave, angle):
    k = np.zeros(len(x), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = x, y, octave, angle
    k["size"], k["class_id"] = 31.0, -1
    return k


def pose_geometry(rng):
    """Keyframe 1 at the world origin, keyframe 2 moved mostly forward so that the epipole lies
    inside image 2.  -> (R2w, t2w, Cw, F12, (ex, ey)): F12 = K^-T [t12]x R12 K^-1 as
    LocalMapping::ComputeF12 forms it (in double here, then float: its rounding is the caller's),
    the epipole by the expressions of ORBmatcher.cc:667-673 in float."""
    w = rng.uniform(-0.02, 0.02, 3)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R21 = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx
    t21 = np.array([rng.uniform(0.01, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.4, 0.6)])
    R12, t12 = R21.T, -R21.T @ t21
    K = np.array([[float(FX), 0, float(CX)], [0, float(FY), float(CY)], [0, 0, 1]])
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = (np.linalg.inv(K).T @ tx @ R12 @ np.linalg.inv(K)).astype(F32)
    R2w, t2w, Cw = R21.astype(F32), t21.astype(F32), np.zeros(3, F32)
    return R2w, t2w, Cw, F12, epipole_of(R2w, t2w, Cw)


def epipole_of(R2w, t2w, Cw):
    """Lines 667-673.  C2 = R2w * Cw + t2w is one cv::gemm (products and t2w accumulated in
    double, rounded to float once per element); invz, ex, ey are float expressions."""
    R, Cd, t = R2w.astype(np.float64), Cw.astype(np.float64), t2w.astype(np.float64)
    C2 = np.array([R[r, 0] * Cd[0] + R[r, 1] * Cd[1] + R[r, 2] * Cd[2] + t[r] for r in range(3)]).astype(F32)
    invz = F32(1.0) / C2[2]
    return F32(FX * C2[0] * invz + CX), F32(FY * C2[1] * invz + CY)


# angle differences and their shares: bins 2 and 3 lead; bin 0 (differences 0 and 900, the
# latter through bin 30) is third only with both of its halves, ahead of bin 5; bin 8 is dropped
ROT_CLASSES = ((60.0, 0.50), (90.0, 0.18), (150.0, 0.08), (0.0, 0.065), (900.0, 0.065),
               (240.0, 0.05))


@functools.lru_cache(maxsize=None)
def tri_case(seed, stereo_frac=0.5, round_epipole=True):
    """Two keyframes of about 330 / 380 features seeing one set of 3-D points (pose-derived F12).
    By construction: keyframe-1 clones that want one keyframe-2 feature (contention, and a first
    clone whose match the orientation filter drops), keyframe-2 clones at equal distance (ties),
    pairs at distance exactly 50 and 51, MapPoints on both sides, mixed stereo / mono features,
    keyframe-2 features inside, on and just outside the epipole radius (mono and stereo), angle
    differences that wrap below zero or land in bin 30 (an angle of 900 against 0: the histogram
    has 30 bins of which angles in [0, 360) reach 13; no pairing here reaches a bin above 30,
    where the reference writes outside rotHist), nodes present on one side only."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    R2w, t2w, Cw, F12, (ex, ey) = pose_geometry(rng)
    if round_epipole:   # quarter pixels: distex / distey of the placed features are then exact
        ex, ey = F32(round(float(ex) * 4) / 4), F32(round(float(ey) * 4) / 4)
    R21, t21 = R2w.astype(np.float64), t2w.astype(np.float64)
    nb = 14
    bases = _bases(rng, nb)
    f1, f2 = [], []     # dicts: x, y, oct, ang, desc, node, st, mp

    def add_pair(px2, depth, base, pk, pq, octave, rot, a2, st1, st2, mp1=0, mp2=0, n_clone1=1,
                 n_clone2=1, clone_pq=None, clone_rot=None, node2_shift=0):
        if rot >= 885:      # bin 30: 900 against 0, so that no pairing in the node passes bin 30
            a2 = 0.0
        X2 = depth * np.array([(px2[0] - float(CX)) / float(FX), (px2[1] - float(CY)) / float(FY), 1.0])
        X1 = R21.T @ (X2 - t21)
        if X1[2] <= 0.2:
            return False
        p1 = (float(FX) * X1[0] / X1[2] + float(CX), float(FY) * X1[1] / X1[2] + float(CY))
        if not (2 <= p1[0] < W - 2 and 2 <= p1[1] < H - 2):
            return False
        for cl in range(n_clone2):
            f2.append(dict(x=px2[0], y=px2[1], oct=octave, ang=a2, desc=_flip(bases[base], rng, pk, 0),
                           node=7 * base + 3 + node2_shift, st=st2, mp=mp2))
        for cl in range(n_clone1):
            r = rot if (clone_rot is None or cl > 0) else clone_rot
            a1 = a2 + r if r >= 885 else (a2 + r) % 360.0
            q = pq if clone_pq is None else clone_pq[cl]
            f1.append(dict(x=p1[0] + 0.05 * cl, y=p1[1], oct=octave, ang=a1,
                           desc=_flip(bases[base], rng, q, 1), node=7 * base + 3, st=st1, mp=mp1))
        return True

    def rnd_rot():
        u, acc = rng.uniform(), 0.0
        for r, p in ROT_CLASSES:
            acc += p
            if u < acc:
                return r
        return 60.0

    def rnd_px():
        return (float(F32(rng.uniform(20, W - 20))), float(F32(rng.uniform(20, H - 20))))

    def st():
        return bool(rng.uniform() < stereo_frac)

    a2s = (0.0, 45.0, 200.0, 310.0)
    # regular correspondences (bases 0-9 common; 10-11 only on one side's node id)
    for _ in range(230):
        base = int(rng.integers(0, 12))
        add_pair(rnd_px(), rng.uniform(2, 8), base, int(rng.integers(0, 9)), int(rng.integers(0, 9)),
                 int(rng.integers(0, NLEVELS)), rnd_rot(), a2s[int(rng.integers(0, 4))], st(), st(),
                 mp1=int(rng.uniform() < 0.12), mp2=int(rng.uniform() < 0.12),
                 node2_shift=1 if base >= 10 else 0)
    # contention: three keyframe-1 clones, the closest one last; the first clone's angle falls in
    # a rare bin so that the filter drops its match
    for _ in range(10):
        add_pair(rnd_px(), rng.uniform(2, 8), 12, 3, 0, 0, 60.0, 45.0, st(), st(), n_clone1=3,
                 clone_pq=(6, 4, 2), clone_rot=240.0)
    # ties: three keyframe-2 clones at the same distance
    for _ in range(10):
        add_pair(rnd_px(), rng.uniform(2, 8), 13, 4, 3, int(rng.integers(0, NLEVELS)), 60.0, 0.0,
                 st(), st(), n_clone2=3)
    # distance exactly 50 and exactly 51
    for _ in range(8):
        add_pair(rnd_px(), rng.uniform(2, 8), int(rng.integers(0, 10)), 25, 25, 1, 90.0, 200.0, st(), st())
        add_pair(rnd_px(), rng.uniform(2, 8), int(rng.integers(0, 10)), 26, 25, 1, 90.0, 200.0, st(), st())
    # around the epipole: inside, on and just outside the radius 10 sqrt(scale) (750)
    for k in range(30):
        octave = 0 if k % 3 == 1 else int(rng.integers(0, NLEVELS))
        thr = 100.0 * float(SCALE[octave])
        if k % 3 == 0:
            rr = math.sqrt(thr * rng.uniform(0.3, 0.9))
        elif k % 3 == 1:
            rr = 10.0                                    # exactly on the radius at octave 0
        else:
            rr = math.sqrt(thr * rng.uniform(1.05, 1.25))
        if k % 3 == 1:
            dx, dy = ((6.0, 8.0), (-8.0, 6.0), (0.0, -10.0), (10.0, 0.0), (-6.0, -8.0))[(k // 3) % 5]
        else:
            ang = rng.uniform(0, 2 * math.pi)
            dx, dy = rr * math.cos(ang), rr * math.sin(ang)
        px = (float(F32(float(ex) - dx)), float(F32(float(ey) - dy)))
        mono = (k // 3) % 3 != 2
        add_pair(px, rng.uniform(3, 8), int(rng.integers(0, 10)), 2, 2, octave, 60.0, 45.0,
                 not mono and k % 2 == 0, not mono)
    # keyframe-2 features without a partner
    for _ in range(40):
        px = rnd_px()
        f2.append(dict(x=px[0], y=px[1], oct=int(rng.integers(0, NLEVELS)), ang=0.0,
                       desc=_flip(bases[int(rng.integers(0, 12))], rng, 5, 0),
                       node=7 * int(rng.integers(0, 12)) + 3, st=st(), mp=0))

    def pack(fs, noise):
        perm = rng.permutation(len(fs))
        fs = [fs[i] for i in perm]
        x = np.array([f["x"] for f in fs], np.float64) + rng.uniform(-noise, noise, len(fs))
        y = np.array([f["y"] for f in fs], np.float64) + rng.uniform(-noise, noise, len(fs))
        keys = _keys(x.astype(F32), y.astype(F32), [f["oct"] for f in fs], [f["ang"] for f in fs])
        ur = np.array([f["x"] - 20.0 if f["st"] else -1.0 for f in fs], F32)
        kf = Frame(keys, np.stack([f["desc"] for f in fs]), W, H, SCALE, ur)
        mp = np.array([f["mp"] for f in fs], np.uint8)
        return kf, mp, feature_vector([f["node"] for f in fs], len(fs))

    kf1, mp1, fv1 = pack(f1, 0.25)
    kf2, mp2, fv2 = pack(f2, 0.0)
    assert kf1.n <= 400 and kf2.n <= 400
    return dict(kf1=kf1, kf2=kf2, mp1=mp1, mp2=mp2, fv1=fv1, fv2=fv2, F12=F12,
                epipole=np.array([ex, ey], F32), sigma2=SIGMA2, pose=(R2w, t2w, Cw))


def den0_case(seed=0):
    """tri_case with the first two columns of F12 zero: a = b = 0 for every keyframe-1 feature."""
    c = dict(tri_case(seed))
    F = c["F12"].copy()
    F[:, :2] = 0
    c["F12"] = F
    return c


def monocular(c):
    """The case with mvuRight absent on both sides (u_right NULL)."""
    k1, k2 = c["kf1"], c["kf2"]
    return dict(c, kf1=Frame(k1.keys, k1.desc, W, H, SCALE), kf2=Frame(k2.keys, k2.desc, W, H, SCALE))


BAND_F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F32)   # a = 0, b = 1, c = -y1
NUM_384 = F32(np.sqrt(3.84))   # its float square is (float)3.84f, which is below the double 3.84
assert F32(NUM_384 * NUM_384) == F32(3.84) and float(F32(3.84)) < 3.84


def band_case(node_sizes2, n1_per_node=None, seed=0, octave=0, all_mp1=False, dup=False):
    """One node per entry of node_sizes2 with that many keyframe-2 features, every feature of one
    base; F12 = BAND_F12, the epipole far away.  Keyframe-2 feature r of a node sits at
    y = 20 r (its own band); keyframe-1 feature k of the node at y of feature r = (k * 37 + 11) mod
    size (every feature once when n1_per_node is None), shifted by 1 px, so it passes the line
    test for that feature alone; dup adds a second keyframe-1 feature on each (contention)."""
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    base = _bases(rng, 1)[0]
    f1, f2 = [], []
    for node, size in enumerate(node_sizes2):
        for r in range(size):
            f2.append((100.0 + node, 20.0 * r, _flip(base, rng, int(rng.integers(0, 6)), 0), 10 * node + 5))
        for k in range((size if n1_per_node is None else n1_per_node) if size else 1):
            r = (k * 37 + 11) % max(size, 1)
            for e in range(2 if dup else 1):
                f1.append((50.0 + k, 20.0 * r + 1.0 - 0.5 * e, _flip(base, rng, int(rng.integers(0, 6)), 1),
                           10 * node + 5))

    def pack(fs):
        keys = _keys(np.array([f[0] for f in fs], F32), np.array([f[1] for f in fs], F32),
                     np.full(len(fs), octave), np.zeros(len(fs), F32))
        desc = np.stack([f[2] for f in fs]) if fs else np.zeros((0, 32), np.uint8)
        return Frame(keys, desc, W, H, SCALE), feature_vector([f[3] for f in fs], len(fs))

    (kf1, fv1), (kf2, fv2) = pack(f1), pack(f2)
    return dict(kf1=kf1, kf2=kf2, mp1=np.full(kf1.n, int(all_mp1), np.uint8), mp2=np.zeros(kf2.n, np.uint8),
                fv1=fv1, fv2=fv2, F12=BAND_F12, epipole=np.array([-5000, -5000], F32), sigma2=SIGMA2)


def threshold_case():
    """Eight nodes of one keyframe-1 feature at y = 0 and one keyframe-2 feature at y = num
    (octave 0, sigma2 = 1): num = NUM_384 gives dsqr = (float)3.84f, accepted by the reference's
    double comparison and rejected by a float one; the next float above is rejected by both, the
    one below accepted by both."""
    rng = np.random.Generator(np.random.PCG64(99))
    base = _bases(rng, 1)[0]
    up, down = np.nextafter(NUM_384, F32(10)), np.nextafter(NUM_384, F32(0))
    y2 = np.array([NUM_384] * 6 + [up, down], F32)
    n = len(y2)
    k1 = _keys(np.arange(n, dtype=F32) * 7, np.zeros(n, F32), np.zeros(n, int), np.zeros(n, F32))
    k2 = _keys(np.arange(n, dtype=F32) * 5, y2, np.zeros(n, int), np.zeros(n, F32))
    d1 = np.stack([_flip(base, rng, 3, 1) for _ in range(n)])
    d2 = np.stack([_flip(base, rng, 2, 0) for _ in range(n)])
    fv = feature_vector(np.arange(n) * 4 + 2, n)
    return dict(kf1=Frame(k1, d1, W, H, SCALE), kf2=Frame(k2, d2, W, H, SCALE),
                mp1=np.zeros(n, np.uint8), mp2=np.zeros(n, np.uint8), fv1=fv, fv2=fv, F12=BAND_F12,
                epipole=np.array([-5000, -5000], F32), sigma2=SIGMA2)


def built_cases():
    """name -> case: the set the mutant and coverage tests run over."""
    return {"pose0": tri_case(0), "pose1": tri_case(1), "pose2_stereo": tri_case(2, 0.9),
            "den0": den0_case(0), "threshold": threshold_case(),
            "band": band_case((5, 1, 70, 0, 9), seed=1, dup=True)}


CONFIGS = [(ori, blk, st) for ori in (False, True) for blk in (False, True) for st in (False, True)]


def dump_case(path, c, check_ori, only_stereo):
    """The case as the flat binary tests/cpp/triangulation_test.cpp reads (little endian): header
    of int32 {n1, n2, nn1, nn2, tot1, tot2, nlevels, check_ori, only_stereo, stereo}, then camera
    fx fy cx cy, R2w (9), t2w (3), Cw (3), F12 (9), scale, sigma2, and per keyframe keys,
    descriptors, u_right (when stereo), map-point flags, node ids, node offsets, features."""
    kf1, kf2 = c["kf1"], c["kf2"]
    R2w, t2w, Cw = c["pose"]
    stereo = int(kf1.u_right is not None)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<10i", kf1.n, kf2.n, len(c["fv1"][0]), len(c["fv2"][0]), len(c["fv1"][2]),
                             len(c["fv2"][2]), len(SCALE), int(check_ori), int(only_stereo), stereo))
        for a in (np.array([FX, FY, CX, CY], F32), R2w, t2w, Cw, c["F12"], SCALE, c["sigma2"]):
            fh.write(np.ascontiguousarray(a, F32).tobytes())
        for kf, mp, fv in ((kf1, c["mp1"], c["fv1"]), (kf2, c["mp2"], c["fv2"])):
            fh.write(kf.keys.tobytes())
            fh.write(kf.desc.tobytes())
            if stereo:
                fh.write(kf.u_right.tobytes())
            fh.write(mp.tobytes())
            for a in fv:
                fh.write(np.ascontiguousarray(a, np.int32).tobytes())
