"""The order-dependent matchers -- SearchForInitialization (ORBmatcher.cc:408-523),
SearchByProjection local map (45-137), last frame (1331-1473) and keyframe (1475-1602) -- as
pure-Python restatements written from those lines (with Frame::GetFeaturesInArea / PosInGrid,
Frame.cc:445-510, and ComputeThreeMaxima, ORBmatcher.cc:1604-1645) and seeded adversarial inputs
that reach their tie and quirk branches on purpose.

The restatements enumerate their own candidates (cell = std::round of the float product, the
window by floor / ceil, candidates in column, row, keypoint-index order), compute their own Hamming
distances and follow the float evaluation order of DESIGN section 2.  Each counts the branches it
takes into an optional `stats` dict and takes `mutant=`, which flips exactly one decision (used
only by the discrimination test).  The keyframe overload's restatement is
test_sbp_keyframe.restated.

Inputs are built, never extracted: keypoints on a 40 px lattice of sites (some exactly on the
`.5` cell boundaries), octaves 0-3, angles from a short list, and quantised descriptors -- a
base descriptor with `pk` bits flipped in its first half for a frame keypoint and `pq` bits flipped
in its second half for a query, so that distance(query, keypoint) = pk + pq exactly whenever the two
share a base.
"""
from __future__ import annotations

import math

import numpy as np

import oracle
import scenarios as S
from orbslam_mapsave_amd.abi import KEYPOINT_DTYPE, Frame, MapPoints
from test_sbp_keyframe import restated as restated_keyframe  # noqa: F401  (re-exported)

F32 = np.float32
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30   # ORBmatcher.cc:37-39
INT_MAX = 2 ** 31 - 1
SCALE = (F32(1.2) ** np.arange(8)).astype(F32)
LOG_SCALE = float(np.log(F32(1.2)).astype(F32))
GRID_COLS, GRID_ROWS = 64, 48
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)

SFI_MUTANTS = ("steal_lt", "stolen_not_in_hist", "th_lt", "ratio_le", "round_half_even", "maxima_ge",
               "tenth_double", "order_by_index")
LOCAL_MUTANTS = ("ratio_any_level", "ratio_ge", "th_lt", "stereo_ge", "order_by_index")
LAST_MUTANTS = ("overwritten_not_cleared", "overwritten_not_counted", "th_lt", "stereo_ge",
                "round_half_even", "maxima_ge", "tenth_double", "order_by_index")
# The mutants of the projection gates in front of the greedy part (tests/projection_cases.py
# builds the inputs that show them).  *_EQUIVALENT: decisions written differently that no input
# separates, asserted as equivalences:
#   radius_ge              no float equals the double 0.998, so `>=` and `>` agree on every float
#   th_always_multiplied   r * 1.0f == r: `if(bFactor)` only saves the product
#   invz_float, stereo_ur_uses_float_invz
#                          (float)(1.0 / (double)z) == 1.0f / z for every float z (a quotient
#                          rounded to 53 bits and then to 24 is the quotient rounded to 24)
LOCAL_GATE_MUTANTS = ("radius_float_0998", "level_window_plus1", "stereo_ge")
LOCAL_GATE_EQUIVALENT = ("radius_ge", "th_always_multiplied")
#   depth_z_lt0            z = -0.0f passes `z < 0` and fails `invzc < 0`; but then u and v are
#                          NaN or infinite: the point leaves at the image test or searches
#                          around a NaN centre, which finds nothing (DESIGN H21).  The branch
#                          counter `behind` tells the two apart, the outputs do not.
LAST_GATE_MUTANTS = ("bounds_strict", "forward_ge", "backward_ge", "forward_ignores_mono",
                     "window_forward_closed")
LAST_GATE_EQUIVALENT = ("depth_z_lt0", "invz_float", "stereo_ur_uses_float_invz")


def _bump(st, key, n=1):
    if st is not None:
        st[key] = st.get(key, 0) + n


def hamming(d, D):
    """Hamming distances of descriptor d (32 bytes) to the rows of D."""
    return _POP[np.bitwise_xor(D, d)].sum(axis=1)


def _round_away(a):
    """std::round of float values: halves away from zero."""
    a = np.asarray(a, np.float64)
    return np.where(a >= 0, np.floor(a + 0.5), -np.floor(-a + 0.5)).astype(np.int64)


class Grid:
    """Frame::AssignFeaturesToGrid + GetFeaturesInArea (Frame.cc:341-356, 445-510)."""

    def __init__(self, f: Frame):
        k = f.keys
        self.kx, self.ky, self.oct = k["x"], k["y"], k["octave"]
        self.minx, self.miny = F32(f.min_x), F32(f.min_y)
        self.gw, self.gh = F32(f.grid_w_inv), F32(f.grid_h_inv)
        gx = _round_away((self.kx - self.minx) * self.gw)   # PosInGrid (500-510)
        gy = _round_away((self.ky - self.miny) * self.gh)
        idx = np.flatnonzero((gx >= 0) & (gx < GRID_COLS) & (gy >= 0) & (gy < GRID_ROWS))
        o = np.lexsort((idx, gy[idx], gx[idx]))             # mGrid[ix][iy], insertion order
        self.order = idx[o]
        self.ogx, self.ogy = gx[self.order], gy[self.order]

    def area(self, x, y, r, lo, hi, by_index=False):
        x, y, r = F32(x), F32(y), F32(r)
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(r)):
            # (int)floor(NaN) is undefined in the reference; pinned (DESIGN H21): no candidates
            return np.zeros(0, np.int64)
        cx0 = max(0, math.floor((x - self.minx - r) * self.gw))
        if cx0 >= GRID_COLS:
            return np.zeros(0, np.int64)
        cx1 = min(GRID_COLS - 1, math.ceil((x - self.minx + r) * self.gw))
        if cx1 < 0:
            return np.zeros(0, np.int64)
        cy0 = max(0, math.floor((y - self.miny - r) * self.gh))
        if cy0 >= GRID_ROWS:
            return np.zeros(0, np.int64)
        cy1 = min(GRID_ROWS - 1, math.ceil((y - self.miny + r) * self.gh))
        if cy1 < 0:
            return np.zeros(0, np.int64)
        c = self.order[(self.ogx >= cx0) & (self.ogx <= cx1) & (self.ogy >= cy0) & (self.ogy <= cy1)]
        if lo > 0 or hi >= 0:                               # bCheckLevels (466)
            c = c[self.oct[c] >= lo]
            if hi >= 0:
                c = c[self.oct[c] <= hi]
        c = c[(np.abs(self.kx[c] - x) < r) & (np.abs(self.ky[c] - y) < r)]
        return np.sort(c) if by_index else c


def rot_bin(a1, a2, st=None, mutant=None):
    """ORBmatcher.cc:478-483 / 1436-1441.  rot < 360 gives bin <= 12: `bin == HISTO_LENGTH` is
    unreachable and has no counter."""
    rot = F32(a1) - F32(a2)
    if rot < 0.0:
        rot = rot + F32(360.0)
        _bump(st, "bin_wrap")
    x = float(rot * (F32(1.0) / F32(HISTO_LENGTH)))
    if x - math.floor(x) == 0.5:
        _bump(st, "bin_half")
    b = int(np.rint(x)) if mutant == "round_half_even" else int(math.floor(x + 0.5))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes, st=None, mutant=None):
    """ComputeThreeMaxima (1604-1645) -> (ind1, ind2, ind3)."""
    if mutant == "maxima_ge":
        def gt(a, b):
            return a > 0 and a >= b
    else:
        def gt(a, b):
            return a > b
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > 0 and (s == m1 or (s < m1 and s == m2) or (s < m2 and s == m3)):
            _bump(st, "maxima_tie")
        if gt(s, m1):
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif gt(s, m2):
            m3, m2, i3, i2 = m2, s, i2, i
        elif gt(s, m3):
            m3, i3 = s, i
    if mutant == "tenth_double":            # 0.1f promoted: (double)0.1f * 10 > 1
        edge = float(F32(0.1)) * m1
    else:
        edge = F32(0.1) * F32(m1)
    if m1 > 0 and F32(m2) == F32(0.1) * F32(m1):
        _bump(st, "maxima_tenth_edge")
    if m2 < edge:
        i2 = i3 = -1
    else:
        if m1 > 0 and F32(m3) == F32(0.1) * F32(m1):
            _bump(st, "maxima_tenth_edge")
        if m3 < edge:
            i3 = -1
    return i1, i2, i3


# ---- SearchForInitialization (408-523) -----------------------------------------------------------

def restated_sfi(f1: Frame, f2: Frame, prev, window, nnratio, check_ori=True, stats=None,
                 mutant=None):
    """-> (vnMatches12, nmatches, vbPrevMatched)."""
    st = stats
    g2 = Grid(f2)
    prev = np.ascontiguousarray(prev, F32).reshape(-1, 2).copy()
    n1, n2 = f1.n, f2.n
    m12 = np.full(n1, -1, np.int32)
    m21 = [-1] * n2
    md = [INT_MAX] * n2
    hist = [[] for _ in range(HISTO_LENGTH)]
    bin_of = {}
    nm = 0
    ratio = F32(nnratio)
    for i1 in range(n1):
        lvl = int(f1.keys["octave"][i1])
        if lvl > 0:
            continue
        c = g2.area(prev[i1, 0], prev[i1, 1], F32(window), lvl, lvl, mutant == "order_by_index")
        if len(c) == 0:
            continue
        best = second = INT_MAX
        bi, nbest = -1, 0
        for i2, d in zip(c.tolist(), hamming(f1.desc[i1], f2.desc[c]).tolist()):
            if md[i2] == d:
                _bump(st, "steal_refused_equal")
            if (md[i2] < d) if mutant == "steal_lt" else (md[i2] <= d):   # 447
                continue
            if d < best:
                second, best, bi, nbest = best, d, i2, 1
            elif d < second:
                second = d
                nbest += d == best
        th_ok = best < TH_LOW if mutant == "th_lt" else best <= TH_LOW
        if th_ok and F32(best) == F32(second) * ratio:
            _bump(st, "ratio_equal_reject")
        passes = F32(best) <= F32(second) * ratio if mutant == "ratio_le" else \
            F32(best) < F32(second) * ratio
        if th_ok and passes:                                             # 462-464
            if best == TH_LOW:
                _bump(st, "best_eq_th")
            if nbest > 1:
                _bump(st, "first_wins_tie")
            if m21[bi] >= 0:                                             # 466-470
                j = m21[bi]
                m12[j] = -1
                nm -= 1
                _bump(st, "steal")
                if check_ori:
                    _bump(st, "stolen_in_hist")
                    if mutant == "stolen_not_in_hist":
                        hist[bin_of[j]].remove(j)
            m12[i1] = bi
            m21[bi] = i1
            md[bi] = best
            nm += 1
            if check_ori:
                b = rot_bin(f1.keys["angle"][i1], f2.keys["angle"][bi], st, mutant)
                hist[b].append(i1)
                bin_of[i1] = b
    if check_ori:
        keep = three_maxima([len(h) for h in hist], st, mutant)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for i1 in hist[b]:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nm -= 1
    for i1 in range(n1):
        if m12[i1] >= 0:
            prev[i1, 0] = f2.keys["x"][m12[i1]]
            prev[i1, 1] = f2.keys["y"][m12[i1]]
    return m12, nm, prev


# ---- SearchByProjection, local map (45-137) -------------------------------------------------------

def radius_by_viewing_cos(view_cos, th, mutant=None):
    """RadiusByViewingCos (131-137) and `if(bFactor) r*=th` (49, 65-66): the float viewCos and th
    are compared with the double literals 0.998 and 1.0."""
    if mutant == "radius_float_0998":            # (float)0.998 > 0.998: the boundary float
        near = F32(view_cos) > F32(0.998)
    elif mutant == "radius_ge":
        near = float(view_cos) >= 0.998
    else:
        near = float(view_cos) > 0.998
    r = F32(2.5) if near else F32(4.0)
    if float(th) != 1.0 or mutant == "th_always_multiplied":
        r = r * F32(th)
    return r


def restated_local(f: Frame, mps: MapPoints, th, nnratio, frame_mp=None, frame_mp_obs=None,
                   mp_ids=None, stats=None, mutant=None, info=None):
    """-> (frame_mp, frame_mp_obs, nmatches).  A predicted level outside mvScaleFactors (the
    reference reads past the vector, ORBmatcher.cc:69) skips the point and sets
    info["unsupported"]."""
    st = stats
    g = Grid(f)
    fmp = np.full(f.n, -1, np.int32) if frame_mp is None else np.array(frame_mp, np.int32)
    fobs = np.zeros(f.n, np.int32) if frame_mp_obs is None else np.array(frame_mp_obs, np.int32)
    ours = set()
    nm = 0
    th = F32(th)
    ratio = F32(nnratio)
    for i in range(mps.m):
        if not mps.track_in_view[i] or mps.is_bad[i]:
            continue
        pl = int(mps.pred_level[i])
        if pl < 0 or pl >= len(f.scale_factors):
            _bump(st, "level_outside")
            if info is not None:
                info["unsupported"] = True
            continue
        r = radius_by_viewing_cos(mps.view_cos[i], th, mutant)          # 131-137
        _bump(st, "radius_2.5" if r == F32(2.5) * (th if float(th) != 1.0 else F32(1.0))
              else "radius_4.0")
        rs = r * f.scale_factors[pl]
        hi = pl + 1 if mutant == "level_window_plus1" else pl
        c = g.area(mps.proj_x[i], mps.proj_y[i], rs, pl - 1, hi, mutant == "order_by_index")
        if len(c) == 0:
            continue
        best = second = 256
        bl = sl = bi = -1
        nbest = 0
        for idx, d in zip(c.tolist(), hamming(mps.desc[i], f.desc[c]).tolist()):
            if fmp[idx] >= 0 and fobs[idx] > 0:                         # 87-89
                continue
            if f.u_right is not None and f.u_right[idx] > 0:            # 91-96
                er = abs(mps.proj_xr[i] - f.u_right[idx])
                if er == rs:
                    _bump(st, "stereo_edge")
                if (er >= rs) if mutant == "stereo_ge" else (er > rs):
                    continue
            lv = int(f.keys["octave"][idx])
            if d < best:
                second, best, sl, bl, bi, nbest = best, d, bl, lv, idx, 1
            elif d < second:
                sl, second = lv, d
                nbest += d == best
            elif d == best:
                nbest += 1
        if (best < TH_HIGH) if mutant == "th_lt" else (best <= TH_HIGH):  # 118
            bound = ratio * F32(second)
            fails = F32(best) >= bound if mutant == "ratio_ge" else F32(best) > bound
            if bl == sl or mutant == "ratio_any_level":
                if bl == sl and F32(best) == bound:
                    _bump(st, "ratio_equal_pass")
                if fails:
                    if bl == sl:
                        _bump(st, "ratio_same_level_reject")
                    continue
            elif fails:
                _bump(st, "ratio_skipped_levels_differ")
            if best == TH_HIGH:
                _bump(st, "best_eq_th")
            if nbest > 1:
                _bump(st, "first_wins_tie")
            if bi in ours:
                _bump(st, "overwrite_nobs0")
            ours.add(bi)
            fmp[bi] = i if mp_ids is None else mp_ids[i]
            fobs[bi] = mps.n_obs[i]
            nm += 1
    return fmp, fobs, nm


# ---- SearchByProjection, last frame (1331-1473) ---------------------------------------------------

def camera_center(T):
    """-Rcw^T tcw, accumulated in double."""
    return [F32(-(float(T[0, i]) * float(T[0, 3]) + float(T[1, i]) * float(T[1, 3]) +
                  float(T[2, i]) * float(T[2, 3]))) for i in range(3)]


def rigid(T, P):
    return [((T[r, 0] * P[0] + T[r, 1] * P[1]) + T[r, 2] * P[2]) + T[r, 3] for r in range(3)]


def last_motion(c, mono, mutant=None):
    """(bForward, bBackward) (1341-1352)."""
    Tc = np.asarray(c["tcw_cur"], F32).reshape(3, 4)
    Tl = np.asarray(c["tcw_last"], F32).reshape(3, 4)
    tlc = rigid(Tl, camera_center(Tc))
    b = F32(c["cam"].b)
    fwd = tlc[2] >= b if mutant == "forward_ge" else tlc[2] > b
    bwd = -tlc[2] >= b if mutant == "backward_ge" else -tlc[2] > b
    return (bool(fwd and (not mono or mutant == "forward_ignores_mono")), bool(bwd and not mono))


def last_project(c, i, mutant=None):
    """(invz, u, v, ur) of last-frame point i in the current frame."""
    return _last_project(c, i, mutant)[:4]


def _last_project(c, i, mutant=None):
    """(invz, u, v, ur, z) of last-frame point i in the current frame (1363-1374, 1412):
    invzc = 1.0 / z is a double quotient rounded to float, -inf for z = -0.0f."""
    T = np.asarray(c["tcw_cur"], F32).reshape(3, 4)
    cam = c["cam"]
    pc = rigid(T, np.asarray(c["last_xyz"], F32)[i])
    with np.errstate(all="ignore"):
        if mutant == "invz_float":
            invz = F32(1.0) / pc[2]
        else:
            invz = F32(np.float64(1.0) / np.float64(pc[2]))
        u = F32(cam.fx) * pc[0] * invz + F32(cam.cx)
        v = F32(cam.fy) * pc[1] * invz + F32(cam.cy)
        if mutant == "stereo_ur_uses_float_invz":
            ur = u - F32(cam.bf) * (F32(1.0) / pc[2])
        else:
            ur = u - F32(cam.bf) * invz
    return invz, u, v, ur, pc[2]


def restated_last(c, th, mono, check_ori=True, frame_mp=None, frame_mp_obs=None, stats=None,
                  mutant=None):
    """`c` as scenarios.sbp_last_case -> (frame_mp, frame_mp_obs, nmatches)."""
    st = stats
    cur = c["cur"]
    g = Grid(cur)
    fmp = np.full(cur.n, -1, np.int32) if frame_mp is None else np.array(frame_mp, np.int32)
    fobs = np.zeros(cur.n, np.int32) if frame_mp_obs is None else np.array(frame_mp_obs, np.int32)
    fwd, bwd = last_motion(c, mono, mutant)
    lk = c["last_keys"]
    ids = c.get("last_ids")
    holder = {}                                   # slot -> acceptance that holds it
    hist = [[] for _ in range(HISTO_LENGTH)]      # (slot, acceptance)
    nm = 0
    for i in range(len(lk)):
        if not c["last_valid"][i] or c["last_outlier"][i]:
            continue
        invz, u, v, ur, z = _last_project(c, i, mutant)
        if (z < 0) if mutant == "depth_z_lt0" else (invz < 0):          # 1370: -0.0f is behind
            _bump(st, "behind")
            continue
        if mutant == "bounds_strict":
            out = (u <= F32(cur.min_x) or u >= F32(cur.max_x) or v <= F32(cur.min_y) or
                   v >= F32(cur.max_y))
        else:                                                           # 1376-1379: NaN passes
            out = (u < F32(cur.min_x) or u > F32(cur.max_x) or v < F32(cur.min_y) or
                   v > F32(cur.max_y))
        if out:
            _bump(st, "outside")
            continue
        _bump(st, "window_forward" if fwd else "window_backward" if bwd else "window_both")
        o = int(lk["octave"][i])
        radius = F32(th) * cur.scale_factors[o]
        lo, hi = (o, -1) if fwd else (0, o) if bwd else (o - 1, o + 1)  # 1388-1393
        if fwd and mutant == "window_forward_closed":
            hi = o + 1
        cand = g.area(u, v, radius, lo, hi, mutant == "order_by_index")
        if len(cand) == 0:
            continue
        best, bi, nbest = 256, -1, 0
        for i2, d in zip(cand.tolist(), hamming(c["last_desc"][i], cur.desc[cand]).tolist()):
            if fmp[i2] >= 0 and fobs[i2] > 0:                           # 1406-1408
                continue
            if cur.u_right is not None and cur.u_right[i2] > 0:         # 1410-1416
                er = abs(ur - cur.u_right[i2])
                if er == radius:
                    _bump(st, "stereo_edge")
                if (er >= radius) if mutant == "stereo_ge" else (er > radius):
                    continue
            if d < best:
                best, bi, nbest = d, i2, 1
            elif d == best:
                nbest += 1
        if (best < TH_HIGH) if mutant == "th_lt" else (best <= TH_HIGH):  # 1429
            if best == TH_HIGH:
                _bump(st, "best_eq_th")
            if nbest > 1:
                _bump(st, "first_wins_tie")
            if bi in holder:
                _bump(st, "overwrite_nobs0")
                if mutant == "overwritten_not_counted":
                    nm -= 1
            holder[bi] = i
            fmp[bi] = i if ids is None else ids[i]
            fobs[bi] = c["last_nobs"][i]
            nm += 1
            if check_ori:
                hist[rot_bin(lk["angle"][i], cur.keys["angle"][bi], st, mutant)].append((bi, i))
    if check_ori:
        keep = three_maxima([len(h) for h in hist], st, mutant)
        bin_of = {i: b for b in range(HISTO_LENGTH) for _, i in hist[b]}
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for bi, i in hist[b]:
                if holder[bi] != i:
                    if mutant == "overwritten_not_cleared":
                        continue
                    if bin_of[holder[bi]] in keep:
                        _bump(st, "cleared_by_overwritten_bin")
                fmp[bi] = -1
                fobs[bi] = 0
                nm -= 1
    return fmp, fobs, nm


# ---- adversarial inputs --------------------------------------------------------------------------

def _bases():
    """Six base descriptors at pairwise distance >= 112."""
    rng = np.random.Generator(np.random.PCG64(2024))
    out = []
    while len(out) < 6:
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        if all(int(_POP[d ^ o].sum()) >= 112 for o in out):
            out.append(d)
    return out


BASES = _bases()
HALF_DIFFS = (15, 135, 255)   # F32(diff) * F32(1/30) lands exactly on k + 0.5
KP_ANGLES = (0.0, 30.0, 100.0, 200.0, 350.0)


def quantised(base, pk=0, kvar=0, pq=0, qvar=0):
    """BASES[base] with pk bits flipped among bits 0-127 and pq among bits 128-255."""
    bits = np.unpackbits(BASES[base])
    for j in range(pk):
        bits[(kvar * 17 + j) % 128] ^= 1
    for j in range(pq):
        bits[128 + (qvar * 13 + j) % 128] ^= 1
    return np.packbits(bits)


class Builder:
    """Keypoints of the searched frame and queries (F1 keypoints / map points) placed gadget by
    gadget on lattice sites.  A keypoint's `ur` is (query, kind) with kind in none / zero / inside
    / edge / beyond, resolved against that query's right-image coordinate by the matcher's
    finaliser."""

    OFFSETS = ((0.0, 0.0), (5.0, 0.0), (0.0, 5.0), (5.0, 5.0), (2.5, 1.25), (-0.75, 0.5))

    def __init__(self, seed, stride=1):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        sites = [(float(x), float(y)) for x in range(40, 601, 40 * stride)
                 for y in range(40, 441, 40 * stride)]
        self.rng.shuffle(sites)
        self.sites = sites
        self.kp, self.q = [], []

    def site(self):
        x, y = self.sites.pop()
        dx, dy = self.OFFSETS[self.rng.integers(len(self.OFFSETS))]
        return x + dx, y + dy

    def add_kp(self, x, y, octave, angle, base, pk, var=0, ur=None):
        self.kp.append(dict(x=x, y=y, oct=int(octave), ang=float(angle),
                            desc=quantised(base, pk, var), ur=ur))
        return len(self.kp) - 1

    def add_q(self, x, y, lvl, angle, base, pq, var=0, nobs=1, near=False, flag=None):
        self.q.append(dict(x=x, y=y, lvl=int(lvl), ang=float(angle) % 360.0,
                           desc=quantised(base, 0, 0, pq, var), nobs=int(nobs), near=bool(near),
                           flag=flag, z=float(self.rng.uniform(2.0, 8.0))))
        return len(self.q) - 1


def _lvl(b, sfi):
    return 0 if sfi else int(b.rng.integers(0, 4))


def _populate(b: Builder, thr, sfi=False, kf=False, stereo=False, spread=6.0, n_sites=None):
    """Contention, tie, threshold, ratio, level-decoy and stereo gadgets over the sites."""
    rng = b.rng
    nobs_patterns = ((0, 0, 1, 1), (1, 1, 1, 1), (0, 1, 0, 1), (0, 0, 0, 1), (0, 0, 0, 0))
    ties = ((-spread, 0.0, spread, 0.0), (spread, 0.0, -spread, 0.0), (0.0, spread, 0.0, -spread),
            (0.0, -spread, 0.0, spread), (-1.0, 0.0, 1.0, 0.0), (1.0, 0.5, -1.0, -0.5))
    kinds = ["tie_group", "steal_chain", "two_slot", "threshold", "ratio", "half", "two_slot",
             "tie_group", "threshold"] + (["stereo", "stereo"] if stereo else [])
    n_sites = len(b.sites) if n_sites is None else n_sites
    for g in range(n_sites):
        kind = kinds[g % len(kinds)]
        x, y = b.site()
        L = _lvl(b, sfi)
        base = int(rng.integers(len(BASES)))
        ka = KP_ANGLES[rng.integers(len(KP_ANGLES))]
        diff = (0, 0, 0, 90, 180, -30, 330)[rng.integers(7)]
        near = bool(rng.integers(2))
        lo_oct = max(L - 1, 0)
        if kind == "tie_group":
            # one contended slot, a fallback slot, a decoy two levels up; equal distances
            s = b.add_kp(x, y, L, ka, base, 0)
            b.add_kp(x + spread * 0.5, y, lo_oct, ka, base, 5, 1)
            b.add_kp(x, y + spread * 0.5, L + 2, ka, base, 0, 2)
            d0 = (10, 20, thr - 5)[rng.integers(3)]
            pat = nobs_patterns[rng.integers(len(nobs_patterns))]
            for j in range(4):
                b.add_q(x + 0.25 * j, y, L, ka + diff + (HALF_DIFFS[0] if j == 3 else 0), base, d0,
                        j, pat[j], near)
            del s
        elif kind == "steal_chain":
            b.add_kp(x, y, L, ka, base, 0)
            b.add_kp(x - spread * 0.5, y, L, ka, base, 12, 1)
            for j, pq in enumerate(((30, 20, 10), (30, 20, 20), (10, 20, 30))[rng.integers(3)]):
                b.add_q(x, y + 0.25 * j, L, ka + (diff, 90, 180)[j], base, pq, j,
                        (0, 0, 1)[j] if rng.integers(2) else 1, near)
        elif kind == "two_slot":
            # two keypoints at one distance: in two cells, one cell, equal or different levels
            ax, ay, bx, by = ties[rng.integers(len(ties))]
            oa, ob = ((L, L), (lo_oct, L), (L, lo_oct))[rng.integers(3)]
            b.add_kp(x + ax, y + ay, oa, ka, base, 3, 0)
            b.add_kp(x + bx, y + by, ob, ka + 90, base, 3, 1)
            b.add_q(x, y, L, ka + diff, base, 20, 0, int(rng.integers(2)), False)
        elif kind == "threshold":
            b.add_kp(x, y, L, ka, base, 4)
            b.add_q(x + 0.5, y - 0.5, L, ka + diff, base, thr - 4 + int(rng.integers(2)), 0, 1, near)
        elif kind == "ratio":
            # best q0, second q0 + dB: at one level or two
            q0, dB = ((40, 5), (20, 10), (20, 20), (20, 19), (36, 4))[rng.integers(5)]
            ob = (L, lo_oct)[rng.integers(2)]
            b.add_kp(x - 1.0, y, L, ka, base, 0)
            b.add_kp(x + 1.0, y, ob, ka, base, dB, 1)
            b.add_q(x, y, L, ka + diff, base, q0, 0, 1, False)
        elif kind == "half":
            hd = HALF_DIFFS[rng.integers(len(HALF_DIFFS))]
            b.add_kp(x, y, L, ka, base, 0)
            b.add_q(x, y, L, ka + hd, base, 8, 0, 1, near)
        else:  # stereo: the best keypoint's right coordinate on, past or inside the bound
            qid = len(b.q)
            kind_a = ("edge", "edge", "beyond", "zero", "inside")[rng.integers(5)]
            if kind_a == "edge":
                L = 0                             # th * mvScaleFactors[0]: an exact bound
            b.add_kp(x - 1.0, y, L, ka, base, 0, 0, (qid, kind_a))
            b.add_kp(x + 1.0, y, L, ka, base, 10, 1, (qid, "none"))
            b.add_q(x, y, L, ka + diff, base, 15, 0, 1, False)
        if kf and len(b.kp) > 380:
            break
    return b


def _fillers(b: Builder, n, flags):
    """Queries without a gadget: random places, some flagged invalid / bad / outside / behind."""
    rng = b.rng
    for j in range(n):
        flag = flags[rng.integers(len(flags))] if flags and j % 3 == 0 else None
        b.add_q(float(rng.uniform(20, 620)), float(rng.uniform(20, 460)), int(rng.integers(0, 4)),
                KP_ANGLES[rng.integers(len(KP_ANGLES))], int(rng.integers(len(BASES))),
                int(rng.integers(0, 40)), j, int(rng.integers(0, 3)), bool(rng.integers(2)), flag)


def _bins(b: Builder, spec, sfi=False):
    """Isolated (query, keypoint) pairs whose matches land in prescribed rotation bins: spec is
    a list of (angle difference in degrees, count), or (first difference, second difference,
    count) for pairs of queries on one keypoint: the first (Observations() == 0, the larger
    distance) is accepted and then stolen from / overwritten by the second, and stays in the
    histogram."""
    for entry in spec:
        if len(entry) == 3:
            for j in range(entry[2]):
                x, y = b.site()
                L = _lvl(b, sfi)
                ka = KP_ANGLES[j % len(KP_ANGLES)]
                b.add_kp(x, y, L, ka, j % len(BASES), 0)
                b.add_q(x, y, L, ka + entry[0], j % len(BASES), 30, 0, 0, True)
                b.add_q(x, y, L, ka + entry[1], j % len(BASES), 10, 1, 1, True)
            continue
        diff, count = entry
        for j in range(count):
            x, y = b.site()
            L = _lvl(b, sfi)
            ka = KP_ANGLES[(j + int(diff)) % len(KP_ANGLES)]
            base = (j + int(diff)) % len(BASES)
            b.add_kp(x, y, L, ka, base, 0)
            b.add_q(x, y, L, ka + diff, base, 8, 0, 1, True)
    return b


BIN_SPECS = (
    # equal counts: strict `>` keeps the first three bins (0, 3, 6); 9 loses; 15 deg -> bin 1
    [(0, 4), (90, 4), (180, 4), (270, 4), (15, 2)],
    # 10 vs 1: m2 == 0.1f * m1 is kept (float), as is m3; the later 1-bins lose
    [(0, 10), (90, 1), (180, 1), (270, 1), (-90, 1)],
    # 20 vs 2, with a half bin that only rounding away from zero puts outside the top three
    [(0, 20), (60, 2), (120, 2), (135, 2), (255, 1)],
    # fewer than three non-empty bins, negative differences
    [(-30, 3), (-200, 2)],
    [(15, 5), (0, 3), (30, 3), (300, 3), (-15, 1)],
    # stolen / overwritten acceptances decide the maxima: bins 0, 3, 6, 9 hold 3, 2 + 3, 1 + 3, 4
    [(0, 3), (90, 2), (180, 1), (270, 4), (90, 180, 3)],
    [(0, 10), (45, 1), (100, 1)],
    [(0, 20), (90, 2), (200, 2), (-100, 1)],
)


def _frame(b: Builder, ur=None):
    k = np.zeros(len(b.kp), KEYPOINT_DTYPE)
    for j, p in enumerate(b.kp):
        k[j] = (p["x"], p["y"], 31.0, p["ang"] % 360.0, 1.0, p["oct"], -1)
    d = np.array([p["desc"] for p in b.kp], np.uint8).reshape(-1, 32)
    return Frame(k, d, S.W, S.H, SCALE, ur)


def _shuffle_kp(b: Builder):
    """Keypoint indices in random order, so that grid order and index order differ."""
    perm = b.rng.permutation(len(b.kp))
    b.kp = [b.kp[i] for i in perm]


def _prior(rng, n):
    """frame_mp / frame_mp_obs before the call: a tenth of the slots held, some with
    Observations() == 0 (not blocking)."""
    fmp = np.where(rng.uniform(size=n) < 0.1, 7000 + np.arange(n), -1).astype(np.int32)
    fobs = np.where(fmp >= 0, rng.integers(0, 3, n), 0).astype(np.int32)
    return fmp, fobs


def _edge_value(ur, radius, kind):
    """A keypoint's mvuRight relative to a query's right coordinate `ur` and bound `radius`."""
    ur, radius = F32(ur), F32(radius)
    if kind == "none":
        return F32(-1.0)
    if kind == "zero":
        return F32(0.0)
    if kind == "inside":
        return F32(ur - radius * F32(0.5))
    if kind == "beyond":
        return F32(ur - radius - F32(1.5))
    v = F32(ur - radius)
    for _ in range(8):                        # |ur - v| == radius exactly where a float allows
        e = abs(ur - v)                       # it (level 0: radius is a small integer or x.5),
        if e == radius:                       # else the last value inside the bound
            return v
        if e < radius and abs(ur - np.nextafter(v, F32(-np.inf))) > radius:
            return v
        v = np.nextafter(v, F32(np.inf) if e > radius else F32(-np.inf))
    return v


def sfi_ties(seed, nnratio=0.9, window=10, bins=None):
    """-> dict(f1, f2, prev, window, nnratio).  nnratio > 1 makes an exact tie of the two best
    candidates acceptable, so that the candidate order decides (with nnratio <= 1 a tie always
    fails the ratio test: SearchForInitialization is then order-independent)."""
    b = Builder(1000 + seed, stride=2 if bins is not None else 1)
    if bins is not None:
        _bins(b, bins, sfi=True)
    else:
        _populate(b, TH_LOW, sfi=True)
        _fillers(b, 40, ("octave",))
        for p in b.kp[::7]:
            p["oct"] = 1 + p["oct"] % 3        # never candidates of a level-0 query
    _shuffle_kp(b)
    f2 = _frame(b)
    k1 = np.zeros(len(b.q), KEYPOINT_DTYPE)
    for j, q in enumerate(b.q):
        k1[j] = (q["x"], q["y"], 31.0, q["ang"], 1.0, 1 if q["flag"] else 0, -1)
    f1 = Frame(k1, np.array([q["desc"] for q in b.q], np.uint8).reshape(-1, 32), S.W, S.H, SCALE)
    prev = np.stack([k1["x"], k1["y"]], 1).astype(F32)
    return dict(f1=f1, f2=f2, prev=prev, window=window, nnratio=nnratio)


def sfi_prefix(c, n1=None, n2=None):
    f1, f2 = c["f1"], c["f2"]
    n1 = f1.n if n1 is None else n1
    n2 = f2.n if n2 is None else n2
    return dict(c, f1=Frame(f1.keys[:n1], f1.desc[:n1], S.W, S.H, SCALE),
                f2=Frame(f2.keys[:n2], f2.desc[:n2], S.W, S.H, SCALE), prev=c["prev"][:n1])


def _backproject(q, tcw):
    """World point that the pose projects to (q.x, q.y) at depth q.z (float64, then float)."""
    T = np.asarray(tcw, np.float64).reshape(3, 4)
    z = -q["z"] if q["flag"] == "behind" else q["z"]
    x = q["x"] + 2 * S.W if q["flag"] == "outside" else q["x"]
    pc = np.array([(x - S.CX) / S.FX * abs(z), (q["y"] - S.CY) / S.FY * abs(z), z])
    return T[:, :3].T @ (pc - T[:, 3])


def local_mps(c):
    """Frame::isInFrustum over the case's local map (Tracking.cc:1403-1438) -> MapPoints."""
    lm = c["lm"]
    inv, px, py, pxr, pl, vc = oracle.is_in_frustum(
        lm["xyz"], lm["normal"], lm["min_dist"], lm["max_dist"], lm["tcw"], c["cam"],
        (0.0, float(S.W), 0.0, float(S.H)), LOG_SCALE, 0.5)
    inv[(lm["skip"] > 0) | (lm["bad"] > 0)] = 0
    return MapPoints(px, py, pl, vc, lm["desc"], lm["nobs"], track_in_view=inv, is_bad=lm["bad"],
                     proj_xr=pxr)


def local_ties(seed, stereo=False, th=2.0, nnratio=0.8, b=None):
    """-> dict(f, lm, cam, th, nnratio): the local map as world points (identity pose) whose
    isInFrustum outputs are the SearchByProjection inputs (local_mps).  b: a Builder that
    already holds the keypoints and queries, in place of the seeded gadgets."""
    if b is None:
        b = Builder(2000 + seed)
        _populate(b, TH_HIGH, stereo=stereo, spread=6.0 if th >= 2.0 else 3.0)
        _fillers(b, 60, ("bad", "skip", "behind", "outside"))
    _shuffle_kp(b)
    tcw = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F32)
    m = len(b.q)
    xyz = np.array([_backproject(q, tcw) for q in b.q])
    dist = np.linalg.norm(xyz, axis=1)
    lvl = np.array([q["lvl"] for q in b.q])
    s = np.float64(F32(1.2))
    maxd = dist * s ** (lvl - 0.5)                 # MapPoint::PredictScale returns lvl
    d = xyz / dist[:, None]
    cosv = np.where([q["near"] for q in b.q], 1.0, 0.9)
    perp = np.cross(d, [0.3, -0.5, 0.8])
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    normal = d * cosv[:, None] + perp * np.sqrt(1 - cosv ** 2)[:, None]
    fmp, fobs = _prior(b.rng, len(b.kp))
    lm = dict(xyz=xyz.astype(F32), normal=normal.astype(F32), min_dist=(maxd / s ** 7).astype(F32),
              max_dist=maxd.astype(F32), desc=np.array([q["desc"] for q in b.q], np.uint8),
              nobs=np.array([q["nobs"] for q in b.q], np.int32),
              bad=np.array([q["flag"] == "bad" for q in b.q], np.uint8),
              skip=np.array([q["flag"] == "skip" for q in b.q], np.uint8),
              ids=(np.arange(m) + 100_000).astype(np.int32), frame_mp=fmp, frame_mp_obs=fobs,
              tcw=tcw)
    c = dict(f=_frame(b), lm=lm, cam=S.camera(), th=th, nnratio=nnratio)
    if stereo:
        mps = local_mps(c)
        ur = np.full(len(b.kp), -1.0, F32)
        for j, p in enumerate(b.kp):
            if p["ur"] is not None:
                qi, kind = p["ur"]
                r = F32(2.5) if float(mps.view_cos[qi]) > 0.998 else F32(4.0)
                if th != 1.0:
                    r = r * F32(th)
                ur[j] = _edge_value(mps.proj_xr[qi], r * SCALE[mps.pred_level[qi]], kind)
            elif j % 3 == 0:
                ur[j] = F32(p["x"] - 8.0)
        c["f"] = _frame(b, ur)
    return c


def local_prefix(c, m=None, n=None):
    f, lm = c["f"], c["lm"]
    m = len(lm["xyz"]) if m is None else m
    n = f.n if n is None else n
    out = dict(lm)
    for k in ("xyz", "normal", "min_dist", "max_dist", "desc", "nobs", "bad", "skip", "ids"):
        out[k] = np.ascontiguousarray(lm[k][:m])
    for k in ("frame_mp", "frame_mp_obs"):
        out[k] = np.ascontiguousarray(lm[k][:n])
    ur = None if f.u_right is None else f.u_right[:n]
    return dict(c, f=Frame(f.keys[:n], f.desc[:n], S.W, S.H, SCALE, ur), lm=out)


LAST_TCW = {"mono": (0.02, -0.01, 0.03), "near": (0.01, 0.0, 0.05), "forward": (0.0, 0.01, -0.3),
            "backward": (0.01, 0.0, 0.3)}


def last_ties(seed, motion="mono", th=None, bins=None, b=None):
    """-> a scenarios.sbp_last_case dict plus th, mono, frame_mp, frame_mp_obs.  motion: mono,
    near (stereo, |tlc.z| <= mb), forward, backward (tlc.z beyond mb either way).  b: as
    local_ties'."""
    mono = motion == "mono"
    th = (15.0 if mono else 7.0) if th is None else th
    if b is not None:
        pass
    elif bins is not None:
        b = Builder(3000 + seed, stride=2)
        _bins(b, bins)
    else:
        b = Builder(3000 + seed)
        _populate(b, TH_HIGH, stereo=not mono)
        _fillers(b, 60, ("invalid", "outlier", "behind", "outside"))
    _shuffle_kp(b)
    tcw = np.hstack([np.eye(3), np.array(LAST_TCW[motion])[:, None]]).astype(F32)
    n = len(b.q)
    lk = np.zeros(n, KEYPOINT_DTYPE)
    for j, q in enumerate(b.q):
        lk[j] = (q["x"], q["y"], 31.0, q["ang"], 1.0, q["lvl"], -1)
    fmp, fobs = _prior(b.rng, len(b.kp))
    if bins is not None:
        fmp[:], fobs[:] = -1, 0
    c = dict(cur=_frame(b), tcw_cur=tcw, cam=S.camera(), last_keys=lk,
             last_valid=np.array([q["flag"] != "invalid" for q in b.q], np.uint8),
             last_outlier=np.array([q["flag"] == "outlier" for q in b.q], np.uint8),
             last_xyz=np.array([_backproject(q, tcw) for q in b.q]).astype(F32).reshape(-1, 3),
             last_desc=np.array([q["desc"] for q in b.q], np.uint8).reshape(-1, 32),
             last_nobs=np.array([q["nobs"] for q in b.q], np.int32),
             tcw_last=np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F32),
             last_ids=(np.arange(n) + 500).astype(np.int32), th=th, mono=mono, frame_mp=fmp,
             frame_mp_obs=fobs)
    if not mono:
        ur = np.full(len(b.kp), -1.0, F32)
        for j, p in enumerate(b.kp):
            if p["ur"] is not None:
                qi, kind = p["ur"]
                uq = last_project(c, qi)[3]
                ur[j] = _edge_value(uq, F32(th) * SCALE[b.q[qi]["lvl"]], kind)
            elif j % 3 == 0:
                ur[j] = F32(p["x"] - 8.0)
        c["cur"] = _frame(b, ur)
    return c


def last_args(c):
    return (c["cur"], c["tcw_cur"], c["cam"], c["last_keys"], c["last_valid"], c["last_outlier"],
            c["last_xyz"], c["last_desc"], c["last_nobs"], c["tcw_last"])


def last_prefix(c, m=None, n=None):
    cur = c["cur"]
    m = len(c["last_keys"]) if m is None else m
    n = cur.n if n is None else n
    out = dict(c)
    for k in ("last_keys", "last_valid", "last_outlier", "last_xyz", "last_desc", "last_nobs",
              "last_ids"):
        out[k] = np.ascontiguousarray(c[k][:m])
    for k in ("frame_mp", "frame_mp_obs"):
        out[k] = np.ascontiguousarray(c[k][:n])
    ur = None if cur.u_right is None else cur.u_right[:n]
    out["cur"] = Frame(cur.keys[:n], cur.desc[:n], S.W, S.H, SCALE, ur)
    return out


def keyframe_ties(seed, th=3.0, orb_dist=64, cluster=0, bins=None, b=None):
    """-> a scenarios.sbp_keyframe_case dict plus th, orb_dist.  cluster = 16 / 17: one more
    point whose window holds exactly that many candidates (the fixed candidate slots hold 16).
    b: as local_ties'."""
    if b is not None:
        pass
    elif bins is not None:
        b = Builder(4000 + seed, stride=2)
        _bins(b, bins)
    else:
        b = Builder(4000 + seed)
        _populate(b, orb_dist, kf=True, spread=3.0, n_sites=len(b.sites) - 1)
        _fillers(b, 40, ("invalid", "bad", "found", "outside"))
    if cluster:
        x, y = b.site()
        for j in range(cluster):                 # a 2 px lattice inside the th * 1.2 window
            b.add_kp(x + 0.5 * (j % 5) - 1.0, y + 0.5 * (j // 5) - 1.0, 1, 30.0, 0, 1 + j % 3, j)
        b.add_q(x, y, 1, 30.0, 0, 6, 0)
    _shuffle_kp(b)
    tcw = np.hstack([np.eye(3), np.array([0.01, -0.02, 0.02])[:, None]]).astype(F32)
    n = len(b.q)
    xyz = np.array([_backproject(q, tcw) for q in b.q])
    T = tcw.astype(np.float64)
    dist = np.linalg.norm(xyz + T[:, :3].T @ T[:, 3], axis=1)   # |P - Ow|
    s = np.float64(F32(1.2))
    maxd = dist * s ** (np.array([q["lvl"] for q in b.q]) - 0.5)
    fmp = np.where(b.rng.uniform(size=len(b.kp)) < 0.1, 9000 + np.arange(len(b.kp)), -1)
    if bins is not None or cluster:
        fmp[:] = -1
    return dict(cur=_frame(b), tcw_cur=tcw, cam=S.camera(), log_scale=LOG_SCALE,
                frame_mp=fmp.astype(np.int32),
                kf_angle=np.array([q["ang"] for q in b.q], F32),
                kf_valid=np.array([q["flag"] != "invalid" for q in b.q], np.uint8),
                kf_bad=np.array([q["flag"] == "bad" for q in b.q], np.uint8),
                found=np.array([q["flag"] == "found" for q in b.q], np.uint8),
                kf_xyz=xyz.astype(F32).reshape(-1, 3),
                kf_desc=np.array([q["desc"] for q in b.q], np.uint8).reshape(-1, 32),
                kf_min=(maxd / s ** 7).astype(F32), kf_max=maxd.astype(F32),
                kf_ids=(np.arange(n) + 20_000).astype(np.int32), th=th, orb_dist=orb_dist)


def keyframe_prefix(c, m=None, n=None):
    cur = c["cur"]
    m = len(c["kf_angle"]) if m is None else m
    n = cur.n if n is None else n
    out = dict(c)
    for k in ("kf_angle", "kf_valid", "kf_bad", "found", "kf_xyz", "kf_desc", "kf_min", "kf_max",
              "kf_ids"):
        out[k] = np.ascontiguousarray(c[k][:m])
    out["frame_mp"] = np.ascontiguousarray(c["frame_mp"][:n])
    out["cur"] = Frame(cur.keys[:n], cur.desc[:n], S.W, S.H, SCALE)
    return out


def keyframe_candidates(c, i):
    """Candidate count of keyframe point i (its GetFeaturesInArea window), for the 16 / 17 case."""
    T = np.asarray(c["tcw_cur"], F32).reshape(3, 4)
    cam, cur = c["cam"], c["cur"]
    P = c["kf_xyz"][i]
    pc = rigid(T, P)
    invz = F32(1.0 / float(pc[2]))
    u = F32(cam.fx) * pc[0] * invz + F32(cam.cx)
    v = F32(cam.fy) * pc[1] * invz + F32(cam.cy)
    ow = camera_center(T)
    po = [P[j] - ow[j] for j in range(3)]
    d3 = F32(math.sqrt(sum(float(a) * float(a) for a in po)))
    lvl = int(math.ceil(F32(math.log(float(c["kf_max"][i] / d3))) / F32(c["log_scale"])))
    return len(Grid(cur).area(u, v, F32(c["th"]) * cur.scale_factors[lvl], lvl - 1, lvl + 1))
