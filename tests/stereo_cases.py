"""Frame::ComputeStereoMatches (Frame.cc:584-756) as a pure-Python restatement written from
those lines, and crafted rectified pairs that reach its branch edges, ties and size seams on
purpose (test_stereo_edges.py; test_stereo.py uses the restatement on natural pairs).

The restatement builds its own row table, enumerates its own candidates in ascending iR, computes
its own Hamming distances and window SADs and follows the reference's float evaluation order.  It
counts the branches it takes into an optional `stats` dict and takes `mutant=`, which flips
exactly one decision (used only by the discrimination test).  Where the reference indexes out of
range or trips an OpenCV assertion it raises `Unsupported`.

Inputs are built, never extracted.  Level 0 of a pyramid is the image itself, so an octave-0 pair
is exact: the right image is the left one moved `shift` columns (per band of rows), a right
keypoint at the true column has SAD 0 at incR = 0, and `dial` raises that SAD to a chosen integer
by changing single pixels of the right window outside the centre row.  Descriptors are quantised:
a partner is its left descriptor with k bits flipped, so their distance is k exactly; the other
descriptors are random, and where hundreds of them share a band (dense_case, key16_case) they are
drawn again until each is further than TH_HIGH + 10 from every left descriptor.

Each case returns (params, imL, imR, kl, dl, kr, dr, bf, b).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import oracle
from orbslam_mapsave_amd.abi import KEYPOINT_DTYPE, ORBFE_ERR_UNSUPPORTED, ORBFE_OK, OrbfeError

F32 = np.float32
TH_HIGH = 100                                  # ORBmatcher::TH_HIGH (ORBmatcher.cc:37)
W, H = 201, 160
P = oracle.params(1000, 1.2, 8, 20, 7)
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)

MUTANTS = ("u_lo_strict", "u_hi_strict", "oct_band0", "oct_band2", "tie_last", "th_gt",
           "sad_last_min", "keep_edge_inc", "median_lo", "filter_gt", "row_round",
           "rows_round", "first64", "ir15")


class Unsupported(Exception):
    """The reference indexes a vector out of range or fails a rowRange / colRange assertion."""


def _bump(st, key, n=1):
    if st is not None and n:
        st[key] = st.get(key, 0) + int(n)


def _rnd(v):
    """std::round of a float: halves away from zero."""
    return F32(math.floor(abs(float(v)) + 0.5) * (1 if v >= 0 else -1))


def _below(v):
    return np.nextafter(F32(v), F32(-np.inf))


def _above(v):
    return np.nextafter(F32(v), F32(np.inf))


def restated(p, im_l, im_r, kl, dl, kr, dr, bf, b, stats=None, mutant=None):
    """Frame::ComputeStereoMatches restated line by line (float32 scalars, python ints)."""
    st = stats
    tab = oracle.tables(p)
    scale, inv = tab["scale"], tab["inv_scale"]
    nlev = len(scale)
    pl, pr = oracle.pyramid(p, im_l), oracle.pyramid(p, im_r)
    nl, nr = len(kl), len(kr)
    n_rows = im_l.shape[0]
    ur_out = np.full(nl, -1, F32)
    dp_out = np.full(nl, -1, F32)
    # row table (591-609)
    rows = [[] for _ in range(n_rows)]
    k_oct = kr["octave"].astype(np.int64)
    k_x = kr["x"].astype(F32)
    if nr:
        ky = kr["y"].astype(F32)
        rad = (F32(2.0) * scale[k_oct]).astype(F32)
        top, bot = (ky - rad).astype(F32), (ky + rad).astype(F32)
        lo, hi = np.floor(top).astype(np.int64), np.ceil(bot).astype(np.int64)
        r_lo = np.where(top >= 0, np.floor(top + F32(0.5)), -np.floor(-top + F32(0.5))).astype(np.int64)
        r_hi = np.floor(bot + F32(0.5)).astype(np.int64)
        _bump(st, "row_table_floor", (lo != r_lo).sum())
        _bump(st, "row_table_ceil", (hi != r_hi).sum())
        _bump(st, "row_table_oct7", (k_oct == nlev - 1).sum())
        if mutant == "rows_round":
            lo, hi = r_lo, r_hi
        if lo.min() < 0 or hi.max() >= n_rows:
            raise Unsupported("vRowIndices[yi]")
        for ir in range(nr):
            for yi in range(lo[ir], hi[ir] + 1):
                rows[yi].append(ir)
    min_d = F32(-3)
    max_d = F32(bf) / F32(b)
    acc = []
    for il in range(nl):
        lvl = int(kl["octave"][il])
        vl, ul = F32(kl["y"][il]), F32(kl["x"][il])
        if not vl > -1 or not vl < n_rows:
            raise Unsupported("vRowIndices[vL]")
        row = int(vl)                               # float -> size_t: truncation, (-1, 0) -> 0
        if int(_rnd(vl)) != row:
            _bump(st, "row_trunc")
            if mutant == "row_round":
                row = min(int(_rnd(vl)), n_rows - 1)
        if vl < 0:
            _bump(st, "row_negative_fraction")
        cand = np.asarray(rows[row], np.int64)
        if not len(cand):
            _bump(st, "row_empty")
            continue
        min_u, max_u = ul - max_d, ul - min_d
        if max_u < 0:
            _bump(st, "maxu_neg")
            continue
        if len(cand) > 64:
            _bump(st, "band_gt_64")
            if mutant == "first64":
                cand = cand[:64]
        band = {"oct_band0": 0, "oct_band2": 2}.get(mutant, 1)
        oc = k_oct[cand]
        _bump(st, "octave_edge_keep", (abs(oc - lvl) == 1).sum())
        _bump(st, "octave_edge_drop", (abs(oc - lvl) == 2).sum())
        if lvl in (0, nlev - 1):
            _bump(st, "octave_end_level", (abs(oc - lvl) <= 2).sum())
        in_oct = (oc >= lvl - 1) & (oc <= lvl + 1)
        u = k_x[cand]
        _bump(st, "u_edge_keep", (in_oct & ((u == min_u) | (u == max_u))).sum())
        _bump(st, "u_edge_drop", (in_oct & ((u == _below(min_u)) | (u == _above(max_u)))).sum())
        ok = (oc >= lvl - band) & (oc <= lvl + band)
        ok &= (u > min_u) if mutant == "u_lo_strict" else (u >= min_u)
        ok &= (u < max_u) if mutant == "u_hi_strict" else (u <= max_u)
        elig = cand[ok]
        if not len(elig):
            continue
        d = _POP[np.bitwise_xor(dr[elig], dl[il])].sum(axis=1)
        best = int(d.min())
        at = np.flatnonzero(d == best)
        if best == TH_HIGH:
            _bump(st, "best_eq_th")
        if best == TH_HIGH - 1:
            _bump(st, "best_eq_th_minus_1")
        if best > TH_HIGH or (best == TH_HIGH and mutant != "th_gt"):
            continue
        if len(at) > 1:
            _bump(st, "hamming_tie_first_wins")
        best_ir = int(elig[at[-1] if mutant == "tie_last" else at[0]])
        if best_ir >= 32768:
            _bump(st, "best_ir_ge_32768")
            if mutant == "ir15":
                best_ir &= 0x7fff
        if best_ir >= 64 and (cand[:64] != best_ir).all():
            _bump(st, "best_beyond_first_64")
        # sub-pixel match by correlation (663-735)
        if lvl < 0 or lvl >= nlev:
            raise Unsupported("mvInvScaleFactors[kpL.octave]")
        sf = inv[lvl]
        sul, svl, sur0 = _rnd(ul * sf), _rnd(vl * sf), _rnd(F32(kr["x"][best_ir]) * sf)
        PL, PR = pl[lvl], pr[lvl]                   # uint8: windows are widened where they are cut
        r0, c0 = int(svl) - 5, int(sul) - 5
        if r0 < 0 or r0 + 11 > PL.shape[0] or c0 < 0 or c0 + 11 > PL.shape[1]:
            raise Unsupported("IL rowRange / colRange")
        cols = PR.shape[1]
        if sur0 + 11 == cols - 1:
            _bump(st, "endu_edge_keep")
        if sur0 < 0 or sur0 + 11 >= cols:
            _bump(st, "endu_reject", sur0 + 11 >= cols)
            continue
        if sur0 < 10:
            raise Unsupported("IR colRange")
        IL = PL[r0:r0 + 11, c0:c0 + 11].astype(np.int64)
        IL = IL - IL[5, 5]
        dists = []
        for inc in range(-5, 6):
            cc = int(sur0) + inc - 5
            IR = PR[r0:r0 + 11, cc:cc + 11].astype(np.int64)
            dists.append(int(np.abs(IL - (IR - IR[5, 5])).sum()))
        mins = [k for k, s in enumerate(dists) if s == min(dists)]
        if len(mins) > 1:
            _bump(st, "sad_tie_first_min")
        bi = (mins[-1] if mutant == "sad_last_min" else mins[0]) - 5
        if bi in (-5, 5):
            _bump(st, "inc_edge_reject")
            if mutant != "keep_edge_inc":
                continue
        if bi in (-4, 4):
            _bump(st, "inc_pm4_keep")
        dd = [0] + dists + [0]                      # only the keep_edge_inc mutant reads the pads
        d1, d2, d3 = (F32(dd[6 + bi + k]) for k in (-1, 0, 1))
        with np.errstate(all="ignore"):
            delta = (d1 - d3) / (F32(2.0) * (d1 + d3 - F32(2.0) * d2))
        if delta < -1 or delta > 1:
            continue
        bur = scale[lvl] * ((sur0 + F32(bi)) + delta)
        disp = ul - bur
        if disp >= max_d:
            _bump(st, "disp_ge_maxd")
        if disp < 0:
            _bump(st, "disp_negative")
        if disp >= 0 and disp < max_d:
            if disp <= 0:
                _bump(st, "clamp")
                disp = F32(0.01)
                bur = F32(float(ul) - 0.01)
                if bur != ul - F32(0.01):
                    _bump(st, "clamp_double_differs")     # no float uL >= 4 does: see the test
            dp_out[il] = F32(bf) / disp
            ur_out[il] = bur
            acc.append((dists[5 + bi], il))
    # median rule (738-755)
    n = len(acc)
    if n <= 2:
        _bump(st, "median_n_small")
    _bump(st, "median_n_even" if n % 2 == 0 else "median_n_odd")
    if acc:
        acc.sort()
        med_i = acc[(n - 1) // 2 if mutant == "median_lo" else n // 2][0]
        median = F32(med_i)
        if med_i == 0:
            _bump(st, "median_zero")
        _bump(st, "median_bin0" if med_i < 256 else "median_bin_ge1")
        if sum(1 for s, _ in acc if s >> 8 == med_i >> 8) > 1:
            _bump(st, "median_shared_high_byte")
        th = (F32(1.5) * F32(1.4)) * median
        for s, il in acc:
            if s == math.ceil(float(th)) - 1:
                _bump(st, "filter_edge_keep")
            if s == math.ceil(float(th)) and med_i:
                _bump(st, "filter_edge_drop")
            if F32(s) == th and med_i:
                _bump(st, "filter_eq_th")
            if (F32(s) > th) if mutant == "filter_gt" else (not F32(s) < th):
                ur_out[il] = dp_out[il] = -1
    return ur_out, dp_out


def run_restated(c, **kw):
    """-> (status, mvuRight, mvDepth); the outputs are None where the reference is undefined."""
    try:
        return (ORBFE_OK,) + restated(*c, **kw)
    except Unsupported:
        return ORBFE_ERR_UNSUPPORTED, None, None


def run_oracle(c):
    try:
        return (ORBFE_OK,) + oracle.compute_stereo_matches(*c)
    except OrbfeError as e:
        return e.status, None, None


# ---- building blocks -------------------------------------------------------------------------------

def flipped(d, k, start=0):
    """Descriptor d with bits start .. start + k - 1 flipped: distance k from d exactly."""
    bits = np.unpackbits(d)
    bits[start:start + k] ^= 1
    return np.packbits(bits)


def texture(rng, h, w, smooth=0):
    """Random bytes; smooth > 0: a random field of that cell size, bilinearly interpolated, so
    that the higher pyramid levels keep structure."""
    if not smooth:
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    gh, gw = h // smooth + 2, w // smooth + 2
    g = rng.integers(0, 256, (gh, gw)).astype(np.float64)
    y, x = np.arange(h) / smooth, np.arange(w) / smooth
    y0, x0 = y.astype(int), x.astype(int)
    fy, fx = (y - y0)[:, None], (x - x0)[None, :]
    a = g[y0][:, x0] * (1 - fx) + g[y0][:, x0 + 1] * fx
    c = g[y0 + 1][:, x0] * (1 - fx) + g[y0 + 1][:, x0 + 1] * fx
    return np.clip(np.rint(a * (1 - fy) + c * fy), 0, 255).astype(np.uint8)


class Pair:
    """One rectified pair under construction."""

    def __init__(self, seed, w=W, h=H, shift=8, bf=50.0, b=0.1, smooth=0):
        self.rng = np.random.default_rng(seed)
        self.w, self.h, self.shift, self.bf, self.b = w, h, shift, bf, b
        self.L = texture(self.rng, h, w, smooth)
        self.R = texture(self.rng, h, w, smooth)
        self.R[:, :w - shift] = self.L[:, shift:]
        self.kl, self.dl, self.kr, self.dr = [], [], [], []

    def band_shift(self, y, s, half=8):
        """Rows y - half .. y + half of the right image are the left ones moved s columns."""
        r = slice(max(0, y - half), min(self.h, y + half + 1))
        self.R[r] = self.rng.integers(0, 256, self.R[r].shape)
        self.R[r, :self.w - s] = self.L[r, s:] if s else self.L[r]

    def patch(self, y, x0, x1, block, both=True):
        """Rows y - 5 .. y + 5, columns x0 .. x1 - 1 of the left (and right) image := block."""
        self.L[y - 5:y + 6, x0:x1] = block
        if both:
            self.R[y - 5:y + 6, x0:x1] = block

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def left(self, x, y, octave=0, d=None):
        self.kl.append((x, y, octave))
        self.dl.append(self.desc() if d is None else d)
        return len(self.kl) - 1

    def right(self, x, y, octave=0, d=None):
        self.kr.append((x, y, octave))
        self.dr.append(self.desc() if d is None else d)
        return len(self.kr) - 1

    def dial(self, xr, y, sad):
        """Raise the SAD of the right window centred (xr, y) by `sad` exactly: single pixels of
        rows above and below the centre row (which holds every window centre of the search)."""
        ys = [y + k for k in (-5, 5, -4, 4, -3, 3, -2, 2, -1, 1)]
        for yy in ys:
            for xx in range(xr - 5, xr + 6):
                if sad <= 0:
                    return
                v = min(sad, 50)
                self.R[yy, xx] = self.R[yy, xx] + v if self.R[yy, xx] <= 200 else self.R[yy, xx] - v
                sad -= v
        assert sad <= 0

    def pair(self, x, y, sad=6, off=0, shift=None, dist=0, yr=None, octr=0, d=None):
        """A left keypoint at (x, y), octave 0, and its partner `off` columns from the true
        column, with descriptor distance `dist` and window SAD `sad` at the true column."""
        s = self.shift if shift is None else shift
        d = self.desc() if d is None else d
        il = self.left(x, y, 0, d)
        xr = int(_rnd(F32(x))) - s
        self.dial(xr, int(_rnd(F32(y))), sad)
        ir = self.right(xr + off, y if yr is None else yr, octr, flipped(d, dist))
        return il, ir

    def done(self):
        def keys(v):
            k = np.zeros(len(v), KEYPOINT_DTYPE)
            for i, (x, y, o) in enumerate(v):
                k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
            k["size"], k["angle"], k["response"], k["class_id"] = 31, 0, 20, -1
            return k
        dl = np.array(self.dl, np.uint8).reshape(-1, 32)
        dr = np.array(self.dr, np.uint8).reshape(-1, 32)
        return P, self.L, self.R, keys(self.kl), dl, keys(self.kr), dr, self.bf, self.b


XS = (30, 54, 78, 102, 126, 150, 174)          # left columns 24 apart: windows and searches disjoint
YS = tuple(10 + 12 * k for k in range(12))     # rows 12 apart: windows and octave-0 bands disjoint
SLOTS = [(x, y) for y in YS for x in XS]


# ---- the crafted cases -----------------------------------------------------------------------------

MEDIAN_LISTS = {
    "n1": [7], "n1_zero": [0], "n2": [3, 10], "n2_equal": [5, 5], "n2_zero_k": [0, 9],
    "n2_zeros": [0, 0], "n3": [4, 9, 30], "n3_zero_k": [0, 4, 9], "n3_zeros_k": [0, 0, 5],
    "n4": [2, 5, 11, 12], "n5_equal": [6] * 5, "n5_zero_median": [0, 0, 0, 4, 9],
    "same_high_byte": [300, 310, 320, 700], "bins_0_1_2": [10, 300, 520, 600, 1300],
    "bin1_pair": [260, 270, 300, 500, 560], "floor_ceil_th": [1, 7, 7, 14, 15],
    "floor_ceil_th_11": [1, 1, 1, 7, 7, 7, 7, 14, 14, 15, 15], "n4_zeros": [0, 0, 0, 8],
    "bin2": [256, 511, 512, 767, 768], "bin3_low_edge": [255, 256, 768, 769, 1023],
    # 1.5f * 1.4f * 10 = 21 and * 20 = 42 exactly: SAD == thDist is dropped by the strict '<'
    "equal_th_21": [10] * 7 + [21] * 3 + [20] * 2, "equal_th_42": [20] * 6 + [42] * 3 + [41, 43],
}


def median_case(name):
    sads = MEDIAN_LISTS[name]
    c = Pair(100 + sorted(MEDIAN_LISTS).index(name))
    order = c.rng.permutation(len(sads))          # iL order is not the SAD order
    for k, i in enumerate(order):
        x, y = SLOTS[(5 * k + 3) % len(SLOTS)]
        c.pair(x, y, sad=sads[i])
    return c.done()


def identical_case():
    """imR == imL with every keypoint its own partner: disparity 0 clamps, every SAD is 0, the
    median is 0 and the strict '<' drops every match."""
    c = Pair(7, shift=0)
    for x, y in SLOTS[::9]:
        c.pair(x, y, sad=0)
    return c.done()


def _clamp_blocks(rng, x0, want):
    """Random 11 x 21 blocks for a window centred on column x0 and the uR their parabola offset
    gives: a left keypoint at x = uR has a disparity of exactly 0 at a fractional uL."""
    blk = rng.integers(0, 256, (want, 11, 21)).astype(np.int64)
    ref = blk[:, :, 5:16] - blk[:, 5:6, 10:11]
    d1 = np.abs(ref - (blk[:, :, 4:15] - blk[:, 5:6, 9:10])).sum((1, 2)).astype(F32)
    d3 = np.abs(ref - (blk[:, :, 6:17] - blk[:, 5:6, 11:12])).sum((1, 2)).astype(F32)
    delta = ((d1 - d3) / (F32(2.0) * (d1 + d3 - F32(0.0)))).astype(F32)
    ur = ((F32(x0) + F32(0.0)) + delta).astype(F32)
    return [(blk[i].astype(np.uint8), ur[i]) for i in range(want)]


def clamp_case():
    """Disparity exactly 0 -> disparity 0.01, uR = uL - 0.01 evaluated in double."""
    c = Pair(11)
    sym = c.rng.integers(0, 256, (11, 21)).astype(np.uint8)
    sym[:, 11:] = sym[:, 9::-1]                   # mirror-symmetric about its centre column
    for k, ul in enumerate((100, 57, 151)):       # d1 == d3: delta 0, uR == uL, an integer
        y = YS[k]
        c.patch(y, ul - 10, ul + 11, sym)
        d = c.desc()
        c.left(ul, y, 0, d)
        c.right(ul, y, 0, d)
    for k, (blk, ur) in enumerate(_clamp_blocks(c.rng, 12, 5)):
        y = YS[3 + k]
        c.patch(y, 2, 23, blk)
        d = c.desc()
        c.left(ur, y, 0, d)
        c.right(12, y, 0, d)
    for k in range(10):                           # SADs > 0, so the median is not 0
        x, y = XS[2 + k % 5], YS[8 + k // 3]
        c.pair(x, y, sad=6)
    return c.done()


def inc_case():
    """bestincR = +-4 (kept) and +-5 (dropped), a flat window (every incR tied at 0: the first
    minimum is incR = -5), and windows of horizontal period 4 (incR = -4, 0, 4 tied)."""
    c = Pair(12)
    for k, off in enumerate((4, -4, 5, -5) * 3):
        x, y = XS[1 + k % 4], YS[k // 4]
        c.pair(x, y, sad=6, off=off)
    for k in range(5):
        x, y = XS[k], YS[4]
        c.patch(y, x - 24, x + 12, 90)
        c.pair(x, y, sad=0)
    per = c.rng.integers(0, 256, (11, 4)).astype(np.uint8)
    for k in range(6):
        x, y = XS[1 + k % 3 * 2], YS[6 + k // 3 * 2]
        c.patch(y, x - 24, x + 12, np.tile(per, 9))
        c.pair(x, y, sad=0)
        xr = x - c.shift
        c.R[y - 5, xr - 1:xr + 2] += np.uint8(2)   # in the windows of incR -4, 0 and 4 alike
    for k in range(4):
        c.pair(XS[k], YS[10], sad=6)
    return c.done()


def dense_case(kind):
    """>= 200 right keypoints in the row band of six left keypoints.  `best_hi`: the partner is
    the unique best at an index >= 128; `tie`: partner and a decoy 8 px off at distance 3 each,
    one below index 64 and one above (first iR wins: the partner for three left keypoints, the
    decoy for the other three); `th`: the best at TH_HIGH - 1 and at TH_HIGH exactly."""
    c = Pair(20 + ("best_hi", "tie", "th", "th2").index(kind))
    y = 70
    lefts = []
    while len(lefts) < 6:
        d = c.desc()
        if all(int(_POP[d ^ q].sum()) > TH_HIGH + 10 for q in lefts):
            lefts.append(d)
    decoys = []
    while len(decoys) < 210:
        d = c.desc()
        if min(int(_POP[d ^ q].sum()) for q in lefts) > TH_HIGH + 10:
            decoys.append(d)
    early = (0, 2, 4) if kind == "tie" else ()      # partners that sit below index 64
    for k in early:
        c.pair(XS[k], y + k % 3 - 1, sad=6, dist=3, d=lefts[k])
    first_decoy = len(c.kr)
    for k, d in enumerate(decoys):
        c.right(F32(12 + (k * 37) % 150 + 0.25), y + (k % 5 - 2) * 0.5, k % 2, d)
    for k in range(6):
        if k not in early:
            dist = {"best_hi": 0, "tie": 3, "th": (TH_HIGH - 1, TH_HIGH)[k % 2],
                    "th2": (TH_HIGH, TH_HIGH - 1)[k % 2]}[kind]
            c.pair(XS[k], y + k % 3 - 1, sad=6, dist=dist, d=lefts[k])
    if kind == "tie":
        for k in range(6):
            slot = first_decoy + (100 + k if k in early else 10 + k)
            c.kr[slot] = (F32(XS[k] - c.shift - 8), y, 0)
            c.dr[slot] = flipped(lefts[k], 3, start=40)
    return c.done()


def key16_case():
    """nr = 65535: the unique best at indices up to 65534, and a tie between 40000 and 65533."""
    c = Pair(30)
    y = 70
    xs = XS[:6]
    lefts = [c.desc() for _ in xs]
    nr = 65535
    dr = c.rng.integers(0, 256, (nr, 32)).astype(np.uint8)
    while True:
        near = np.zeros(nr, bool)
        for q in lefts:
            near |= _POP[dr ^ q].sum(1) <= TH_HIGH + 10
        if not near.any():
            break
        dr[near] = c.rng.integers(0, 256, (int(near.sum()), 32))
    kx = (12 + c.rng.integers(0, 600, nr) * 0.25).astype(F32)
    ky = (y + c.rng.integers(-4, 5, nr) * 0.5).astype(F32)
    ko = c.rng.integers(0, 2, nr)
    for k, (x, idx, dist) in enumerate(zip(xs, (65534, 40000, 100, 32768, 50000, 65532),
                                           (0, 3, 0, 0, 1, 2))):
        c.left(x, y + k % 3 - 1, 0, lefts[k])
        xr = x - c.shift
        c.dial(xr, y + k % 3 - 1, 6)
        kx[idx], ky[idx], ko[idx], dr[idx] = xr, y, 0, flipped(lefts[k], dist)
    kx[65533], ky[65533], ko[65533], dr[65533] = 20, y, 0, flipped(lefts[1], 3, start=40)
    c.kr = list(zip(kx, ky, ko))
    c.dr = list(dr)
    return c.done()


def ubounds_case():
    """maxD = 16: right x exactly at minU = uL - 16 and maxU = uL + 3 (kept) and one ulp outside
    each (dropped); maxU < 0; maxU == 0."""
    c = Pair(40, bf=16.0, b=1.0)
    for k in range(12):
        x, y = F32(XS[2 + k % 4] + (0.25 if k % 3 == 2 else 0)), YS[k]
        d = c.desc()
        c.left(x, y, 0, d)
        lo = k % 4 < 2
        s = 13 if lo else 1                        # true column 3 right of minU / 4 left of maxU
        c.band_shift(y, s, half=5)
        c.dial(int(_rnd(x)) - s, y, 6)
        edge = F32(x) - F32(16) if lo else F32(x) + F32(3)
        c.right(edge if k % 2 == 0 else (_below(edge) if lo else _above(edge)), y, 0, d)
    for k, ul in enumerate((-4.0, -3.5, -10.0, float(_below(-3.0)), -3.0, -64.0, -3.25)):
        c.left(ul, YS[k], 0, c.dr[k])
    return c.done()


def disparity_case():
    """maxD = 16 and true disparities of 17 .. 19 px (disparity >= maxD), -1 .. -3 px
    (disparity < 0) and 15 px (kept)."""
    c = Pair(41, bf=16.0, b=1.0)
    for k, s in enumerate((17, 18, 19, 17, 18, 19, 15, 15, 14)):
        x, y = XS[3 + k % 3], YS[k]
        c.band_shift(y, s, half=5)
        d = c.desc()
        c.left(x, y, 0, d)
        c.dial(x - s, y, 6)
        c.right(x - 16 + k % 2, y, 0, d)
    for k in range(6):
        s, x, y = 1 + k % 3, XS[1 + 3 * (k // 3)], YS[9 + k % 3]
        if k < 3:
            c.R[y - 5:y + 6] = c.rng.integers(0, 256, (11, c.w))
            c.R[y - 5:y + 6, s:] = c.L[y - 5:y + 6, :c.w - s]     # the right image moved right
        d = c.desc()
        c.left(x, y, 0, d)
        c.dial(x + s, y, 6)
        c.right(x + s, y, 0, d)
    return c.done()


def octave_case():
    """Right octaves lvl - 2 .. lvl + 2 at lvl = 0, 3 and 7.  Each left keypoint has a fallback
    partner at its own level (distance 50) and one nearer decoy (distance k) per other octave:
    the +-1 decoys win, the +-2 ones are not candidates."""
    c = Pair(50, smooth=6)
    s = c.shift
    rows = {0: (YS[0], YS[11], YS[10]), 3: YS[1:6], 7: YS[6:9]}
    for lvl, x in ((0, 102), (3, 100), (7, 84)):
        offs = [do for do in (-2, -1, 1, 2, 0) if 0 <= lvl + do <= 7]
        for y, do in zip(rows[lvl], offs):
            for rep in range(2):
                d = c.desc()
                xx = x + 24 * rep
                c.left(xx, y, lvl, d)
                if lvl == 0:
                    c.dial(xx - s, y, 6)
                c.right(xx - s, y, lvl, flipped(d, 50))
                if do:
                    c.right(xx - s - (16 if lvl < 7 else 24), y, lvl + do, flipped(d, 5))
    return c.done()


def endu_case():
    """scaleduR0 + 11 == cols - 1 (kept), cols and cols + 1 (dropped) at levels 1, 2 and 3."""
    c = Pair(51, shift=4, smooth=5)
    lw, _ = oracle.level_sizes(P, W, H)
    sc = oracle.tables(P)["scale"]
    row = 0
    for lvl in (1, 2, 3):
        for over in (-1, 0, 1, -1):
            sur0 = int(lw[lvl]) + over - 11
            xr = F32(sur0) * sc[lvl]
            assert _rnd(xr * oracle.tables(P)["inv_scale"][lvl]) == sur0
            y = YS[row]
            row += 1
            d = c.desc()
            c.left(xr + F32(c.shift), y, lvl, d)
            c.right(xr, y, lvl, d)
    return c.done()


def rowtable_case():
    """Fractional right y at every octave with left keypoints on floor(y - r), ceil(y + r) and
    the rows just outside; fractional left y (the row is the truncation); rows with no candidate."""
    c = Pair(52, smooth=6)
    sc = oracle.tables(P)["scale"]
    s = c.shift
    for o in range(8):
        yr = F32(80.3 if o % 2 else 79.6)
        r = F32(2.0) * sc[o]
        lo, hi = math.floor(yr - r), math.ceil(yr + r)
        lvl = 0 if o < 2 else o - 1
        x = 40 + 18 * o if o < 2 else 60 + 10 * o
        d = c.desc()
        c.right(x - s, yr, o, d)
        for yl in (lo - 1, lo, hi, hi + 1, lo + 0.75, hi + 0.75):
            c.left(x, yl, lvl, d)
            if lvl == 0:
                c.dial(x - s, int(_rnd(F32(yl))), 2)
    for k in range(4):                              # octave-0 pairs: band 2 rows each way
        x = XS[k]
        for yl, yr in ((20.6, 18.0), (20.4, 22.0), (140.5, 138.0), (140.49, 142.4)):
            c.pair(x, yl, sad=3, yr=yr)
    return c.done()


TALL_WIDTH = {1100: 640, 2049: 1152, 4096: 2176}


def tall_case(h):
    """A frame of h rows, octave-0 pairs in the first, middle and last rows a band may touch and
    on each side of every run boundary of the row scan.  The extractor refuses a frame whose
    round(width / height) of a level with FAST cells is 0 (the reference divides by it), so the
    widths are just over half the heights."""
    c = Pair(60 + h % 7, w=TALL_WIDTH[h], h=h)
    per = -(-h // 1024)
    marks = {5, 6, 17, h // 2 - 12, h // 2, h // 2 + 12, h - 6, h - 18, h - 30}
    for t in (256, 512, 768):
        for dy in (-13, -1, 12):
            marks.add(t * per + dy)
    for k in (1023, 1024, 2047, 2048, 3071, 3072):
        if k + 30 < h:
            marks |= {k - 12, k, k + 12}
    for k, y in enumerate(sorted(m for m in marks if 5 <= m <= h - 6)):
        x = (48, 100)[k % 2]
        c.pair(x, y, sad=4 + k % 3, yr=y + (k % 3 - 1) * 1.5)
    c.right(30, 2.0)                                # its band touches row 0
    c.right(30, h - 3.0)                            # ... and row h - 1
    return c.done()


def unsupported_case(kind):
    """Inputs on which the reference is undefined (status only) and their defined neighbours."""
    c = Pair(70)
    for k in range(4):
        c.pair(XS[1 + k], YS[6 + k], sad=6)
    d = c.desc()
    if kind == "right_band_above":
        c.right(60, 1.5)
    elif kind == "right_band_below":
        c.right(60, H - 2.5)
    elif kind == "right_band_below_oct7":
        c.right(60, H - 8.0, 7)
    elif kind == "right_strip_left":               # scaleduR0 = 9: colRange(-1, ...)
        c.left(17, 34, 0, d), c.right(9, 34, 0, d)
    elif kind == "left_window_left":
        c.left(4, 34, 0, d), c.right(6, 34, 0, d)
    elif kind == "left_window_below":
        c.left(60, H - 5, 0, d), c.right(52, H - 6, 0, d)
    elif kind == "left_octave_8":                  # a candidate at octave 7 matches it
        c.left(60, 34, 8, d), c.right(52, 34, 7, d)
    elif kind == "left_octave_m1":
        c.left(60, 34, -1, d), c.right(52, 34, 0, d)
    elif kind == "left_row_negative_matched":      # vL = -0.5 reads row 0, then rowRange(-6, ...)
        c.left(60, -0.5, 0, d), c.right(52, 2.0, 0, d)
    elif kind == "ok_left_row_negative_empty":     # vL in (-1, 0) is row 0; nothing there
        for vl in (-0.5, -0.99, -0.25, -0.75, -1e-6):
            c.left(60, vl, 0, d)
        c.right(52, 3.0, 0, d)
    elif kind == "ok_left_row_negative_unmatched":
        c.left(60, -0.5, 0, d), c.right(52, 2.0, 0, flipped(d, TH_HIGH))
    elif kind == "ok_left_octave_far":             # no candidate octave: the level is never used
        c.left(60, 34, 9, d), c.left(60, 34, -2, d), c.right(52, 34, 7, d), c.right(52, 34, 0, d)
    else:
        raise KeyError(kind)
    return c.done()


UNSUPPORTED = ("right_band_above", "right_band_below", "right_band_below_oct7", "right_strip_left",
               "left_window_left", "left_window_below", "left_octave_8", "left_octave_m1",
               "left_row_negative_matched")
DEFINED_NEIGHBOURS = ("ok_left_row_negative_empty", "ok_left_row_negative_unmatched",
                      "ok_left_octave_far")

CASES = {f"median_{k}": functools.partial(median_case, k) for k in MEDIAN_LISTS}
CASES.update(identical=identical_case, clamp=clamp_case, inc=inc_case,
             dense_best_hi=functools.partial(dense_case, "best_hi"),
             dense_tie=functools.partial(dense_case, "tie"),
             dense_th=functools.partial(dense_case, "th"),
             dense_th2=functools.partial(dense_case, "th2"), ubounds=ubounds_case,
             disparity=disparity_case, octave=octave_case, endu=endu_case, rowtable=rowtable_case)
CASES.update({k: functools.partial(unsupported_case, k) for k in DEFINED_NEIGHBOURS})
BIG = {"key16": key16_case}
TALL = {f"tall_{h}": functools.partial(tall_case, h) for h in (1100, 2049, 4096)}
STATUS_ONLY = {k: functools.partial(unsupported_case, k) for k in UNSUPPORTED}


@functools.lru_cache(maxsize=None)
def get(name):
    for table in (CASES, BIG, TALL, STATUS_ONLY):
        if name in table:
            return table[name]()
    raise KeyError(name)
