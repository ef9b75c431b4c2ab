"""describe_kernel's matrix-core path on small frames, byte-exact against the oracle.

The kernel blurs every keypoint's window with constants folded into spare K slots of its MFMAs,
tests the x86 reading's rounding ties once per window (a window with a tie, or one that reaches
the scalar tail columns, is blurred again with the half-to-even fix-up), keeps the never-loaded
lanes of its window registers zero across keypoints and reads the IC-angle masks from a table.
Frames of 160 x 120 and 258 x 130 (1.2 x 8) make every one of these paths carry weight at
once:

* nfeatures 90 / 150 / 500 give slot capacities (164 / 198 / 532) that are no multiple of a
  workgroup's 32 slots (8-keypoint waves) or 8 slots (2-keypoint waves), so the last workgroup
  holds waves without a slot; nfeatures 40 gives 160, every level at its minimum of 20 slots and
  whole workgroups only; a flat frame between textured ones has only empty waves, and the top
  levels are too small for any keypoint;
* keypoints within 21 px of each of the four level edges take the byte-gather window loads;
* windows hold rounding ties left of the SIMD body's end and (258 wide, one pixel of one frame
  set for it) in the tail columns.

The preconditions are asserted from the oracle alone (no GPU); the GPU cases compare all 28
bytes of every keypoint and every descriptor in both arithmetic readings: single frames
(2-keypoint waves), a batch of 9 (8-keypoint waves, strided), the batch with grouped slots
(ORBFE_DESC_STRIDE=0) and with 16-keypoint waves (ORBFE_DESC_G16=1).
"""
import numpy as np
import pytest

import oracle
from orbslam_mapsave_amd import native
from orbslam_mapsave_amd.synth import synthetic_frame

SF, NL, INI, MIN = 1.2, 8, 20, 7
SIZES = [(160, 120), (258, 130)]
NFEAT = [40, 90, 150, 500]
SEED = {(160, 120): 0, (258, 130): 0}  # first seed of the batch; chosen so the preconditions hold
FLAT = 4                                # the batch's flat frame
ARITH = {"scalar": oracle.VAR_SCALAR, "x86": oracle.VAR_X86}
ENV = ["ORBFE_DESC_STRIDE", "ORBFE_DESC_G16", "ORBFE_DESC_MFMA", "ORBFE_PREBLUR", "ORBFE_PRE_MASK",
       "ORBFE_DESC_ORDER"]
MODES = {"batch": {}, "grouped": {"ORBFE_DESC_STRIDE": "0"}, "g16": {"ORBFE_DESC_G16": "1"}}
_CACHE = {}


def frames(size):
    if ("frames", size) not in _CACHE:
        w, h = size
        f = [synthetic_frame(SEED[size] + i, w, h) for i in range(9)]
        f[FLAT] = np.full((h, w), 128, np.uint8)
        if size == (258, 130):
            # a window reaches the scalar tail columns 256 / 257 of level 0 only from a keypoint
            # at x = 238, and a tie is 1 sum in 65,536: this pixel (208 in the synthetic frame)
            # makes the sum at one such place a tie without moving the keypoints around it
            assert f[3][29, 253] == 208, "the synthetic frame changed: choose the pixel again"
            f[3][29, 253] = 216
        _CACHE["frames", size] = np.stack(f)
    return _CACHE["frames", size]


def reference(size, nf, arith):
    """The oracle's (keypoints, descriptors) of the nine frames, computed once."""
    key = ("ref", size, nf, arith)
    if key not in _CACHE:
        p = oracle.params(nf, SF, NL, INI, MIN)
        with oracle.variant(ARITH[arith]):
            _CACHE[key] = [oracle.extract(p, f) for f in frames(size)]
    return _CACHE[key]


def level_xy(kps):
    """Level coordinates of the oracle's keypoints (kp.x = x * scale[octave] in float)."""
    scale = oracle.tables(oracle.params(500, SF, NL, INI, MIN))["scale"]
    s = scale[kps["octave"]].astype(np.float64)
    return (np.rint(kps["x"] / s).astype(int), np.rint(kps["y"] / s).astype(int), kps["octave"].astype(int))


def blur_sums(level):
    """The 7 x 7 blur's 32-bit sums before rounding (BORDER_REFLECT_101, fixed-point taps)."""
    taps = [int(t) for t in native.describe_blur_fragments(500, SF, NL, INI, MIN)[0]]
    p = np.pad(level.astype(np.int64), 3, mode="reflect")
    h, w = level.shape
    rows = sum(taps[k] * p[:, k:k + w] for k in range(7))
    return sum(taps[k] * rows[k:k + h, :] for k in range(7))


def window_mask(shape, xs, ys):
    m = np.zeros(shape, bool)
    for x, y in zip(xs, ys):
        x0 = (x - 18) & ~3
        m[max(y - 18, 0):y + 19, max(x0, 0):x0 + 40] = True
    return m


# ---------------------------------------------------------------------------------------------
# preconditions, from the oracle alone

@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nf", NFEAT)
def test_partial_workgroups_and_empty_waves(size, nf):
    cap = native.keypoint_capacity(nf, SF, NL, INI, MIN, *size)
    if nf == 40:
        assert cap == 20 * NL  # every level at its minimum: whole workgroups, the seam case
    else:
        # 8-keypoint waves: 32 slots per workgroup, the last one with a wave past the end
        assert 0 < cap % 32 <= 24, cap
        # 2-keypoint waves: 8 slots per workgroup
        assert 0 < cap % 8 <= 6, cap
    ref = reference(size, nf, "x86")
    assert len(ref[FLAT][0]) == 0                          # every wave of the flat frame is empty
    assert len(ref[FLAT - 1][0]) > 0 and len(ref[FLAT + 1][0]) > 0
    for kps, _ in ref:                                     # the top levels yield no keypoint
        assert len(kps) == 0 or kps["octave"].max() < NL - 2
    assert any(len(k) and k["octave"].max() >= 2 for k, _ in ref)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_edge_windows_on_all_four_sides(size):
    p = oracle.params(500, SF, NL, INI, MIN)
    lw, lh = oracle.level_sizes(p, *size)
    sides = np.zeros(4, int)
    for kps, _ in reference(size, 500, "x86"):
        if len(kps) == 0:
            continue
        x, y, l = level_xy(kps)
        assert (x >= 19).all() and (y >= 19).all() and (x < lw[l] - 19).all() and (y < lh[l] - 19).all()
        sides += [(x < 21).sum(), (y < 21).sum(), (x + 21 >= lw[l]).sum(), (y + 21 >= lh[l]).sum()]
    assert (sides > 0).all(), sides


def _ties_in_windows(size):
    """(ties inside windows left of the SIMD body's end, ties inside windows in the tail columns)"""
    p = oracle.params(500, SF, NL, INI, MIN)
    body = tail = 0
    for f, (kps, _) in zip(frames(size), reference(size, 500, "x86")):
        if len(kps) == 0:
            continue
        x, y, l = level_xy(kps)
        with oracle.variant(oracle.VAR_H5_SSE2):
            levels = oracle.pyramid(p, f)
        for lv in np.unique(l):
            lev = levels[lv]
            xb = lev.shape[1] & ~3  # the SIMD body's end: whole groups of 4 columns
            with oracle.variant(oracle.VAR_H6_SIMD):
                b_x86 = oracle.gaussian_blur(lev)
            with oracle.variant(oracle.VAR_SCALAR):
                b_sc = oracle.gaussian_blur(lev)
            win = window_mask(lev.shape, x[l == lv], y[l == lv])
            diff = (b_x86 != b_sc) & win
            assert not diff[:, xb:].any()  # the readings differ in the body only
            body += int(diff[:, :xb].sum())
            tie = ((blur_sums(lev) & 0xffff) == 0x8000) & win
            tail += int(tie[:, xb:].sum())
    return body, tail


def test_rounding_ties_inside_windows():
    got = {s: _ties_in_windows(s) for s in SIZES}
    assert all(b > 0 for b, _ in got.values()), got  # both sizes: a tie the readings round apart
    assert any(t > 0 for _, t in got.values()), got  # one size: a tie in the scalar tail columns


# ---------------------------------------------------------------------------------------------
# the GPU against the oracle

def _same(kps, desc, okps, odesc, what):
    assert len(kps) == len(okps), (what, len(kps), len(okps))
    assert kps.tobytes() == okps.tobytes(), f"{what}: keypoints differ"
    assert np.array_equal(desc, odesc), f"{what}: {(desc != odesc).any(axis=1).sum()} descriptors differ"


def _extractor(size, nf, arith, env, monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = native.ORBextractor(nf, SF, NL, INI, MIN, device=0, max_width=size[0], max_height=size[1], max_batch=9)
    e.set_arithmetic(e.ARITH_X86_SIMD if arith == "x86" else e.ARITH_SCALAR)
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("nf", NFEAT)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_frames(size, nf, arith, monkeypatch):
    ref = reference(size, nf, arith)
    e = _extractor(size, nf, arith, {}, monkeypatch)
    try:
        for f in (0, FLAT, 8):
            kps, desc = e(frames(size)[f])
            _same(kps, desc, *ref[f], f"single frame {f}")
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("nf", NFEAT)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_of_nine(size, nf, arith, mode, monkeypatch):
    ref = reference(size, nf, arith)
    e = _extractor(size, nf, arith, MODES[mode], monkeypatch)
    try:
        kps, desc, cnt = e.extract_batch(frames(size))
        assert [int(c) for c in cnt] == [len(k) for k, _ in ref]
        for f in range(9):
            _same(kps[f, :cnt[f]], desc[f, :cnt[f]], *ref[f], f"{mode} batch frame {f}")
    finally:
        e.close()
