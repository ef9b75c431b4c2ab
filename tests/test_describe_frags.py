"""Describe's matrix-core window blur, host side (orbfe_describe_blur_fragments; no device).

The two blur passes are i8 GEMMs whose additive constants ride in K slots that carry no pixel:
the row pass's raw columns 48..63 (every A fragment holds -128 there) and the column pass's R
rows j = 12..15 (constant bytes in B), so that every MFMA's C operand is 0.  This rebuilds the
fragments from the taps, checks the real slots against the taps and the spare slots' sums against
the three constants, and runs both passes in integers on random windows against the blur
written out directly (GaussianBlur 7x7's fixed-point passes, ORBextractor.cc:1088-1089).
"""
import numpy as np
import pytest

from orbslam_mapsave_amd import native

PARAMS = [(1000, 1.2, 8, 20, 7), (2000, 1.5, 4, 32, 7)]


@pytest.fixture(scope="module", params=PARAMS, ids=["s1.2_l8", "s1.5_l4"])
def built(request):
    taps, frags, pads = native.describe_blur_fragments(*request.param)
    taps = [int(t) for t in taps]
    assert taps == taps[::-1] and len(taps) == 7
    return taps, frags.astype(np.int64), pads.astype(np.int64)


def _tap(taps, d):
    return taps[3 + d] if -3 <= d <= 3 else 0


def _kc(S, x86):
    return 128 * 257 * S + (0x7fff if x86 else 0x8000)


def test_real_slots_are_the_taps(built):
    taps, fr, _ = built
    for q in range(3):
        for lane in range(64):
            n, g = lane & 15, lane >> 4
            for j in range(16):
                t, i = j >> 2, j & 3
                if g < 3:  # H_q[raw column 16 g + j][window column 16 q + n]
                    assert fr[q, lane, j] == _tap(taps, 16 * g + j - 16 * q - n - 4), (q, lane, j)
                if t < 3:  # V_q[window row 16 q + n][R row 16 t + 4 g + i]
                    assert fr[3 + q, lane, j] == _tap(taps, 16 * t + 4 * g + i - 16 * q - n - 3), (q, lane, j)


def test_spare_slots_add_the_three_constants(built):
    taps, fr, pads = built
    S = sum(taps)
    # int8 on the way out of the library: a weight that did not fit would have wrapped and
    # the sums below would miss
    assert fr.min() >= -128 and fr.max() <= 127 and pads.min() >= -128 and pads.max() <= 127
    for q in range(3):
        for n in range(16):
            # row pass: the 16 slots of lane group g = 3 meet A bytes of -128
            assert -128 * int(fr[q, n + 48, :].sum()) == 128 * S + (1 << 15), (q, n)
            for x86 in (0, 1):
                hi = sum(int(fr[3 + q, n + 16 * g, 12 + i]) * int(pads[0, x86, i])
                         for g in range(4) for i in range(4))
                lo = sum(int(fr[3 + q, n + 16 * g, 12 + i]) * int(pads[1, x86, i])
                         for g in range(4) for i in range(4))
                assert hi == _kc(S, x86) >> 8, (q, n, x86, hi)
                assert lo == _kc(S, x86) & 0xff, (q, n, x86, lo)


@pytest.mark.parametrize("x86", [0, 1], ids=["scalar", "x86"])
def test_both_passes_in_integers_match_the_direct_blur(built, x86):
    """Sums before the final rounding bit and the >> 16: (Dh << 8) + Dl of every stored element
    (window rows < 37, columns < 40) equals sum_r tap sum_k tap raw + the reading's constant."""
    taps, fr, pads = built
    rng = np.random.default_rng(5)
    for trial in range(3):
        raw = rng.integers(0, 256, (48, 48), dtype=np.int64)
        if trial == 1:
            raw[:] = 255
        if trial == 2:
            raw[:] = 0
        raw[43:, :] = 0  # rows the kernel does not load
        # row pass: A[r][k] = raw - 128 for k < 48, -128 in the spare columns
        A = np.full((48, 64), -128, np.int64)
        A[:, :48] = raw - 128
        Hm = np.zeros((64, 48), np.int64)
        for q in range(3):
            for lane in range(64):
                n, g = lane & 15, lane >> 4
                Hm[16 * g:16 * g + 16, 16 * q + n] = fr[q, lane, :]
        R = A @ Hm  # [raw row][window column], true R + 2^15
        Rt = np.zeros((48, 40), np.int64)
        for c in range(40):
            for d in range(-3, 4):
                Rt[:, c] += _tap(taps, d) * raw[:, c + 4 + d]
        assert np.array_equal(R[:43, :40], Rt[:43] + (1 << 15))
        # column pass: B's K slot (g, j = 4 t + i) = R row 16 t + 4 g + i, or the constant bytes
        lo = (R & 0xff) - 128                    # (lo ^ 0x80) as i8
        hi = ((R >> 8) & 0xff)
        hi = np.where(hi >= 128, hi - 256, hi)   # byte 1 of R as i8
        O = np.zeros((48, 48), np.int64)
        for u in range(3):
            Vm = np.zeros((16, 64), np.int64)    # [window row n][K = 16 g + j]
            for lane in range(64):
                n, g = lane & 15, lane >> 4
                Vm[n, 16 * g:16 * g + 16] = fr[3 + u, lane, :]
            Bh = np.zeros((64, 48), np.int64)
            Bl = np.zeros((64, 48), np.int64)
            for g in range(4):
                for j in range(16):
                    t, i = j >> 2, j & 3
                    if t < 3:
                        Bh[16 * g + j, :] = hi[16 * t + 4 * g + i, :]
                        Bl[16 * g + j, :] = lo[16 * t + 4 * g + i, :]
                    else:
                        Bh[16 * g + j, :] = pads[0, x86, i]
                        Bl[16 * g + j, :] = pads[1, x86, i]
            O[16 * u:16 * u + 16, :] = (((Vm @ Bh) << 8) + (Vm @ Bl)) & 0xffffffff
        Ot = np.zeros((37, 40), np.int64)
        for wr in range(37):
            for d in range(-3, 4):
                Ot[wr] += _tap(taps, d) * Rt[wr + 3 + d]
        Ot += 0x7fff if x86 else 0x8000
        assert np.array_equal(O[:37, :40], Ot)
