"""Frame::ComputeStereoMatches at its branch edges, ties and size seams (stereo_cases.py).

CPU: the C oracle against the restatement, on float bits, on every crafted case; the crafted cases
reach every edge branch at least five times (counted by the restatement); every single-decision
mutant of the restatement changes the answer on at least one crafted case, so a kernel with that
slip would fail the GPU tests below.  GPU: every crafted case through the host ABI (frame 0, frame
2 of a batched extraction, short and unequal counts) and through the device batch, bit-exact on
mvuRight / mvDepth against the oracle, and the status codes of the undefined inputs.

Branch counts over the crafted cases (restatement), floor 5 each:
  band_gt_64 30, best_beyond_first_64 18, hamming_tie_first_wins 7, best_eq_th 7,
  best_eq_th_minus_1 6, best_ir_ge_32768 5, octave_edge_keep / drop > 50 each, u_edge_keep 629,
  u_edge_drop 6, maxu_neg 6, endu_edge_keep 6, endu_reject 6, inc_edge_reject 19, inc_pm4_keep 17,
  sad_tie_first_min 11, clamp 8, disp_ge_maxd 6, disp_negative 11, median_n_small 6,
  median_n_even 23, median_n_odd 18, median_zero 6, median_bin0 33, median_bin_ge1 8,
  median_shared_high_byte 39, filter_edge_keep 6, filter_edge_drop 11, filter_eq_th 6,
  row_trunc 28, row_negative_fraction 6, row_empty 8, row_table_floor / ceil > 10000 each,
  row_table_oct7 8.
No counter, because unreachable:
  * `deltaR < -1 || deltaR > 1`: dist2 is a minimum of the eleven SADs, so |dist1 - dist3| <=
    dist1 + dist3 - 2 dist2 and |deltaR| <= 0.5; a 0 / 0 plateau gives NaN, which passes both
    comparisons and fails `disparity >= 0`.
  * uL - 0.01 in double against float: within one binade of uL the distance of uL - 0.01 to the
    next rounding midpoint is constant, and for every binade from 4 (the window needs uL >= 4.5)
    to 4096 it is far more than the 2.2e-10 between 0.01 and 0.01f, so both evaluations round to
    the same float (test_clamp_in_double_equals_float_for_every_reachable_ul); the clamp itself
    is pinned by the `clamp` case at integer and fractional uL.
  * plan.h > 4096 in the stereo entry points: the extractor refuses such a frame first
    (test_gpu_4097_rows_refused).
"""
import numpy as np
import pytest

import stereo_cases as SC
from orbslam_mapsave_amd.abi import ORBFE_ERR_UNSUPPORTED, ORBFE_OK, OrbfeError

F32 = np.float32
ALL = list(SC.CASES) + list(SC.BIG) + list(SC.TALL)
SENTINEL = F32(-7.5)

REACH = ("band_gt_64", "best_beyond_first_64", "hamming_tie_first_wins", "best_eq_th",
         "best_eq_th_minus_1", "best_ir_ge_32768", "octave_edge_keep", "octave_edge_drop",
         "octave_end_level", "u_edge_keep", "u_edge_drop", "maxu_neg", "endu_edge_keep",
         "endu_reject", "inc_edge_reject", "inc_pm4_keep", "sad_tie_first_min", "clamp",
         "disp_ge_maxd", "disp_negative", "median_n_small", "median_n_even", "median_n_odd",
         "median_zero", "median_bin0", "median_bin_ge1", "median_shared_high_byte",
         "filter_edge_keep", "filter_edge_drop", "filter_eq_th", "row_trunc",
         "row_negative_fraction", "row_empty", "row_table_floor", "row_table_ceil",
         "row_table_oct7")


def same(a, b):
    """(status, mvuRight, mvDepth) equal: the status, and on ORBFE_OK the float bits."""
    if a[0] != b[0]:
        return False
    return a[0] != ORBFE_OK or all(
        np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[1:], b[1:]))


def cut(c, nl=None, nr=None):
    p, L, R, kl, dl, kr, dr, bf, b = c
    return p, L, R, kl[:nl], dl[:nl], kr[:nr], dr[:nr], bf, b


# ---- CPU -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_oracle_vs_restated(name):
    c = SC.get(name)
    o = SC.run_oracle(c)
    assert o[0] == ORBFE_OK
    assert same(SC.run_restated(c), o)


@pytest.mark.parametrize("name", list(SC.STATUS_ONLY))
def test_oracle_vs_restated_undefined_inputs(name):
    """Status only: the oracle returns at the first undefined step."""
    c = SC.get(name)
    assert SC.run_oracle(c)[0] == SC.run_restated(c)[0] == ORBFE_ERR_UNSUPPORTED
    assert SC.run_oracle(cut(c, 4, 4))[0] == ORBFE_OK   # the case without its offending keypoints


def test_known_answers():
    """Figures worked out by hand: uL = 100 clamps to uR = 99.99 and depth bf / 0.01; a median
    of 0 drops every match; 1.5f * 1.4f * 10 is 21 exactly."""
    _, ur, dp = SC.run_oracle(SC.get("clamp"))
    assert ur[0] == F32(100.0 - 0.01) and dp[0] == F32(50.0) / F32(0.01) == F32(5000.0)
    _, ur, dp = SC.run_oracle(SC.get("identical"))
    assert (ur == -1).all() and (dp == -1).all()
    assert F32(1.5) * F32(1.4) * F32(10) == 21 and F32(1.5) * F32(1.4) * F32(20) == 42
    for name in ("tall_1100", "tall_2049", "tall_4096", "key16", "dense_best_hi"):
        _, ur, dp = SC.run_oracle(SC.get(name))
        assert (ur >= 0).all(), name                  # every crafted pair of these is matched


def test_crafted_cases_reach_every_branch():
    """A condition on the inputs: the restatement alone counts the branches it takes."""
    stats = {}
    for name in ALL:
        SC.run_restated(SC.get(name), stats=stats)
    print({k: stats.get(k, 0) for k in sorted(stats)})
    for k in REACH:
        assert stats.get(k, 0) >= 5, (k, stats)
    assert stats.get("clamp_double_differs", 0) == 0


@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_every_mutant_changes_an_answer(mutant):
    """One flipped decision in the restatement shows on at least one crafted case: the GPU parity
    tests on these cases would fail for a kernel with that slip.  `first64` is a kernel that
    drops candidates 64 and up, `rows_round` / a wrong run scan show on the tall cases' matches."""
    hit = [n for n in ALL if not same(SC.run_restated(SC.get(n), mutant=mutant),
                                      SC.run_restated(SC.get(n)))]
    print(mutant, hit)
    assert hit


def test_clamp_in_double_equals_float_for_every_reachable_ul():
    """(float)((double)uL - 0.01) == uL - 0.01f wherever a window fits (see the module docstring):
    the start of every binade, where the result's exponent drops, and a sample of the rest."""
    rng = np.random.default_rng(0)
    for e in range(2, 12):
        lo = F32(2.0 ** e)
        ulp = np.spacing(lo)
        ul = np.concatenate([lo + ulp * np.arange(40000, dtype=np.float64),
                             lo + ulp * rng.integers(0, 2 ** 23, 20000)]).astype(F32)
        assert np.array_equal((ul.astype(np.float64) - 0.01).astype(F32), ul - F32(0.01)), e


# ---- GPU -------------------------------------------------------------------------------------------

class Handles:
    """Two extractor handles per image size, made on first use."""

    def __init__(self):
        self.h = {}

    def get(self, w, h):
        from orbslam_mapsave_amd.native import ORBextractor
        batch = 48 if h <= 200 else 4
        if (w, h) not in self.h:
            self.h[w, h] = tuple(ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_width=w,
                                              max_height=h, max_batch=batch) for _ in range(2))
        return self.h[w, h]

    def close(self):
        for pair in self.h.values():
            for e in pair:
                e.close()


@pytest.fixture(scope="module")
def handles():
    hs = Handles()
    yield hs
    hs.close()


def g_host(hs, c, frame=0):
    """The host ABI on case c -> (status, mvuRight, mvDepth); frame > 0: the pair is frame `frame`
    of a batched extraction whose other frames hold another pair."""
    p, L, R, kl, dl, kr, dr, bf, b = c
    el, er = hs.get(L.shape[1], L.shape[0])
    if frame == 0:
        el(L), er(R)
    else:
        other = SC.get("median_n4" if L.shape == (SC.H, SC.W) else "tall_%d" % L.shape[0])
        il = np.stack([other[2]] * frame + [L])
        ir = np.stack([other[1]] * frame + [R])
        el.extract_batch(il), er.extract_batch(ir)
    try:
        return (ORBFE_OK,) + el.ComputeStereoMatches(er, kl, dl, kr, dr, bf, b, frame=frame)
    except OrbfeError as e:
        return e.status, None, None


@pytest.mark.gpu
@pytest.mark.parametrize("frame", [0, 2])
def test_gpu_host_abi(handles, frame):
    """Every crafted case, consecutively on one pair of handles per size."""
    for name in ALL:
        assert same(g_host(handles, SC.get(name), frame), SC.run_oracle(SC.get(name))), name


@pytest.mark.gpu
def test_gpu_host_abi_short_and_unequal_counts(handles):
    """nl in {1, 2, 3, 5} (not a multiple of 4), nl > nr and nr > nl: the slabs are max(nl, nr)
    apart."""
    for name in ("median_bins_0_1_2", "clamp", "inc", "rowtable", "dense_tie", "tall_2049"):
        c = SC.get(name)
        for nl, nr in ((1, None), (2, None), (3, None), (5, None), (None, 3), (5, 2), (2, 5)):
            cc = cut(c, nl, nr)
            assert same(g_host(handles, cc), SC.run_oracle(cc)), (name, nl, nr)
    c = SC.get("median_n4")
    assert same(g_host(handles, cut(c, None, 0)), SC.run_oracle(cut(c, None, 0)))
    assert g_host(handles, cut(c, 0, None))[0] == ORBFE_OK


@pytest.mark.gpu
def test_gpu_undefined_inputs_report_unsupported_and_reset(handles):
    """Each undefined input reports ORBFE_ERR_UNSUPPORTED; the next clean call reports ORBFE_OK
    and the oracle's answer."""
    clean = SC.get("median_n4")
    for name in SC.STATUS_ONLY:
        assert g_host(handles, SC.get(name))[0] == ORBFE_ERR_UNSUPPORTED, name
        assert same(g_host(handles, clean), SC.run_oracle(clean)), name


@pytest.mark.gpu
def test_gpu_65536_right_keypoints_refused(handles):
    """The candidate key packs iR in 16 bits: nr = 65535 is served (key16), 65536 refused."""
    p, L, R, kl, dl, kr, dr, bf, b = SC.get("key16")
    kr2, dr2 = np.concatenate([kr, kr[:1]]), np.concatenate([dr, dr[:1]])
    assert g_host(handles, (p, L, R, kl, dl, kr2, dr2, bf, b))[0] == ORBFE_ERR_UNSUPPORTED
    assert same(g_host(handles, SC.get("key16")), SC.run_oracle(SC.get("key16")))
    el, er = handles.get(SC.W, SC.H)
    with pytest.raises(OrbfeError) as e:                  # refused before any pointer is read
        el.compute_stereo_matches_device(er, 1, 256, 256, 256, 256, 256, 256, 65536, bf, b, 256, 256)
    assert e.value.status == ORBFE_ERR_UNSUPPORTED


@pytest.mark.gpu
def test_gpu_4097_rows_refused(handles):
    """A 4097-row frame never reaches the stereo kernels' 4096-row LDS table: the extractor
    refuses it, and the handles go on serving 4096 rows."""
    c = SC.get("tall_4096")
    el, er = handles.get(c[1].shape[1], 4096)
    with pytest.raises(OrbfeError) as e:
        el(np.zeros((4097, c[1].shape[1]), np.uint8))
    assert e.value.status == ORBFE_ERR_UNSUPPORTED
    assert same(g_host(handles, c), SC.run_oracle(c))


def device_batch(hs, cases, cap, extra=()):
    """orbfe_compute_stereo_matches_device on the cases stacked as frames of one call, plus the
    `extra` frames (case, nl, nr) whose counts are overridden -> per frame (count, uR, depth)."""
    import torch
    dev = torch.device("cuda", 0)
    frames = [(c, len(c[3]), len(c[5])) for c in cases] + list(extra)
    n = len(frames)
    h, w = frames[0][0][1].shape
    el, er = hs.get(w, h)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    slab = {k: np.zeros((n, cap), SC.KEYPOINT_DTYPE) for k in "lr"}
    desc = {k: np.zeros((n, cap, 32), np.uint8) for k in "lr"}
    cnt = {k: np.zeros(n, np.int32) for k in "lr"}
    for f, (c, nl, nr) in enumerate(frames):
        for k, keys, d, m in (("l", c[3], c[4], nl), ("r", c[5], c[6], nr)):
            m_in = min(m, cap, len(keys))
            slab[k][f, :m_in], desc[k][f, :m_in], cnt[k][f] = keys[:m_in], d[:m_in], m
    imgs = {k: up(np.stack([c[i] for c, _, _ in frames])) for k, i in (("l", 1), ("r", 2))}
    ecap = el.capacity(w, h)
    scratch = [torch.zeros(n * ecap * 28, dtype=torch.uint8, device=dev),
               torch.zeros(n * ecap * 32, dtype=torch.uint8, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev)]
    for k, e in (("l", el), ("r", er)):
        e.extract_batch_device(imgs[k].data_ptr(), n, w, h, w, w * h, scratch[0].data_ptr(), ecap,
                               scratch[1].data_ptr(), scratch[2].data_ptr())
        e.synchronize()
    D = {k: (up(slab[k]), up(desc[k]), up(cnt[k])) for k in "lr"}
    ur = torch.full((n, cap), float(SENTINEL), dtype=torch.float32, device=dev)
    dp = torch.full((n, cap), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    bf, b = frames[0][0][7], frames[0][0][8]
    assert all(c[7] == bf and c[8] == b for c, _, _ in frames)
    el.compute_stereo_matches_device(er, n, *(t.data_ptr() for t in D["l"]),
                                     *(t.data_ptr() for t in D["r"]), cap, bf, b,
                                     ur.data_ptr(), dp.data_ptr())
    try:
        el.stereo_status()
        st = ORBFE_OK
    except OrbfeError as e:
        st = e.status
    return st, frames, ur.cpu().numpy(), dp.cpu().numpy()


def check_device_batch(hs, names, cap, with_odd_frames=True):
    cases = [SC.get(n) for n in names]
    big = max(cases, key=lambda c: len(c[3]))
    extra = []
    if with_odd_frames:
        p, L, R, kl, dl, kr, dr, bf, b = big            # the count says more than the slab holds
        rep = -(-cap // len(kl))
        over = (p, L, R, np.concatenate([kl] * rep)[:cap], np.concatenate([dl] * rep)[:cap],
                kr, dr, bf, b)
        extra = [(cases[0], 0, len(cases[0][5])), (cases[0], len(cases[0][3]), 0),
                 (over, cap + 7, len(over[5]))]
    st, frames, ur, dp = device_batch(hs, cases, cap, extra)
    assert st == ORBFE_OK
    for f, (c, nl, nr) in enumerate(frames):
        m = min(nl, cap)
        o = SC.run_oracle(cut(c, m, min(nr, cap)))
        assert o[0] == ORBFE_OK
        assert same((ORBFE_OK, ur[f, :m], dp[f, :m]), o), (names + ["nl0", "nr0", "over"])[f]
        assert (ur[f, m:] == SENTINEL).all() and (dp[f, m:] == SENTINEL).all(), f


@pytest.mark.gpu
def test_gpu_device_batch(handles):
    """The crafted cases as frames of one call (one call per bf / b and image size), with a
    frame of nl = 0, one of nr = 0 and one whose count exceeds kps_cap; slabs pre-filled with a
    sentinel that must survive at and beyond min(nl, kps_cap)."""
    wide = [n for n in SC.CASES if SC.get(n)[7] == 50.0]
    check_device_batch(handles, wide, 220)                 # the dense cases have nr = 216 or 217
    check_device_batch(handles, [n for n in SC.CASES if SC.get(n)[7] != 50.0], 16)
    for name in SC.TALL:
        check_device_batch(handles, [name], 24)
    check_device_batch(handles, ["key16"], 65535, with_odd_frames=False)


@pytest.mark.gpu
def test_gpu_device_batch_status(handles):
    """One undefined frame in a batch sets the status; the next clean batch resets it."""
    bad = [SC.get("median_n4"), SC.get("left_octave_8"), SC.get("median_n2")]
    assert device_batch(handles, bad, 8)[0] == ORBFE_ERR_UNSUPPORTED
    assert device_batch(handles, [SC.get("median_n4")], 8)[0] == ORBFE_OK
    for name in ("right_band_above", "left_row_negative_matched", "right_strip_left"):
        assert device_batch(handles, [SC.get(name)], 8)[0] == ORBFE_ERR_UNSUPPORTED, name
    check_device_batch(handles, ["median_n4", "ok_left_row_negative_empty"], 8)
