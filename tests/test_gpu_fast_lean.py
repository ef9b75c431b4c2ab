"""fast_kernel's leaner instruction stream (orbfe_extract.hip K2; profiles/fast_issue): the
pre-test's lane layout comes from a per-plan table keyed by (x0 & 3, candidate columns), the
sweep address advances by a uniform step, list entries are LDS addresses and the ROI rows are
staged by chunk count.  None of that may show: the per-level FAST lists (order included), the
keypoints' 28 bytes and the descriptors stay the oracle's (ORBextractor.cc:764-831).

The inputs are chosen so that every path runs; the tests without the gpu mark prove that from
the oracle pyramid alone, with the kernel's arithmetic written out in numpy (cells, groups per
row, rows per sweep, the pre-test, the flush rule).  ORBFE_FAST_LIST_CAP=322
lowers the list to its minimum so that small frames flush."""
import math

import numpy as np
import pytest

import oracle
from orbslam_mapsave_amd.synth import synthetic_frame

LIST_CAP = 512   # kFastListCap
LOW_CAP = 322    # the smallest list a flush still makes progress with
FAST_PITCH = 48  # kFastPitch: the compile-time ROI pitch of fast_kernel<48>


def noise_frame(seed, w, h):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def checker_frame(w, h, period):
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x // period) + (y // period)) % 2 == 0, 40, 215).astype(np.uint8)


def ramped(img):
    """The frame with its contrast about 128 rising as x^4 from none at the left edge: cells
    that keep few pre-test survivors beside cells that keep nearly all."""
    w = img.shape[1]
    x = np.arange(w, dtype=np.int64)[None, :]
    return (128 + (img.astype(np.int64) - 128) * x ** 4 // w ** 4).astype(np.uint8)


def frame(kind, seed, w, h):
    if kind.endswith("_ramp"):
        return ramped(frame(kind[:-5], seed, w, h))
    if kind == "noise":
        return noise_frame(seed, w, h)
    if kind.startswith("checker"):
        return checker_frame(w, h, int(kind[-1]))
    return synthetic_frame(seed, w, h)


# ---- the plan's arithmetic (plan_levels, plan_fast, fast_shape) ---------------------------------

def cells_of(lw, lh):
    """FAST cells (y0, y1, x0, x1) of an lw x lh level (ORBextractor.cc:772-806)."""
    maxx, maxy = lw - 16, lh - 16
    width, height = maxx - 16, maxy - 16
    ncols, nrows = width // 30, height // 30
    out = []
    if ncols <= 0 or nrows <= 0:
        return out
    wc, hc = math.ceil(width / ncols), math.ceil(height / nrows)
    for i in range(nrows):
        y0 = 16 + i * hc
        if y0 >= maxy - 3:
            continue
        y1 = min(y0 + hc + 6, maxy)
        for j in range(ncols):
            x0 = 16 + j * wc
            if x0 >= maxx - 6:
                continue
            out.append((y0, y1, x0, min(x0 + wc + 6, maxx)))
    return out


def plan_of(p, w, h, cap=LIST_CAP):
    """(cells per level, ROI pitch, cand_max) of a w x h input."""
    per_level = [cells_of(int(lw), int(lh)) for lw, lh in zip(*oracle.level_sizes(p, w, h))]
    allc = [c for lv in per_level for c in lv]
    rmax = max([7] + [c[1] - c[0] for c in allc])
    cmax = max([7] + [c[3] - c[2] for c in allc])
    return per_level, (cmax + 3 + 15) & ~15, min((rmax - 6) * (cmax - 6), cap)


def layout(x0, nc):
    """(groups per row, rows per sweep) of a cell's pre-test."""
    X0 = (x0 & 3) + 3
    gpr = ((X0 + nc - 1) >> 2) - (X0 >> 2) + 1
    return gpr, 64 // gpr


def pretest(roi, t):
    """The pre-test's survivors among the candidates of a ROI: two opposite pairs of the four
    cardinal circle points each hold a point brighter than v + t, or each a point darker."""
    a = roi.astype(np.int16)
    v = a[3:-3, 3:-3]
    up, dn, lf, rt = a[:-6, 3:-3], a[6:, 3:-3], a[3:-3, :-6], a[3:-3, 6:]
    br = ((dn > v + t) | (up > v + t)) & ((rt > v + t) | (lf > v + t))
    dk = ((dn < v - t) | (up < v - t)) & ((rt < v - t) | (lf < v - t))
    return br | dk


def cell_model(roi, x0, t, cand_max):
    """One pass of fast_kernel over a cell: (flushes, survivors, the closest a sweep's test
    cnt + rps * nc > cand_max came to its boundary)."""
    nr, nc = roi.shape[0] - 6, roi.shape[1] - 6
    if nr <= 0 or nc <= 0:
        return 0, 0, None
    rows = pretest(roi, t).sum(axis=1)
    _, rps = layout(x0, nc)
    cnt = flushes = 0
    near = None
    for r0 in range(0, nr, rps):
        add = int(rows[r0:r0 + rps].sum())
        d = cnt + rps * nc - cand_max
        if near is None or abs(d) < abs(near):
            near = d
        if d > 0:
            flushes += 1
            cnt = int(rows[r0 - 1])
        cnt += add
    return flushes, int(rows.sum()), near


def frame_model(p, img, ini, mn, cap):
    """Per cell of every level: dict(level, flush0, surv0, near0, rerun, flush1, surv1)."""
    out = []
    levels = [np.asarray(l) for l in oracle.pyramid(p, img)]
    per_level, _, cand_max = plan_of(p, img.shape[1], img.shape[0], cap)
    for lv, (plane, cells) in enumerate(zip(levels, per_level)):
        for (y0, y1, x0, x1) in cells:
            roi = np.ascontiguousarray(plane[y0:y1, x0:x1])
            f0, s0, n0 = cell_model(roi, x0, ini, cand_max)
            d = dict(level=lv, flush0=f0, surv0=s0, near0=n0, rerun=False, flush1=0, surv1=0)
            if roi.shape[0] > 6 and roi.shape[1] > 6 and len(oracle.fast(roi, ini)) == 0:
                d["rerun"] = True
                d["flush1"], d["surv1"], _ = cell_model(roi, x0, mn, cand_max)
            out.append(d)
    return out


# ---- the comparison every GPU case makes --------------------------------------------------------

def check_frame(ex, p, img, kps, desc, frame_index=0):
    okps, odesc = oracle.extract(p, img)
    for lv, plane in enumerate(oracle.pyramid(p, img)):
        assert np.array_equal(ex.get_fast_keys(lv, frame_index), oracle.fast_keys(p, plane)), lv
    assert len(kps) == len(okps)
    assert kps.tobytes() == okps.tobytes()
    assert np.array_equal(desc, odesc)


def run_single(img, ini, mn, levels=8, scale=1.2):
    from orbslam_mapsave_amd.native import ORBextractor
    h, w = img.shape
    p = oracle.params(1000, scale, levels, ini, mn)
    ex = ORBextractor(1000, scale, levels, ini, mn, device=0, max_width=w, max_height=h)
    try:
        kps, desc = ex(img)
        check_frame(ex, p, img, kps, desc)
    finally:
        ex.close()


# ---- 1. all four phases and both cell widths ----------------------------------------------------

# 1000 x 120: level 0's last cell has one candidate column (one group per row)
PHASE_SIZES = [(331, 247), (96, 80), (853, 481), (1000, 120), (700, 500)]


def test_phase_sizes_cover_the_layouts():
    p = oracle.params(1000, 1.2, 8, 20, 7)
    phases, narrow, one_group = set(), 0, 0
    for w, h in PHASE_SIZES:
        per_level, _, _ = plan_of(p, w, h)
        here = set()
        for cells in per_level:
            widths = [c[3] - c[2] for c in cells]
            here |= {c[2] & 3 for c in cells}
            narrow += any(wd < max(widths) for wd in widths)
            one_group += sum(1 for c in cells if 1 <= c[3] - c[2] - 6 <= 4 and layout(c[2], c[3] - c[2] - 6)[0] == 1)
        phases |= here
    assert phases == {0, 1, 2, 3}
    assert narrow >= len(PHASE_SIZES)  # a level with a narrower last cell per frame, on average
    assert one_group > 0
    per_level, _, _ = plan_of(p, 331, 247)
    assert {c[2] & 3 for cells in per_level for c in cells} == {0, 1, 2, 3}  # in one frame


@pytest.mark.gpu
@pytest.mark.parametrize("size", PHASE_SIZES)
def test_phases_and_cell_widths(size):
    run_single(synthetic_frame(21, *size), 20, 7)


# ---- 2. lane-table seams ------------------------------------------------------------------------

@pytest.mark.gpu
def test_batch_of_nine():
    from orbslam_mapsave_amd.native import ORBextractor
    w, h = 331, 247
    p = oracle.params(1000, 1.2, 8, 20, 7)
    imgs = np.stack([synthetic_frame(50 + s, w, h) for s in range(9)])
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_width=w, max_height=h)
    try:
        kps, desc, cnt = ex.extract_batch(imgs)
        for f in range(9):
            check_frame(ex, p, imgs[f], kps[f, :cnt[f]], desc[f, :cnt[f]], f)
    finally:
        ex.close()


@pytest.mark.gpu
def test_two_plans_alive():
    """Two handles of different sizes, used alternately: the tables are per plan."""
    from orbslam_mapsave_amd.native import ORBextractor
    p = oracle.params(1000, 1.2, 8, 20, 7)
    sizes = [(331, 247), (700, 500)]
    exs = [ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_width=w, max_height=h) for w, h in sizes]
    try:
        for rnd in range(2):
            for ex, (w, h) in zip(exs, sizes):
                img = synthetic_frame(60 + rnd, w, h)
                kps, desc = ex(img)
                check_frame(ex, p, img, kps, desc)
    finally:
        for ex in exs:
            ex.close()


def test_both_instantiations_run():
    """Which fast_kernel each size of this file takes: a cell wider than 45 px anywhere in the
    pyramid makes the plan's ROI pitch 64, the runtime-pitch instantiation <0>; 1280 x 720 at
    scale 1.5 / 4 levels has none and takes <48> like the bench sizes."""
    p = oracle.params(1000, 1.2, 8, 20, 7)
    pitch = {s: plan_of(p, *s)[1] for s in PHASE_SIZES + [(160, 120), (640, 480)]}
    assert plan_of(oracle.params(1000, 1.5, 4, 20, 7), 1280, 720)[1] == FAST_PITCH
    for s in [(853, 481), (700, 500), (1000, 120), (640, 480)]:
        assert pitch[s] == FAST_PITCH, s
    for s in [(331, 247), (96, 80), (160, 120)]:
        assert pitch[s] == 64, s


@pytest.mark.gpu
def test_1280x720_scale_1_5():
    run_single(synthetic_frame(22, 1280, 720), 20, 7, levels=4, scale=1.5)


# ---- 3. flush boundary, dense -------------------------------------------------------------------

# (kind, seed, w, h, ini, min); the seeds were searched on the CPU for a sweep whose flush
# test cnt + rps * nc > cand_max lands on its boundary or one beside it
# (test_dense_inputs_reach_the_boundary).  At 160 x 120 and 322 entries every cell of a plain
# textured or noise frame flushes, so those four take the contrast ramp: some cells then stay
# below the list's capacity.
DENSE = [("textured_ramp", 0, 160, 120, 20, 7), ("textured_ramp", 0, 160, 120, 5, 3),
         ("noise_ramp", 3, 160, 120, 20, 7), ("noise_ramp", 0, 160, 120, 5, 3),
         ("textured", 0, 640, 480, 1, 1)]


@pytest.mark.parametrize("case", DENSE)
def test_dense_inputs_reach_the_boundary(case):
    kind, seed, w, h, ini, mn = case
    p = oracle.params(1000, 1.2, 8, ini, mn)
    m = frame_model(p, frame(kind, seed, w, h), ini, mn, LOW_CAP)
    assert any(c["flush0"] or c["flush1"] for c in m)
    assert any(not c["flush0"] and not c["flush1"] and c["surv0"] for c in m)
    assert any(c["near0"] is not None and abs(c["near0"]) <= 1 for c in m)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DENSE)
def test_dense_flushes(case, monkeypatch):
    kind, seed, w, h, ini, mn = case
    monkeypatch.setenv("ORBFE_FAST_LIST_CAP", str(LOW_CAP))
    run_single(frame(kind, seed, w, h), ini, mn)


# ---- 4. flush, nothing emitted, rerun -----------------------------------------------------------

def test_checker_flushes_then_reruns():
    p = oracle.params(1000, 1.2, 8, 7, 3)
    m = frame_model(p, checker_frame(640, 480, 2), 7, 3, LOW_CAP)
    assert any(c["flush0"] and c["rerun"] for c in m)           # flushes, emits nothing, reruns
    assert any(c["rerun"] and not c["flush1"] and c["surv1"] for c in m)  # a rerun without a flush


@pytest.mark.gpu
def test_flush_then_rerun(monkeypatch):
    monkeypatch.setenv("ORBFE_FAST_LIST_CAP", str(LOW_CAP))
    run_single(checker_frame(640, 480, 2), 7, 3)


# ---- 5. chunk edges of the score and emission loops of a pass without a flush -------------------

# survivors in one cell -> (seed, iniThFAST), searched on the CPU (at 20 these small frames keep
# more than half their candidates)
CHUNK_SEEDS = {64: (32, 100), 128: (75, 80)}


def noflush_counts(seed, ini):
    p = oracle.params(1000, 1.2, 8, ini, 7)
    m = frame_model(p, synthetic_frame(seed, 96, 80), ini, 7, LIST_CAP)
    return [c["surv0"] for c in m if not c["flush0"]] + [c["surv1"] for c in m if c["rerun"] and not c["flush1"]]


@pytest.mark.parametrize("n", sorted(CHUNK_SEEDS))
def test_seeds_hit_the_chunk_edges(n):
    counts = noflush_counts(*CHUNK_SEEDS[n])
    assert n in counts
    assert any(c % 64 for c in counts)  # and a partial last chunk


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(CHUNK_SEEDS))
def test_chunk_edges(n):
    seed, ini = CHUNK_SEEDS[n]
    run_single(synthetic_frame(seed, 96, 80), ini, 7)
