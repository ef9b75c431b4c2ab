"""The projection matchers' shared host path: the candidate builder (fixed slots, then a bounded
count -> scan -> fill), the one rerun rule, the driver of the three host forms and the CSR
fallback of the two device forms.

The case is built by hand: 200 keypoints on a 0.5 px lattice (10 x 5 px, octave 1) under two or
three query points, every one of which sees the whole cluster at its levels.  So every point has
more candidates than any form's fixed slots (16, or 64 for the last frame) and more than the 64
per point a bounded fill starts with; the CPU checks below count them with the restatement's
GetFeaturesInArea, so that no GPU test can pass by not overflowing.  Descriptor distances are
5 + 3 j to the lattice's first 25 keypoints and 80 .. 84 to the rest, all within TH_HIGH.

Rerun counts on a fresh matcher, host forms: the fixed slots overflow (1), the bounded fill of
max(64 * 2, the slots' buffer) = 128 entries is short of the 400 candidates (2), the fill at the
reported total fits.  The same call again: the slots overflow (1) and the grown buffer fits.
Device forms, 3 points and a frame past the fused path's 2048 keypoints: 16 * 3 = 48 < 600 (1).
"""
import functools

import numpy as np
import pytest

import greedy_cases as G
import test_greedy_edges as E

F32 = np.float32
CLUSTER, FORMS = 200, ("local", "last", "keyframe")


def _builder(nq, fillers=0):
    b = G.Builder(9000)
    for j in range(CLUSTER):
        b.add_kp(315.0 + 0.5 * (j % 20), 237.5 + 0.5 * (j // 20), 1, 30.0, 0,
                 3 * j if j < 25 else 75 + j % 5, j)
        b.kp[-1]["tag"] = j
    for j in range(fillers):       # far from every query's window, at a level none of them reads
        b.add_kp(20.0 + 10.0 * (j % 60), 330.0 + 4.0 * (j // 60), 5, 0.0, 1, j % 50, j)
        b.kp[-1]["tag"] = -1
    for i in range(nq):
        b.add_q(320.0 + 0.25 * i, 240.0, 1, 30.0, 0, 5, i, 1)
    return b


def _prior(b):
    """Slots taken before the call: the best keypoint held by a point with observations (it
    blocks), the second best by one without (it is overwritten), the third blocked again, and a
    held slot that no point ends on."""
    at = {p["tag"]: i for i, p in enumerate(b.kp)}
    fmp = np.full(len(b.kp), -1, np.int32)
    fobs = np.zeros(len(b.kp), np.int32)
    for tag, obs in ((0, 1), (1, 0), (2, 2), (30, 0)):
        fmp[at[tag]], fobs[at[tag]] = 7000 + tag, obs
    return fmp, fobs


@functools.lru_cache(maxsize=None)
def cluster(form, nq=2, fillers=0):
    b = _builder(nq, fillers)
    if form == "local":
        c = G.local_ties(0, th=2.0, nnratio=0.9, b=b)
        c["lm"]["frame_mp"], c["lm"]["frame_mp_obs"] = _prior(b)
    elif form == "last":
        c = G.last_ties(0, b=b)
        c["frame_mp"], c["frame_mp_obs"] = _prior(b)
    else:
        c = G.keyframe_ties(0, th=6.0, orb_dist=100, b=b)
        c["frame_mp"] = _prior(b)[0]
    return c


def candidates(form, c):
    """Candidates per query point at its accepted levels (the restatement's GetFeaturesInArea)."""
    if form == "keyframe":
        return [G.keyframe_candidates(c, i) for i in range(len(c["kf_angle"]))]
    if form == "last":
        grid, out = G.Grid(c["cur"]), []
        for i in range(len(c["last_keys"])):
            _, u, v, _ = G.last_project(c, i)
            o = int(c["last_keys"]["octave"][i])
            out.append(len(grid.area(u, v, F32(c["th"]) * G.SCALE[o], o - 1, o + 1)))
        return out
    mps, grid, out = G.local_mps(c), G.Grid(c["f"]), []
    for i in range(mps.m):
        r = F32(2.5) if float(mps.view_cos[i]) > 0.998 else F32(4.0)
        pl = int(mps.pred_level[i])
        assert mps.track_in_view[i]
        out.append(len(grid.area(mps.proj_x[i], mps.proj_y[i], r * F32(c["th"]) * G.SCALE[pl], pl - 1, pl)))
    return out


ORACLE = {"local": lambda c: E.o_local(c), "last": lambda c: E.o_last(c, True),
          "keyframe": lambda c: E.o_keyframe(c, True)}
GPU = {"local": E.g_local, "last": E.g_last, "keyframe": E.g_keyframe}


@pytest.mark.parametrize("form", FORMS)
def test_cluster_overflows_every_bound(form):
    """CPU: every point has more than 64 candidates, the oracle agrees with the restatement, and
    its answer depends on the slots held before the call."""
    c = cluster(form)
    assert min(candidates(form, c)) > 64, candidates(form, c)
    e = ORACLE[form](c)
    if form == "local":
        assert E.same(E.r_local(c), e)
        free = dict(c, lm=dict(c["lm"], frame_mp=np.full_like(c["lm"]["frame_mp"], -1)))
    elif form == "last":
        assert E.same(E.r_last(c), e)
        free = dict(c, frame_mp=np.full_like(c["frame_mp"], -1))
    else:
        assert E.same(G.restated_keyframe(c, c["th"], c["orb_dist"]), e)
        free = dict(c, frame_mp=np.full_like(c["frame_mp"], -1))
    assert e[-1] == 2                                   # both points matched
    assert not np.array_equal(ORACLE[form](free)[0], e[0])


def test_device_cluster_overflows_the_bounded_fill():
    c = cluster("local", 3, 1900)
    assert c["f"].n > 2048 and sum(candidates("local", c)) > 16 * 3
    e = E.o_local(c)
    assert E.same(E.r_local(c), e) and e[2] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_double_overflow(form):
    """Fixed slots, then the 64-per-point bound, then the exact total; the slots held before the
    call survive the two failed attempts (the oracle's answer on the original input)."""
    c, e = cluster(form), ORACLE[form](cluster(form))
    m = E.matcher(0.9, True)
    try:
        assert E.same(GPU[form](m, c), e)
        assert m.capacity_retries() == 2
        assert E.same(GPU[form](m, c), e)
        assert m.capacity_retries() == 3                # the slots again; the grown buffer fits
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("zero_copy", [None, "0"])
@pytest.mark.parametrize("entry", ["local_points", "by_projection"])
def test_device_forms_bounded_fill_overflows(entry, zero_copy, monkeypatch):
    """The two device entry points' shared CSR path; its result words come back through the
    staging buffer, device-mapped or (ORBFE_ZERO_COPY=0) by DMA."""
    if zero_copy is None:
        monkeypatch.delenv("ORBFE_ZERO_COPY", raising=False)
    else:
        monkeypatch.setenv("ORBFE_ZERO_COPY", zero_copy)
    monkeypatch.delenv("ORBFE_SBP_DEVICE_CSR", raising=False)
    c = cluster("local", 3, 1900)
    m = E.matcher(0.9, False)
    try:
        if entry == "local_points":
            E.check_local_points(m, c)
        else:
            assert E.same(E.g_local_device(m, c), E.o_local(c))
        assert m.capacity_retries() == 1
    finally:
        m.close()


# test_greedy_edges' degenerate sizes run every form at m = 0, m = 1, n = 0, n = 1 and both 0,
# one after another on one matcher that starts with m = 0.  Left for here: a matcher whose FIRST
# call has no keypoint (no scratch buffer exists yet), and one point against one keypoint.
SEAM_CASES = {"n=0": dict(n=0), "m=1,n=1": dict(m=1, n=1), "m=1,n=0": dict(m=1, n=0)}


@pytest.mark.gpu
@pytest.mark.parametrize("seam", list(SEAM_CASES))
@pytest.mark.parametrize("form", FORMS)
def test_first_call_at_a_seam(form, seam):
    base = {"local": lambda: E.local("stereo"), "last": lambda: E.last("near"),
            "keyframe": lambda: E.keyframe("ties0")}[form]()
    prefix = {"local": G.local_prefix, "last": G.last_prefix, "keyframe": G.keyframe_prefix}[form]
    c = prefix(base, **SEAM_CASES[seam])
    m = E.matcher(base.get("nnratio", 0.9), True)
    try:
        assert E.same(GPU[form](m, c), ORACLE[form](c))
        assert m.capacity_retries() == 0
    finally:
        m.close()
