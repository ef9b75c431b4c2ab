"""The loop-closing matchers' restatements (tests/loop_cases.py) on the CPU: every single-decision
mutant changes an answer on some built case, every branch counter is reached, the built cases
are non-trivial on the restatement alone, and the C ABI refuses bad arguments without a device.
The GPU parity tests are tests/test_gpu_loop_matchers.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import loop_cases as L
from orbslam_mapsave_amd.abi import ORBFE_ERR_ARG, ORBFE_ERR_UNSUPPORTED, Camera, ptr

SBP_COUNTERS = ("skip", "depth", "image", "distance", "angle", "unsupported", "no_candidates",
                "blocked_preheld", "blocked_dynamic", "level_reject", "tie", "best_at_50",
                "accept", "reject_gt_th", "all_blocked")
SIM3_COUNTERS = ("not_searched", "depth", "image", "distance", "unsupported", "no_candidates",
                 "level_reject", "tie", "best_at_100", "accept", "reject_gt_th", "agree",
                 "disagree")
BOW_COUNTERS = ("node_common", "node_skip1", "node_skip2", "kf1_no_mp", "c2_blocked", "c2_no_mp",
                "best_at_49", "best_at_50", "th_reject", "ratio_reject", "match", "rot_wrap",
                "ori_dropped")


# ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) -------------------------------------

@pytest.fixture(scope="module")
def sbp():
    c = L.sbp_case(0)
    pts = L.sbp_points(c, c["th"])
    st = {}
    matched, n, dec, bad = L.loop_sbp(c, c["th"], stats=st, points=pts)
    assert not bad
    return dict(c=c, pts=pts, st=st, matched=matched, n=n, dec=dec)


def test_sbp_case_is_not_trivial(sbp):
    c, dec = sbp["c"], sbp["dec"]
    assert sbp["n"] >= 40
    ind = L.independent(c, c["th"], points=sbp["pts"])
    assert int((ind != dec).sum()) >= 20
    # the point listed twice can match twice: the skip flags are never updated (309-310)
    ids, cnt = np.unique(c["ids"][dec >= 0], return_counts=True)
    assert (cnt == 2).sum() >= 5
    # points of the list that the keyframe already holds are skipped
    assert int(np.isin(c["ids"], c["matched0"]).sum()) >= 30
    assert (dec[np.isin(c["ids"], c["matched0"])] == -1).all()
    # pre-held slots keep their points
    held = c["matched0"] >= 0
    assert np.array_equal(sbp["matched"][held], c["matched0"][held])
    assert int((sbp["matched"] != c["matched0"]).sum()) == len(set(dec[dec >= 0].tolist()))


def test_sbp_chain():
    """A takes s, B falls to s', C falls to s'' (and on down the list)."""
    c = L.chain_case()
    matched, n, dec, _ = L.loop_sbp(c, c["th"])
    assert dec.tolist() == [0, 1, 2, 3, 4] and n == 5
    assert L.independent(c, c["th"]).tolist() == [0, 0, 1, 2, 3]


@pytest.mark.parametrize("mutant", L.SBP_MUTANTS)
def test_sbp_mutant_changes_an_answer(mutant, sbp):
    c = sbp["c"]
    pts = None if mutant in ("image_le", "no_angle") else sbp["pts"]
    matched, n, dec, _ = L.loop_sbp(c, c["th"], mutant=mutant, points=pts)
    assert not np.array_equal(matched, sbp["matched"]) or n != sbp["n"]


def test_sbp_branch_counters(sbp):
    st = dict(sbp["st"])
    for c in (L.sbp_unsupported_case(0), L.chain_case()):
        r = L.loop_sbp(c, c["th"], stats=st)
    assert r is not None
    missing = {k: st.get(k, 0) for k in SBP_COUNTERS if st.get(k, 0) < 5}
    assert not missing, missing


def test_sbp_unsupported_drops_those_points_only():
    c = L.sbp_unsupported_case(0)
    matched, n, dec, bad = L.loop_sbp(c, c["th"])
    assert bad and (dec[c["hit"]] == -1).all() and n >= 40


# ---- SearchBySim3 ------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[False, True], ids=["same", "mixed"])
def s3(request):
    c = L.sim3_case(0, mixed=request.param)
    st = {}
    res = L.sim3(c, stats=st)
    assert not res[4]
    return dict(c=c, st=st, res=res, mixed=request.param)


def test_sim3_case_is_not_trivial(s3):
    c = s3["c"]
    m12, vn1, vn2, nf, _ = s3["res"]
    assert nf >= 40 and nf == int((m12 >= 0).sum())
    assert int(((vn1 >= 0) & (m12 < 0)).sum()) >= 10         # the agreement rejects them
    am1, am2, s1, s2 = L.masks(c)
    assert am1.sum() == 40 and am2.sum() == 38               # two ids outside [0, N2) (1142)
    assert (vn1[am1] == -1).all() and (vn2[am2] == -1).all()
    assert am2[vn1[vn1 >= 0]].any()                          # no target-side filter
    if s3["mixed"]:
        k1, k2 = c["kf1"], c["kf2"]
        assert (k1.max_x, k1.max_y) != (k2.max_x, k2.max_y)
        assert len(k1.scale_factors) != len(k2.scale_factors) and c["log1"] != c["log2"]


def test_sim3_mats_are_inverse():
    c = L.sim3_case(0)
    S12, S21 = L.sim3_mats(c["s12"], c["R12"], c["t12"])
    A = np.vstack([S12.astype(np.float64), [0, 0, 0, 1]])
    B = np.vstack([S21.astype(np.float64), [0, 0, 0, 1]])
    assert np.allclose(A @ B, np.eye(4), atol=1e-6)
    assert abs(float(c["s12"]) - 1.0) > 0.1


@pytest.fixture(scope="module")
def s3_results():
    return {mixed: L.sim3(L.sim3_case(0, mixed=mixed)) for mixed in (False, True)}


@pytest.mark.parametrize("mutant", L.SIM3_MUTANTS)
def test_sim3_mutant_changes_an_answer(mutant, s3_results):
    changed = False
    for mixed, base in s3_results.items():
        r = L.sim3(L.sim3_case(0, mixed=mixed), mutant=mutant)
        changed |= any(not np.array_equal(a, b) for a, b in zip(r[:3], base[:3]))
    assert changed


def test_sim3_branch_counters():
    st = {}
    for c in (L.sim3_case(0), L.sim3_case(0, mixed=True), L.sim3_unsupported_case(0)):
        L.sim3(c, stats=st)
    missing = {k: st.get(k, 0) for k in SIM3_COUNTERS if st.get(k, 0) < 5}
    assert not missing, missing


def test_sim3_unsupported_drops_those_points_only():
    c = L.sim3_unsupported_case(0)
    m12, vn1, vn2, nf, bad = L.sim3(c)
    assert bad and (vn1[c["hit"]] == -1).all() and nf >= 40


# ---- SearchByBoW(pKF1, pKF2) -------------------------------------------------------------------

@pytest.mark.parametrize("ori", [True, False])
def test_bow_case_is_not_trivial(ori):
    c = L.bow_case(0)
    st = {}
    m12, nm = L.bow_kk(c, 0.75, ori, stats=st)
    assert nm >= 40 and nm == int((m12 >= 0).sum())
    assert st["best_at_49"] >= 1 and st["best_at_50"] >= 1
    hit = m12[m12 >= 0]
    assert len(set(hit.tolist())) == len(hit)                # a partial bijection
    assert c["ok1"][m12 >= 0].all() and c["ok2"][hit].all()
    d = np.array([int(L.hamming(c["desc1"][i], c["desc2"][[j]])[0])
                  for i, j in zip(np.flatnonzero(m12 >= 0), hit)])
    assert d.max() == L.TH_LOW - 1                           # 49 matches, 50 does not


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("mutant", L.BOW_MUTANTS)
def test_bow_mutant_changes_an_answer(mutant, ori):
    c = L.bow_case(0)
    base = L.bow_kk(c, 0.75, ori)
    r = L.bow_kk(c, 0.75, ori, mutant=mutant)
    assert not np.array_equal(r[0], base[0])


def test_bow_branch_counters():
    st = {}
    for ori in (True, False):
        L.bow_kk(L.bow_case(0), 0.75, ori, stats=st)
    missing = {k: st.get(k, 0) for k in BOW_COUNTERS if st.get(k, 0) < 5}
    assert not missing, missing


@pytest.mark.parametrize("ny", [63, 64, 65, 256])
def test_bow_seam_cases_match(ny):
    c = L.bow_seam_case(ny)
    m12, nm = L.bow_kk(c)
    assert nm >= 8 and (m12 == ny - 1).any() and (m12 == 0).any()


# ---- the C ABI refuses bad arguments without a device ------------------------------------------

def _view(kf, nlevels=None):
    v = kf.view()
    if nlevels is not None:
        v.nlevels = nlevels
    return v


def test_null_and_bad_arguments():
    from orbslam_mapsave_amd import native
    lib = native.lib()
    c = L.chain_case()
    kf, cam = c["kf"], c["cam"]
    n = len(c["xyz"])
    km = c["matched0"].copy()
    nm = C.c_int32(0)
    t = np.ascontiguousarray(c["tcw"], np.float32)

    def sbp(view=None, tcw=t, cam_=cam, n_mp=n, xyz=c["xyz"], matched=km, out=nm):
        v = view if view is not None else kf.view()
        return lib.orbfe_search_by_projection_sim3(
            None, C.byref(v) if v else None, ptr(tcw), C.byref(cam_) if cam_ else None,
            C.c_float(c["log_scale"]), n_mp, ptr(xyz), ptr(c["normal"]), ptr(c["min_dist"]),
            ptr(c["max_dist"]), ptr(c["desc"]), None, None, 10, ptr(matched),
            C.byref(out) if out is not None else None)
    assert sbp() == ORBFE_ERR_ARG                           # a NULL matcher
    assert sbp(view=False) == ORBFE_ERR_ARG
    assert sbp(tcw=None) == ORBFE_ERR_ARG
    assert sbp(cam_=None) == ORBFE_ERR_ARG
    assert sbp(n_mp=-1) == ORBFE_ERR_ARG
    assert sbp(xyz=None) == ORBFE_ERR_ARG
    assert sbp(matched=None) == ORBFE_ERR_ARG
    assert sbp(out=None) == ORBFE_ERR_ARG
    assert sbp(view=_view(kf, 0)) == ORBFE_ERR_ARG
    assert sbp(view=_view(kf, 17)) == ORBFE_ERR_UNSUPPORTED  # judged before the handle

    s = L.sim3_subset(L.sim3_case(0), 5, 5)
    S12, S21 = L.sim3_mats(s["s12"], s["R12"], s["t12"])
    m12 = np.zeros(5, np.int32)
    nf = C.c_int32(0)
    p1, p2 = s["pts1"], s["pts2"]
    srch = np.ones(5, np.uint8)

    def sim3(v1=None, v2=None, cam_=s["cam1"], t1w=s["T1w"], s21=S21, xyz1=p1["xyz"],
             desc2=p2["desc"], out=m12, nfound=nf):
        a = v1 if v1 is not None else s["kf1"].view()
        b = v2 if v2 is not None else s["kf2"].view()
        return lib.orbfe_search_by_sim3(
            None, C.byref(a) if a else None, C.byref(b) if b else None,
            C.byref(cam_) if cam_ else None, ptr(t1w), ptr(s["T2w"]), ptr(S12), ptr(s21),
            C.c_float(s["log1"]), C.c_float(s["log2"]), ptr(srch), ptr(xyz1),
            ptr(p1["min_dist"]), ptr(p1["max_dist"]), ptr(p1["desc"]), ptr(srch),
            ptr(p2["xyz"]), ptr(p2["min_dist"]), ptr(p2["max_dist"]), ptr(desc2),
            C.c_float(7.5), ptr(out), None, None, C.byref(nfound) if nfound is not None else None)
    assert sim3() == ORBFE_ERR_ARG                          # a NULL matcher
    assert sim3(v1=False) == ORBFE_ERR_ARG
    assert sim3(v2=False) == ORBFE_ERR_ARG
    assert sim3(cam_=None) == ORBFE_ERR_ARG
    assert sim3(t1w=None) == ORBFE_ERR_ARG
    assert sim3(s21=None) == ORBFE_ERR_ARG
    assert sim3(xyz1=None) == ORBFE_ERR_ARG
    assert sim3(desc2=None) == ORBFE_ERR_ARG
    assert sim3(out=None) == ORBFE_ERR_ARG
    assert sim3(nfound=None) == ORBFE_ERR_ARG
    neg = s["kf1"].view()
    neg.n = -1
    assert sim3(v1=neg) == ORBFE_ERR_ARG
    assert sim3(v1=_view(s["kf1"], 17)) == ORBFE_ERR_UNSUPPORTED
    assert sim3(v2=_view(s["kf2"], 17)) == ORBFE_ERR_UNSUPPORTED

    b = L.bow_seam_case(63)
    d1, a1, ok1, (i1, o1, f1) = L.bow_item(b, 1)
    d2, a2, ok2, (i2, o2, f2) = L.bow_item(b, 2)
    out = np.zeros(len(d1), np.int32)

    def bow(n1=len(d1), n2=len(d2), desc1=d1, ok2_=ok2, feat1=f1, feat2=f2, out_=out, nm_=nm):
        return lib.orbfe_search_by_bow_keyframes(
            None, C.c_float(0.75), 1, n1, ptr(desc1), ptr(a1), ptr(ok1), len(i1), ptr(i1),
            ptr(o1), ptr(feat1), n2, ptr(d2), ptr(a2), ptr(ok2_), len(i2), ptr(i2), ptr(o2),
            ptr(feat2), ptr(out_), C.byref(nm_) if nm_ is not None else None)
    assert bow() == ORBFE_ERR_ARG                           # a NULL matcher
    assert bow(n1=-1) == ORBFE_ERR_ARG
    assert bow(n2=-1) == ORBFE_ERR_ARG
    assert bow(desc1=None) == ORBFE_ERR_ARG
    assert bow(ok2_=None) == ORBFE_ERR_ARG
    assert bow(feat1=None) == ORBFE_ERR_ARG
    assert bow(out_=None) == ORBFE_ERR_ARG
    assert bow(nm_=None) == ORBFE_ERR_ARG
    rep = f2.copy()
    rep[1] = rep[0]                                         # a feature index listed twice
    assert bow(feat2=rep) == ORBFE_ERR_ARG
    assert lib.orbfe_search_by_bow_keyframes_batch_device(
        None, C.c_float(0.75), 1, -1, None, None, 0, None, None, None, None, None, None, None,
        None, None, None) == ORBFE_ERR_ARG
    assert isinstance(cam, Camera)
