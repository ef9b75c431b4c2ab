"""The order-dependent matchers at ties, degenerate sizes and seams (greedy_cases.py).

CPU: the C oracle against the independent restatements on every existing scenario and on every
adversarial case; the adversarial cases reach every tie / quirk branch at least five times
(counted by the restatements); every single-decision mutant of a restatement changes the answer
on at least one adversarial case, so a kernel with that slip would fail the GPU tests below.
GPU: every adversarial case, and degenerate sizes of them, through every form the library has,
bit-exact against the oracle.

Branch counts over the adversarial cases (restatements, check_ori on), floor 5 each:
  SearchForInitialization (617 matches): steal 72, steal_refused_equal 649, stolen_in_hist 72,
    first_wins_tie 52 (needs nnratio > 1: with nnratio <= 1 an exact tie of the two best fails
    the ratio test, so the matcher does not depend on the candidate order; two cases run at
    nnratio 1.25), best_eq_th 113, ratio_equal_reject 56, bin_half 90, bin_wrap 259, maxima_tie 10, maxima_tenth_edge 7.
  SearchByProjection local map (815): overwrite_nobs0 267, ratio_same_level_reject 223,
    ratio_equal_pass 15, ratio_skipped_levels_differ 231, best_eq_th 92, stereo_edge 25,
    first_wins_tie 62.
  SearchByProjection last frame (943): overwrite_nobs0 385, cleared_by_overwritten_bin 18,
    best_eq_th 133, stereo_edge 37, first_wins_tie 186, bin_half 139, bin_wrap 414,
    maxima_tie 10, maxima_tenth_edge 7.
`bin == HISTO_LENGTH` is unreachable (rot < 360 gives bin <= 12) and has no counter.
"""
import functools

import numpy as np
import pytest

import greedy_cases as G
import oracle
import scenarios as S
from orbslam_mapsave_amd.abi import Frame

F32 = np.float32

# ---- the adversarial cases -----------------------------------------------------------------------

SFI = {"ties0": dict(seed=0), "ties1": dict(seed=1, window=12), "half": dict(seed=2, nnratio=0.5),
       "order": dict(seed=3, nnratio=1.25), "order2": dict(seed=4, nnratio=1.25, window=14)}
SFI.update({f"bins{k}": dict(seed=10 + k, bins=spec) for k, spec in enumerate(G.BIN_SPECS)})
LOCAL = {"mono": dict(seed=0), "stereo": dict(seed=1, stereo=True),
         "th1_half": dict(seed=2, th=1.0, nnratio=0.5),
         "stereo_half": dict(seed=3, stereo=True, th=3.0, nnratio=0.5)}
LAST = {"mono": dict(seed=0), "near": dict(seed=1, motion="near"),
        "forward": dict(seed=2, motion="forward"), "backward": dict(seed=3, motion="backward"),
        "mono7": dict(seed=4, th=7.0)}
LAST.update({f"bins{k}": dict(seed=10 + k, bins=spec) for k, spec in enumerate(G.BIN_SPECS)})
KEYFRAME = {"ties0": dict(seed=0), "ties1": dict(seed=1, th=3.0, orb_dist=100),
            "c16": dict(seed=2, cluster=16), "c17": dict(seed=3, cluster=17),
            "bins0": dict(seed=10, bins=G.BIN_SPECS[0]), "bins2": dict(seed=12, bins=G.BIN_SPECS[2])}


@functools.lru_cache(maxsize=None)
def sfi(name):
    return G.sfi_ties(**SFI[name])


@functools.lru_cache(maxsize=None)
def local(name):
    return G.local_ties(**LOCAL[name])


@functools.lru_cache(maxsize=None)
def last(name):
    return G.last_ties(**LAST[name])


@functools.lru_cache(maxsize=None)
def keyframe(name):
    return G.keyframe_ties(**KEYFRAME[name])


def same(a, b):
    """Tuples of arrays / counts equal, exactly."""
    return len(a) == len(b) and all(
        np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


# oracle and restatement on a case -> comparable tuples
def o_sfi(c, ori=True):
    return oracle.search_for_initialization(c["f1"], c["f2"], c["prev"], c["window"], c["nnratio"], ori)


def r_sfi(c, ori=True, **kw):
    return G.restated_sfi(c["f1"], c["f2"], c["prev"], c["window"], c["nnratio"], ori, **kw)


def o_local(c):
    lm = c["lm"]
    return oracle.search_by_projection_local(c["f"], G.local_mps(c), c["th"], c["nnratio"],
                                             lm["frame_mp"], lm["frame_mp_obs"], lm["ids"])


def r_local(c, **kw):
    lm = c["lm"]
    return G.restated_local(c["f"], G.local_mps(c), c["th"], c["nnratio"], lm["frame_mp"],
                            lm["frame_mp_obs"], lm["ids"], **kw)


def o_last(c, ori=True):
    return oracle.search_by_projection_last(*G.last_args(c), c["th"], c["mono"], ori,
                                            frame_mp=c["frame_mp"], frame_mp_obs=c["frame_mp_obs"],
                                            last_ids=c["last_ids"])


def r_last(c, ori=True, **kw):
    return G.restated_last(c, c["th"], c["mono"], ori, c["frame_mp"], c["frame_mp_obs"], **kw)


def o_keyframe(c, ori=True):
    return oracle.search_by_projection_keyframe(c, c["th"], c["orb_dist"], ori)


# ---- CPU: the oracle pinned by the restatements ---------------------------------------------------

@pytest.mark.parametrize("seed,window,ori", [(0, 100, True), (1, 100, True), (2, 50, False),
                                             (3, 200, True)])
def test_oracle_vs_restated_sfi_scenarios(seed, window, ori):
    f1, f2, prev = S.sfi_case(seed)
    e = oracle.search_for_initialization(f1, f2, prev, window, 0.9, ori)
    assert e[1] > 20
    assert same(G.restated_sfi(f1, f2, prev, window, 0.9, ori), e)


@pytest.mark.parametrize("seed,th,stereo,prior", [(0, 1.0, False, False), (1, 3.0, True, True),
                                                  (2, 5.0, False, True)])
def test_oracle_vs_restated_local_scenarios(seed, th, stereo, prior):
    f, mps, fmp, fobs, ids = S.sbp_local_case(seed, 5000, stereo=stereo, prior=prior)
    e = oracle.search_by_projection_local(f, mps, th, 0.8, fmp, fobs, ids)
    assert e[2] > 100
    assert same(G.restated_local(f, mps, th, 0.8, fmp, fobs, ids), e)


@pytest.mark.parametrize("seed,stereo,mono,th", [(0, False, True, 15.0), (1, False, True, 30.0),
                                                 (2, True, False, 7.0)])
def test_oracle_vs_restated_last_scenarios(seed, stereo, mono, th):
    c = S.sbp_last_case(seed, stereo=stereo)
    e = oracle.search_by_projection_last(*G.last_args(c), th, mono, True, last_ids=c["last_ids"])
    assert e[2] > 100
    assert same(G.restated_last(c, th, mono, True), e)


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("name", list(SFI))
def test_oracle_vs_restated_sfi(name, ori):
    c = sfi(name)
    assert c["f1"].n <= 400 and c["f2"].n <= 400
    assert same(r_sfi(c, ori), o_sfi(c, ori))


@pytest.mark.parametrize("name", list(LOCAL))
def test_oracle_vs_restated_local(name):
    c = local(name)
    assert c["f"].n <= 400 and len(c["lm"]["xyz"]) <= 600
    assert same(r_local(c), o_local(c))


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("name", list(LAST))
def test_oracle_vs_restated_last(name, ori):
    c = last(name)
    assert c["cur"].n <= 400 and len(c["last_keys"]) <= 600
    assert G.last_motion(c, c["mono"]) == {"forward": (True, False), "backward": (False, True)}.get(
        LAST[name].get("motion"), (False, False))
    assert same(r_last(c, ori), o_last(c, ori))


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("name", list(KEYFRAME))
def test_oracle_vs_restated_keyframe(name, ori):
    c = keyframe(name)
    assert c["cur"].n <= 400 and len(c["kf_angle"]) <= 600
    assert same(G.restated_keyframe(c, c["th"], c["orb_dist"], ori), o_keyframe(c, ori))
    if KEYFRAME[name].get("cluster"):   # the last point's window holds exactly 16 / 17 keypoints
        assert G.keyframe_candidates(c, len(c["kf_angle"]) - 1) == KEYFRAME[name]["cluster"]
    else:
        assert max(G.keyframe_candidates(c, i) for i in range(len(c["kf_angle"]))) <= 16


REACH = {
    "sfi": ("steal", "steal_refused_equal", "stolen_in_hist", "first_wins_tie", "best_eq_th",
            "ratio_equal_reject",
            "bin_half", "bin_wrap", "maxima_tie", "maxima_tenth_edge"),
    "local": ("overwrite_nobs0", "ratio_same_level_reject", "ratio_equal_pass",
              "ratio_skipped_levels_differ", "best_eq_th", "stereo_edge", "first_wins_tie"),
    "last": ("overwrite_nobs0", "cleared_by_overwritten_bin", "best_eq_th", "stereo_edge",
             "first_wins_tie", "bin_half", "bin_wrap", "maxima_tie", "maxima_tenth_edge"),
}


@pytest.mark.parametrize("which", list(REACH))
def test_adversarial_cases_reach_every_branch(which):
    """A condition on the inputs: the restatement alone counts the branches it takes."""
    stats = {}
    nm = 0
    if which == "sfi":
        for name in SFI:
            nm += r_sfi(sfi(name), stats=stats)[1]
    elif which == "local":
        for name in LOCAL:
            nm += r_local(local(name), stats=stats)[2]
    else:
        for name in LAST:
            nm += r_last(last(name), stats=stats)[2]
    print(which, "nmatches", nm, {k: stats.get(k, 0) for k in REACH[which]})
    assert nm > 100
    for k in REACH[which]:
        assert stats.get(k, 0) >= 5, (k, stats)


@pytest.mark.parametrize("which,mutant", [("sfi", m) for m in G.SFI_MUTANTS] +
                         [("local", m) for m in G.LOCAL_MUTANTS] +
                         [("last", m) for m in G.LAST_MUTANTS])
def test_every_mutant_changes_an_answer(which, mutant):
    """One flipped decision in the restatement shows on at least one adversarial case: the GPU
    parity tests on these cases would fail for a kernel with that slip."""
    if which == "sfi":
        hit = [n for n in SFI if not same(r_sfi(sfi(n), mutant=mutant), r_sfi(sfi(n)))]
    elif which == "local":
        hit = [n for n in LOCAL if not same(r_local(local(n), mutant=mutant), r_local(local(n)))]
    else:
        hit = [n for n in LAST if not same(r_last(last(n), mutant=mutant), r_last(last(n)))]
    print(which, mutant, hit)
    assert hit


# ---- GPU -----------------------------------------------------------------------------------------

def matcher(nnratio, ori):
    from orbslam_mapsave_amd.native import ORBmatcher
    return ORBmatcher(nnratio, ori, device=0)


def g_sfi(m, c):
    m.mfNNratio = float(c["nnratio"])
    return m.SearchForInitialization(c["f1"], c["f2"], c["prev"], c["window"])


def g_local(m, c):
    lm = c["lm"]
    m.mfNNratio = float(c["nnratio"])
    return m.SearchByProjection(c["f"], G.local_mps(c), c["th"], lm["frame_mp"],
                                lm["frame_mp_obs"], lm["ids"])


def g_last(m, c):
    return m.SearchByProjectionLast(*G.last_args(c), c["th"], c["mono"], frame_mp=c["frame_mp"],
                                    frame_mp_obs=c["frame_mp_obs"], last_ids=c["last_ids"])


def g_keyframe(m, c):
    return m.SearchByProjectionKeyFrame(
        c["cur"], c["tcw_cur"], c["cam"], c["log_scale"], c["kf_angle"], c["kf_valid"], c["kf_bad"],
        c["found"], c["kf_xyz"], c["kf_desc"], c["kf_min"], c["kf_max"], c["th"], c["orb_dist"],
        frame_mp=c["frame_mp"], kf_ids=c["kf_ids"])


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _i32(t, n):
    return t.cpu().numpy().view(np.int32)[:n].copy()


def g_local_device(m, c):
    """orbfe_search_by_projection_local_device on device copies of the isInFrustum outputs."""
    import torch
    f, lm, mps = c["f"], c["lm"], G.local_mps(c)
    D = {k: _up(v) for k, v in dict(
        inv=mps.track_in_view, bad=mps.is_bad, px=mps.proj_x, py=mps.proj_y, pxr=mps.proj_xr,
        pl=mps.pred_level, vc=mps.view_cos, desc=mps.desc, nobs=mps.n_obs, ids=lm["ids"],
        fmp=lm["frame_mp"], fobs=lm["frame_mp_obs"], keys=f.keys, kd=f.desc).items()}
    d_ur = _up(f.u_right) if f.u_right is not None else None
    torch.cuda.synchronize()
    nm = m.search_by_projection_local_device(
        f.n, _ptr(D["keys"]), _ptr(D["kd"]), _ptr(d_ur), S.W, S.H, f.scale_factors, mps.m,
        _ptr(D["inv"]), _ptr(D["bad"]), _ptr(D["px"]), _ptr(D["py"]), _ptr(D["pxr"]), _ptr(D["pl"]),
        _ptr(D["vc"]), _ptr(D["desc"]), _ptr(D["nobs"]), _ptr(D["ids"]), c["nnratio"], c["th"],
        _ptr(D["fmp"]), _ptr(D["fobs"]))
    return _i32(D["fmp"], f.n), _i32(D["fobs"], f.n), nm


def g_local_points(m, c):
    """orbfe_search_local_points_device on device copies of the frame and the local map ->
    ((frame_mp, frame_mp_obs, nmatches), mbTrackInView, nToMatch)."""
    import torch
    f, lm = c["f"], c["lm"]
    n_mp = len(lm["xyz"])
    T = {k: _up(v) for k, v in lm.items() if k != "tcw"}
    d_keys, d_desc = _up(f.keys), _up(f.desc)
    d_ur = _up(f.u_right) if f.u_right is not None else None
    d_inv = torch.zeros(max(n_mp, 1), dtype=torch.uint8, device=d_keys.device)
    torch.cuda.synchronize()
    nm, nto = m.search_local_points_device(
        f.n, _ptr(d_keys), _ptr(d_desc), _ptr(d_ur), S.W, S.H, f.scale_factors, lm["tcw"], c["cam"],
        G.LOG_SCALE, 0.5, n_mp, _ptr(T["xyz"]), _ptr(T["normal"]), _ptr(T["min_dist"]),
        _ptr(T["max_dist"]), _ptr(T["desc"]), _ptr(T["nobs"]), _ptr(T["bad"]), _ptr(T["skip"]),
        _ptr(T["ids"]), c["nnratio"], c["th"], _ptr(T["frame_mp"]), _ptr(T["frame_mp_obs"]),
        d_inv.data_ptr())
    return ((_i32(T["frame_mp"], f.n), _i32(T["frame_mp_obs"], f.n), nm),
            d_inv.cpu().numpy()[:n_mp], nto)


def check_local_points(m, c):
    got, inv, nto = g_local_points(m, c)
    mps = G.local_mps(c)
    assert same(got, o_local(c))
    assert np.array_equal(inv, mps.track_in_view) and nto == int(mps.track_in_view.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [True, False])
def test_gpu_sfi_adversarial(ori):
    """Every case on one matcher, consecutively (state carried between calls)."""
    m = matcher(0.9, ori)
    try:
        for name in SFI:
            assert same(g_sfi(m, sfi(name)), o_sfi(sfi(name), ori)), name
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_local_adversarial_host():
    m = matcher(0.8, True)
    try:
        for name in LOCAL:
            assert same(g_local(m, local(name)), o_local(local(name))), name
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "csr"])
def test_gpu_local_adversarial_device(path, monkeypatch):
    if path == "csr":
        monkeypatch.setenv("ORBFE_SBP_DEVICE_CSR", "1")
    else:
        monkeypatch.delenv("ORBFE_SBP_DEVICE_CSR", raising=False)
    m = matcher(0.8, False)
    try:
        for name in LOCAL:
            assert same(g_local_device(m, local(name)), o_local(local(name))), name
        if path == "fused":
            assert m.capacity_retries() == 0   # every case stayed in the 16 fixed slots
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_local_adversarial_local_points():
    m = matcher(0.8, False)
    try:
        for name in LOCAL:
            check_local_points(m, local(name))
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [True, False])
def test_gpu_last_adversarial(ori):
    m = matcher(0.9, ori)
    try:
        for name in LAST:
            assert same(g_last(m, last(name)), o_last(last(name), ori)), name
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [True, False])
def test_gpu_keyframe_adversarial(ori):
    """th = 3 keeps every point within the 16 fixed candidate slots; one point with exactly 16
    candidates stays there, one with 17 sends the call to the CSR path."""
    m = matcher(0.9, ori)
    try:
        for name in KEYFRAME:
            before = m.capacity_retries()
            assert same(g_keyframe(m, keyframe(name)), o_keyframe(keyframe(name), ori)), name
            assert m.capacity_retries() - before == (1 if name == "c17" else 0), name
    finally:
        m.close()


# Degenerate sizes: the reference loops over empty vectors without complaint, include/orbfe.h
# documents no refusal for them, so every one returns the oracle's answer.
SEAMS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257)


def sfi_degenerate():
    c = sfi("ties0")
    out = {f"n1={n}": G.sfi_prefix(c, n1=n) for n in SEAMS}
    out.update({f"n2={n}": G.sfi_prefix(c, n2=n) for n in (0, 1)})
    out["both0"] = G.sfi_prefix(c, n1=0, n2=0)
    k = c["f1"].keys.copy()
    k["octave"] = 1                                         # every F1 keypoint filtered out
    out["all_filtered"] = dict(c, f1=Frame(k, c["f1"].desc, S.W, S.H, G.SCALE))
    out["no_candidate"] = dict(c, prev=c["prev"] + F32(2000.0))
    return out


def local_degenerate():
    c = local("stereo")
    out = {f"m={n}": G.local_prefix(c, m=n) for n in SEAMS}
    out.update({f"n={n}": G.local_prefix(c, n=n) for n in (0, 1)})
    out["both0"] = G.local_prefix(c, m=0, n=0)
    lm = c["lm"]
    out["all_bad"] = dict(c, lm=dict(lm, bad=np.ones_like(lm["bad"])))
    out["all_skipped"] = dict(c, lm=dict(lm, skip=np.ones_like(lm["skip"])))
    out["all_behind"] = dict(c, lm=dict(lm, xyz=lm["xyz"] * F32(-1.0)))
    out["all_outside"] = dict(c, lm=dict(lm, xyz=lm["xyz"] + np.array([50, 0, 0], F32)))
    k = c["f"].keys.copy()
    k["octave"] = 7                                         # no keypoint in any point's levels
    out["no_candidate"] = dict(c, f=Frame(k, c["f"].desc, S.W, S.H, G.SCALE, c["f"].u_right))
    return out


def last_degenerate():
    c = last("near")
    out = {f"m={n}": G.last_prefix(c, m=n) for n in SEAMS}
    out.update({f"n={n}": G.last_prefix(c, n=n) for n in (0, 1)})
    out["both0"] = G.last_prefix(c, m=0, n=0)
    out["all_invalid"] = dict(c, last_valid=np.zeros_like(c["last_valid"]))
    out["all_outlier"] = dict(c, last_outlier=np.ones_like(c["last_outlier"]))
    out["all_behind"] = dict(c, last_xyz=c["last_xyz"] * F32(-1.0))
    out["all_outside"] = dict(c, last_xyz=c["last_xyz"] + np.array([50, 0, 0], F32))
    k = c["cur"].keys.copy()
    k["octave"] = 7
    out["no_candidate"] = dict(c, cur=Frame(k, c["cur"].desc, S.W, S.H, G.SCALE, c["cur"].u_right))
    return out


def keyframe_degenerate():
    c = keyframe("ties0")
    out = {f"m={n}": G.keyframe_prefix(c, m=n) for n in SEAMS}
    out.update({f"n={n}": G.keyframe_prefix(c, n=n) for n in (0, 1)})
    out["both0"] = G.keyframe_prefix(c, m=0, n=0)
    out["all_invalid"] = dict(c, kf_valid=np.zeros_like(c["kf_valid"]))
    out["all_bad"] = dict(c, kf_bad=np.ones_like(c["kf_bad"]))
    out["all_found"] = dict(c, found=np.ones_like(c["found"]))
    out["all_outside"] = dict(c, kf_xyz=c["kf_xyz"] + np.array([50, 0, 0], F32))
    k = c["cur"].keys.copy()
    k["octave"] = 7
    out["no_candidate"] = dict(c, cur=Frame(k, c["cur"].desc, S.W, S.H, G.SCALE))
    return out


def empty(name):
    return name in ("m=0", "n=0", "both0") or name.startswith(("all_", "no_"))


def test_degenerate_cases_oracle_vs_restated():
    """The oracle's answers for the degenerate sizes are the restatements' too; the filtered
    cases match nothing, the seam prefixes something."""
    for name, c in sfi_degenerate().items():
        e = o_sfi(c)
        assert same(r_sfi(c), e), name
        assert e[1] == 0 if name in ("n1=0", "n2=0", "both0", "all_filtered", "no_candidate") \
            else e[1] > 0 or name in ("n1=1", "n2=1"), name
    for name, c in local_degenerate().items():
        e = o_local(c)
        assert same(r_local(c), e), name
        assert e[2] == 0 if empty(name) else e[2] > 0 or name in ("m=1", "n=1"), name
    for name, c in last_degenerate().items():
        e = o_last(c)
        assert same(r_last(c), e), name
        assert e[2] == 0 if empty(name) else e[2] > 0 or name in ("m=1", "n=1"), name
    for name, c in keyframe_degenerate().items():
        e = o_keyframe(c)
        assert same(G.restated_keyframe(c, c["th"], c["orb_dist"]), e), name
        assert e[1] == 0 if empty(name) else e[1] > 0 or name in ("m=1", "n=1"), name


@pytest.mark.gpu
def test_gpu_sfi_degenerate():
    m = matcher(0.9, True)
    try:
        for name, c in sfi_degenerate().items():
            assert same(g_sfi(m, c), o_sfi(c)), name
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_local_degenerate_host():
    m = matcher(0.8, True)
    try:
        for name, c in local_degenerate().items():
            assert same(g_local(m, c), o_local(c)), name
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "csr"])
def test_gpu_local_degenerate_device(path, monkeypatch):
    if path == "csr":
        monkeypatch.setenv("ORBFE_SBP_DEVICE_CSR", "1")
    else:
        monkeypatch.delenv("ORBFE_SBP_DEVICE_CSR", raising=False)
    m = matcher(0.8, False)
    try:
        for name, c in local_degenerate().items():
            assert same(g_local_device(m, c), o_local(c)), name
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_local_degenerate_local_points():
    m = matcher(0.8, False)
    try:
        for name, c in local_degenerate().items():
            check_local_points(m, c)
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_last_degenerate():
    m = matcher(0.9, True)
    try:
        for name, c in last_degenerate().items():
            assert same(g_last(m, c), o_last(c)), name
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_keyframe_degenerate():
    m = matcher(0.9, True)
    try:
        for name, c in keyframe_degenerate().items():
            assert same(g_keyframe(m, c), o_keyframe(c)), name
    finally:
        m.close()
