"""The projection gates of isInFrustum, SearchByProjection (local map, last frame, keyframe) and
Fuse, at their edges: inputs that sit on every bound (tests/projection_cases.py), compared
bit for bit.

CPU: the restatements against the oracle, every gate mutant visible (or, where no input can
separate two ways of writing a decision, asserted equal), every branch counter reached, and the
builders' claims -- a point on each bound, little filler -- checked from the restatement alone.
GPU: the kernels against the restatements; statuses asserted; a rejected point's outputs left
as they were.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import fuse_cases as FC
import greedy_cases as G
import oracle
import projection_cases as PC
import scenarios as S
import test_sbp_keyframe as K
from orbslam_mapsave_amd.abi import ORBFE_ERR_UNSUPPORTED, MapPoints, OrbfeError

F32 = np.float32
SE3, SIM3 = FC.SE3, FC.SIM3

FRUSTUM_COUNTERS = ("behind", "u_below", "u_above", "v_below", "v_above", "dist_near", "dist_far",
                    "angle", "in_view")
LAST_COUNTERS = ("behind", "outside", "window_forward", "window_backward", "window_both",
                 "stereo_edge")
KEYFRAME_COUNTERS = ("not_searched", "behind_projected", "outside", "distance", "level_outside",
                     "searched")
FUSE_COUNTERS = ("skip", "depth", "image", "distance", "angle", "level_outside", "level_window",
                 "chi2_stereo", "chi2_mono", "chi2")
FRUSTUM_GATES = ("u_max", "u_min", "v_max", "v_min", "dist_min", "dist_max", "vcos", "level")


@functools.lru_cache(maxsize=None)
def frustum_cases():
    return PC.frustum_cases()


@functools.lru_cache(maxsize=None)
def frustum_expected(name):
    st = {}
    return PC.restated_frustum(**frustum_cases()[name].args(), stats=st), st


@functools.lru_cache(maxsize=None)
def scene(name, levels):
    """frustum_scene of a built case; levels == "pyramid": the points that predict a level
    outside the pyramid flagged bad, so that the call succeeds."""
    sc = PC.frustum_scene(frustum_cases()[name])
    if levels == "pyramid":
        inv, _, _, _, pl, _, ok = frustum_expected(name)[0]
        out = (inv > 0) & (~ok | (pl < 0) | (pl >= PC.NLEVELS))
        sc["lm"]["bad"] = np.where(out, 1, sc["lm"]["bad"]).astype(np.uint8)
    return sc


@functools.lru_cache(maxsize=None)
def last_cases():
    return PC.last_cases()


@functools.lru_cache(maxsize=None)
def keyframe_case(name, levels):
    c = PC.keyframe_case(frustum_cases()[name])
    if levels == "pyramid":
        info = {}
        K.restated(c, c["th"], c["orb_dist"], info=info)
        assert info.get("unsupported")
        c["kf_valid"] = _kf_supported(c).astype(np.uint8)
    return c


def _kf_supported(c):
    """Which keyframe points predict a level inside the pyramid (or never get that far)."""
    ok = np.ones(len(c["kf_xyz"]), bool)
    for i in range(len(ok)):
        one = dict(c, kf_valid=np.eye(len(ok), dtype=np.uint8)[i])
        info = {}
        K.restated(one, c["th"], c["orb_dist"], False, info=info)
        ok[i] = not info.get("unsupported")
    return ok


@functools.lru_cache(maxsize=None)
def fuse_cases():
    return {k: v for k, v in PC.fuse_cases().items()}


@functools.lru_cache(maxsize=None)
def fuse_case(name, levels):
    c = fuse_cases()[name].case(skip_every=11)
    if levels == "pyramid":
        ow = FC.camera_center(c["tcw"].astype(F32))
        for i in range(len(c["xyz"])):
            if FC.search_point(c, i, 3.0, SIM3, ow)[2]:
                c["skip"][i] = 1
    return c


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ==== CPU: isInFrustum ===========================================================================

@pytest.mark.parametrize("name", ["identity", "seeded", "depth"])
def test_frustum_restatement_equals_oracle_on_built_cases(name):
    c = frustum_cases()[name]
    assert PC.frustum_equal(oracle.is_in_frustum(**c.args()), frustum_expected(name)[0])


@pytest.mark.parametrize("seed", [0, 1])
def test_frustum_restatement_equals_oracle_on_seeded_case(seed):
    fc = S.frustum_case(seed, 2000)
    exp = PC.restated_frustum(**fc)
    assert exp[6].all() and 100 <= exp[0].sum() <= 1900     # both answers well represented
    assert PC.frustum_equal(oracle.is_in_frustum(**fc), exp)


@pytest.mark.parametrize("mutant", PC.FRUSTUM_MUTANTS)
def test_frustum_mutant_changes_an_output(mutant):
    seen = False
    for name, c in frustum_cases().items():
        got = PC.restated_frustum(**c.args(), mutant=mutant)
        seen |= not PC.frustum_equal(got[:6], frustum_expected(name)[0])
    assert seen


def test_frustum_invz_forms_are_one_function():
    """1.0f / z == (float)(1.0 / (double)z): on the built cases, and over a sweep of z through
    every binade, the ones with a subnormal quotient included."""
    for name, c in frustum_cases().items():
        got = PC.restated_frustum(**c.args(), mutant="invz_double")
        assert PC.frustum_equal(got[:6], frustum_expected(name)[0])
    rng = np.random.Generator(np.random.PCG64(3))
    bits = rng.integers(0, 2 ** 31, 200_000, dtype=np.int64).astype(np.uint32)
    z = np.concatenate([bits.view(F32), (bits | np.uint32(0x7E800000)).view(F32)])
    z = z[np.isfinite(z)]
    with np.errstate(all="ignore"):
        a = (F32(1.0) / z).astype(F32)
        b = (1.0 / z.astype(np.float64)).astype(F32)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (np.abs(a) < 2.0 ** -126).sum() > 1000        # subnormal quotients were among them


def test_frustum_branch_counters():
    tot = {}
    for name in frustum_cases():
        for k, v in frustum_expected(name)[1].items():
            tot[k] = tot.get(k, 0) + v
    assert set(tot) == set(FRUSTUM_COUNTERS)
    assert min(tot.values()) >= 5, tot


@pytest.mark.parametrize("name", ["identity", "seeded"])
def test_frustum_builders_reach_their_gates(name):
    """From the restatement alone: every bisection group crosses its gate between neighbouring
    floats, on the bound where a float hits it; every gate has such a group; at most a tenth of
    the points reach no gate."""
    c = frustum_cases()[name]
    groups = PC.check_groups(c)
    assert set(groups) == set(FRUSTUM_GATES)
    for gate in FRUSTUM_GATES:
        assert groups[gate][0] >= 3, (gate, groups[gate])
    if name == "identity":      # the constructible exact hits: u = 640, viewCos = 0.5f, dist = z
        for gate in ("u_max", "u_min", "v_max", "v_min", "dist_min", "dist_max", "vcos"):
            assert groups[gate][1] >= 1, (gate, groups[gate])
    assert PC.filler(c) * 10 <= len(c.tag)
    lv = frustum_expected(name)[0]
    levels = set(lv[4][lv[0] > 0].tolist())
    assert {0, 1, 7, PC.NLEVELS, PC.NLEVELS + 1} <= levels
    assert name != "identity" or -1 in levels


def test_frustum_depth_edges_are_what_ieee_says():
    """z = +-0 and denormal with x = y = 0: u = 0 * inf + cx is a NaN, every comparison with it
    is false, and the reference returns the point *in view* with NaN projections; x != 0 makes
    u infinite and the point leaves.  -0.0f passes `PcZ < 0.0f`.  dist == 0 with
    mfMinDistance == 0 makes viewCos 0 / 0 and the ratio infinite: the level is not defined."""
    c = frustum_cases()["depth"]
    res = c.results()
    a = c.args()
    assert PC.filler(c) == 0
    nan_in_view = [r for r in res if r["in_view"] and np.isnan(r["u"]) and np.isnan(r["v"])]
    assert len(nan_in_view) >= 8 and all(np.isnan(r["ur"]) for r in nan_in_view)
    negzero = [r for r in res if r["pc"][2] == 0 and np.signbit(r["pc"][2])]
    assert len(negzero) >= 3 and all(r["reject"] != "behind" for r in negzero)
    assert any(r["in_view"] for r in negzero)
    inf_out = [r for r in res if "u" in r and np.isinf(r["u"])]
    assert len(inf_out) >= 8 and all(r["reject"] == "u" for r in inf_out)
    zero_dist = [r for r in res if r["in_view"] and r["dist"] == 0]
    assert len(zero_dist) >= 3 and all(np.isnan(r["vc"]) and not r["lvl_defined"] for r in zero_dist)
    # a NaN centre with a level inside the pyramid: what the searches must survive
    assert any(r["in_view"] and np.isnan(r["u"]) and r["lvl_defined"] and 0 <= r["lvl"] < 8 for r in res)
    assert (a["min_dist"] == 0).all()


# ==== CPU: SearchByProjection, local map =========================================================

def _local_oracle_equal(f, mps, th, nnratio, fmp, fobs, ids, exp):
    o = oracle.search_by_projection_local(f, mps, th, nnratio, fmp, fobs, ids)
    return same(o[:2], exp[:2]) and o[2] == exp[2]


@pytest.mark.parametrize("th", PC.RADIUS_THS)
def test_local_radius_case(th):
    c = PC.radius_case(th)
    st = {}
    exp = G.restated_local(c["f"], c["mps"], c["th"], c["nnratio"], mp_ids=c["ids"], stats=st)
    assert _local_oracle_equal(c["f"], c["mps"], c["th"], c["nnratio"], None, None, c["ids"], exp)
    assert st["radius_2.5"] >= 5 and st["radius_4.0"] >= 5
    # (float)0.998 > 0.998: the boundary value takes 2.5 and misses its keypoint, as its upper
    # neighbour does; the lower neighbour takes 4.0 and finds it
    roles = np.array(c["roles"])
    vc = c["mps"].view_cos
    hit = np.isin(c["ids"], exp[0])
    assert not hit[(roles == "radius") & (vc >= F32(0.998))].any()
    assert hit[(roles == "radius") & (vc < F32(0.998))].all()
    assert not hit[roles == "level_above"].any() and hit[roles == "stereo_edge"].all()
    for m in G.LOCAL_GATE_EQUIVALENT:
        got = G.restated_local(c["f"], c["mps"], c["th"], c["nnratio"], mp_ids=c["ids"], mutant=m)
        assert same(got[:2], exp[:2]) and got[2] == exp[2], m


@pytest.mark.parametrize("mutant", G.LOCAL_GATE_MUTANTS)
def test_local_gate_mutant_changes_an_output(mutant):
    seen = False
    for th in PC.RADIUS_THS:
        c = PC.radius_case(th)
        exp = G.restated_local(c["f"], c["mps"], c["th"], c["nnratio"], mp_ids=c["ids"])
        got = G.restated_local(c["f"], c["mps"], c["th"], c["nnratio"], mp_ids=c["ids"], mutant=mutant)
        seen |= not (same(got[:2], exp[:2]) and got[2] == exp[2])
    assert seen


@pytest.mark.parametrize("name", ["identity", "seeded", "depth"])
def test_search_local_points_restatement_equals_oracle(name):
    """restatement o restatement against oracle o oracle on the built scenes (the points whose
    level leaves the pyramid flagged bad: the oracle refuses them), and the scene with them:
    unsupported, the other points' results the same."""
    sc = scene(name, "pyramid")
    inv, fmp, fobs, nm, nto, uns, mps = PC.restated_search_local_points(sc)
    assert not uns and nm >= (60 if name != "depth" else 1)
    lm = sc["lm"]
    o = oracle.is_in_frustum(**sc["case"].args())
    oinv = o[0].copy()
    oinv[(lm["skip"] > 0) | (lm["bad"] > 0)] = 0
    assert np.array_equal(oinv, inv)
    omps = MapPoints(o[1], o[2], o[4], o[5], lm["desc"], lm["nobs"], track_in_view=oinv,
                     is_bad=lm["bad"], proj_xr=o[3])
    assert _local_oracle_equal(sc["f"], omps, 1.0, 0.8, lm["frame_mp"], lm["frame_mp_obs"],
                               lm["ids"], (fmp, fobs, nm))
    full = PC.restated_search_local_points(scene(name, "all"))
    assert full[5] and same(full[1:3], (fmp, fobs)) and full[3] == nm and full[4] > nto
    # the flags sit on points that are on a bound
    assert lm["skip"].sum() >= (5 if name != "depth" else 1)
    # no window holds more than the fused kernel's 16 candidate slots: its own answer is the
    # one the GPU test compares, not the CSR rerun's
    g = G.Grid(sc["f"])
    m = full[6]
    widest = 0
    for i in np.flatnonzero((m.track_in_view > 0) & (m.pred_level >= 0) & (m.pred_level < PC.NLEVELS)):
        pl = int(m.pred_level[i])
        rs = G.radius_by_viewing_cos(m.view_cos[i], 1.0) * sc["f"].scale_factors[pl]
        widest = max(widest, len(g.area(m.proj_x[i], m.proj_y[i], rs, pl - 1, pl)))
    assert (4 if name == "depth" else 8) <= widest <= 16


@pytest.mark.parametrize("mutant", [m for m in PC.FRUSTUM_MUTANTS if m != "level_log_float"])
def test_frustum_mutant_changes_search_local_points(mutant):
    """The same mutants seen through the search: in_view, nToMatch or a slot changes.  (Not
    level_log_float: where it differs here it predicts one level more, and the window
    [L, L + 1] still holds the point's keypoint of octave L; it shows on the level itself.)"""
    seen = False
    for name, c in frustum_cases().items():
        sc = PC.frustum_scene(c, flags=False)
        exp = PC.restated_search_local_points(sc)
        got = PC.restated_search_local_points(sc, mutant=mutant)
        seen |= not (same(got[:3], exp[:3]) and got[3:6] == exp[3:6])
    assert seen


# ==== CPU: SearchByProjection, last frame ========================================================

def _last(c, check_ori=True, **kw):
    return G.restated_last(c, c["th"], c["mono"], check_ori, c["frame_mp"], c["frame_mp_obs"], **kw)


def test_last_cases_equal_oracle_and_reach_their_branches():
    tot = {}
    modes = {}
    for name, c in last_cases().items():
        st = {}
        exp = _last(c, stats=st)
        o = oracle.search_by_projection_last(*G.last_args(c), c["th"], c["mono"], True,
                                             c["frame_mp"], c["frame_mp_obs"], c["last_ids"])
        assert same(o[:2], exp[:2]) and o[2] == exp[2], name
        for k, v in st.items():
            tot[k] = tot.get(k, 0) + v
        modes[name] = G.last_motion(c, c["mono"])
        groups = PC.last_group_check(c)
        assert set(groups) == {"u_max", "u_min", "v_max", "v_min"}
        assert all(h >= 1 for _, h in groups.values()), groups     # the exact camera hits them
    for k in LAST_COUNTERS:
        assert tot.get(k, 0) >= 5, (k, tot)
    # tlc.z == mb is neither forward nor backward; its upper neighbour is, unless bMono
    for side, mode in (("fwd", (True, False)), ("bwd", (False, True))):
        assert modes[f"{side}_above_stereo"] == mode
        for other in ("below_stereo", "on_stereo", "below_mono", "on_mono", "above_mono"):
            assert modes[f"{side}_{other}"] == (False, False)


def test_last_window_winners_name_the_mode():
    """Keypoints of octaves 7, 0, o + 1, o - 1, o at distances 1 .. 5: forward [o, -) takes
    octave 7, backward [0, o] octave 0, neither the nearest of them inside [o - 1, o + 1]."""
    for name, want in (("fwd_above_stereo", 7), ("bwd_above_stereo", 0), ("fwd_on_stereo", None)):
        c = last_cases()[name]
        fmp = _last(c, check_ori=False)[0]
        win = np.flatnonzero(np.array(c["tags"]) == "window")
        assert len(win) >= 10
        for i in win:
            slot = np.flatnonzero(fmp == c["last_ids"][i])
            assert len(slot) == 1
            o = int(c["last_keys"]["octave"][i])
            both = 7 if o + 1 == 7 else 0 if o - 1 == 0 else o + 1
            assert c["cur"].keys["octave"][slot[0]] == (both if want is None else want)


@pytest.mark.parametrize("mutant", G.LAST_GATE_MUTANTS)
def test_last_gate_mutant_changes_an_output(mutant):
    seen = False
    for c in last_cases().values():
        exp, got = _last(c), _last(c, mutant=mutant)
        seen |= not (same(got[:2], exp[:2]) and got[2] == exp[2])
    assert seen


@pytest.mark.parametrize("mutant", G.LAST_GATE_EQUIVALENT)
def test_last_gate_equivalences(mutant):
    for name, c in last_cases().items():
        st, stm = {}, {}
        exp, got = _last(c, stats=st), _last(c, mutant=mutant, stats=stm)
        assert same(got[:2], exp[:2]) and got[2] == exp[2], name
        if mutant == "depth_z_lt0" and name == "depth":
            # -0.0f does take the other branch; what follows finds nothing either way
            assert stm.get("behind", 0) < st["behind"]


# ==== CPU: SearchByProjection, keyframe ==========================================================

@pytest.mark.parametrize("name", ["identity", "seeded"])
def test_keyframe_case_equals_oracle(name):
    c = keyframe_case(name, "pyramid")
    exp = K.restated(c, c["th"], c["orb_dist"])
    o = oracle.search_by_projection_keyframe(c, c["th"], c["orb_dist"])
    assert o[1] == exp[1] >= 100 and np.array_equal(o[0], exp[0])
    full = keyframe_case(name, "all")
    info = {}
    got = K.restated(full, full["th"], full["orb_dist"], info=info)
    assert info["unsupported"] and got[1] == exp[1] and np.array_equal(got[0], exp[0])
    with pytest.raises(OrbfeError) as e:
        oracle.search_by_projection_keyframe(full, full["th"], full["orb_dist"])
    assert e.value.status == ORBFE_ERR_UNSUPPORTED


def test_keyframe_branch_counters_and_mutants():
    tot = {}
    seen = set()
    for name in ("identity", "seeded"):
        c = keyframe_case(name, "all")
        st = {}
        exp = K.restated(c, c["th"], c["orb_dist"], stats=st)
        for k, v in st.items():
            tot[k] = tot.get(k, 0) + v
        for m in K.GATE_MUTANTS:
            got = K.restated(c, c["th"], c["orb_dist"], mutant=m)
            if got[1] != exp[1] or not np.array_equal(got[0], exp[0]):
                seen.add(m)
        for m in K.GATE_EQUIVALENT:
            got = K.restated(c, c["th"], c["orb_dist"], mutant=m)
            assert got[1] == exp[1] and np.array_equal(got[0], exp[0]), m
        # a point behind the camera that projects into the image is searched and matched
        behind = np.flatnonzero(np.array(c["tags"]) == "behind")
        assert len(behind) >= 5 and np.isin(c["kf_ids"][behind], exp[0]).all()
    assert seen == set(K.GATE_MUTANTS)
    for k in KEYFRAME_COUNTERS:
        assert tot.get(k, 0) >= 5, (k, tot)


# ==== CPU: Fuse ==================================================================================

@pytest.mark.parametrize("name", ["identity", "seeded"])
def test_fuse_builders_reach_their_gates(name):
    fc = fuse_cases()[name]
    groups = fc.check_groups()
    assert set(groups) == set(PC.FUSE_GATES)
    for gate in PC.FUSE_GATES:
        assert groups[gate][0] >= 3, (gate, groups)
    # e2 * invSigma2 == (float)7.8 and the image bounds are hit exactly
    for gate in ("u_max", "v_max", "chi2_stereo") + (("u_min", "v_min", "dist_min", "dist_max", "vcos")
                                                     if name == "identity" else ()):
        assert groups[gate][1] >= 1, (gate, groups)
    c = fc.case()
    plain = sum(t == "plain" for t in c["tags"])
    assert plain * 10 <= len(c["tags"]) and c["kf"].n <= 256 and len(c["xyz"]) <= 600


def test_fuse_branch_counters_and_mutants():
    tot = {}
    seen = {SE3: set(), SIM3: set()}
    for name in fuse_cases():
        c = fuse_case(name, "all")
        for mode, th in ((SE3, 3.0), (SIM3, 4.0)):
            st = {}
            exp = FC.restated(c, th, mode, stats=st)
            assert exp[3] and exp[2] >= 1
            for k, v in st.items():
                tot[k] = tot.get(k, 0) + v
            for m in FC.GATE_MUTANTS:
                if not same(FC.restated(c, th, mode, mutant=m)[:2], exp[:2]):
                    seen[mode].add(m)
            for m in FC.GATE_EQUIVALENT:
                assert same(FC.restated(c, th, mode, mutant=m)[:2], exp[:2]), (name, m)
    assert seen[SE3] == set(FC.GATE_MUTANTS) - {"sim3_has_chi2"}
    assert seen[SIM3] == set(FC.GATE_MUTANTS) - set(FC.SE3_ONLY)
    for k in FUSE_COUNTERS:
        assert tot.get(k, 0) >= 5, (k, tot)


def test_fuse_zero_depth_leaves_at_the_image_test():
    c = fuse_case("depth", "all")
    ow = FC.camera_center(c["tcw"].astype(F32))
    zero = [i for i in range(len(c["xyz"])) if FC.project(c, i, ow)["pc"][2] == 0]
    assert len(zero) >= 8
    assert all(FC.project(c, i, ow)["reject"] == "image" for i in zero)
    assert all(FC.project(c, i, ow, "depth_le0")["reject"] == "depth" for i in zero)


def test_fuse_batch_keyframes_have_answers_of_their_own():
    c, kfs, poses, skips = PC.fuse_batch(81)
    assert all(f.n == 8 for f in kfs) and len(c["xyz"]) == 12
    for k in (0, 39, 40, 41, 80):
        own = FC.restated(dict(c, kf=kfs[k], tcw=poses[k], skip=skips[k]), 3.0, SE3)
        other = FC.restated(dict(c, kf=kfs[k], tcw=poses[(k + 40) % 80], skip=skips[k]), 3.0, SE3)
        assert own[2] >= 3 and other[2] == 0, k


# ==== GPU ========================================================================================

@pytest.fixture(scope="module")
def mts():
    from orbslam_mapsave_amd.native import ORBmatcher
    ms = {ori: ORBmatcher(0.8, ori, device=0) for ori in (True, False)}
    yield ms
    for m in ms.values():
        m.close()


def _sentinels(n):
    return (np.full(n, 9, np.uint8), np.full(n, PC.SENTINEL_F, F32), np.full(n, PC.SENTINEL_F, F32),
            np.full(n, PC.SENTINEL_F, F32), np.full(n, PC.SENTINEL_I, np.int32),
            np.full(n, PC.SENTINEL_F, F32))


def _gpu_frustum(mt, a):
    out = _sentinels(len(a["xyz"]))
    got = mt.is_in_frustum(**a, out=out)
    assert all(g is o for g, o in zip(got, out))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["identity", "seeded", "depth"])
def test_gpu_is_in_frustum_built_cases(mts, name):
    """in_view for every point, the five outputs bit-exact where in view, the sentinels still
    there where not."""
    got = _gpu_frustum(mts[False], frustum_cases()[name].args())
    assert PC.frustum_equal(got, frustum_expected(name)[0], (PC.SENTINEL_F, PC.SENTINEL_I))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_gpu_is_in_frustum_sizes(mts, n):
    """The wave and block seams of a thread-per-point kernel, on a mix of every gate's points."""
    c = frustum_cases()["identity"]
    idx = (np.arange(n) * 7) % len(c.tag)
    a = c.args(idx)
    exp = tuple(x[idx] for x in frustum_expected("identity")[0])
    assert n < 63 or 0 < exp[0].sum() < n
    assert PC.frustum_equal(_gpu_frustum(mts[False], a), exp, (PC.SENTINEL_F, PC.SENTINEL_I))


def _slp_device(mt, sc, th=1.0, nnratio=0.8):
    """orbfe_search_local_points_device on device copies of the scene -> ((nmatches, nToMatch),
    status, in_view, frame_mp, frame_mp_obs)."""
    import torch
    dev = torch.device("cuda", 0)
    f, lm = sc["f"], sc["lm"]
    m = len(lm["xyz"])
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in lm.items()}
    d_keys = torch.from_numpy(f.keys.view(np.uint8).copy()).to(dev)
    d_desc = torch.from_numpy(f.desc).to(dev)
    d_inv = torch.full((m,), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    status = 0
    try:
        r = mt.search_local_points_device(
            f.n, d_keys.data_ptr(), d_desc.data_ptr(), None, S.W, S.H, f.scale_factors, lm["tcw"],
            sc["cam"], float(PC.LOG_SCALE), 0.5, m, T["xyz"].data_ptr(), T["normal"].data_ptr(),
            T["min_dist"].data_ptr(), T["max_dist"].data_ptr(), T["desc"].data_ptr(),
            T["nobs"].data_ptr(), T["bad"].data_ptr(), T["skip"].data_ptr(), T["ids"].data_ptr(),
            nnratio, th, T["frame_mp"].data_ptr(), T["frame_mp_obs"].data_ptr(), d_inv.data_ptr())
    except OrbfeError as e:
        status, r = e.status, e.results
    torch.cuda.synchronize()
    return r, status, d_inv.cpu().numpy(), T["frame_mp"].cpu().numpy(), T["frame_mp_obs"].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("levels", ["pyramid", "all"])
@pytest.mark.parametrize("name", ["identity", "seeded", "depth"])
def test_gpu_search_local_points_built_cases(mts, name, levels):
    """sbp_local_fused_kernel's own evaluation of frustum_eval, skip / bad set on points that
    sit on a bound: in_view, nToMatch, slots, nmatches against restatement o restatement; with
    the levels outside the pyramid left in, ORBFE_ERR_UNSUPPORTED and the same slots."""
    sc = scene(name, levels)
    inv, fmp, fobs, nm, nto, uns, _ = PC.restated_search_local_points(sc)
    assert uns == (levels == "all")
    before = mts[False].capacity_retries()
    r, status, ginv, gfmp, gfobs = _slp_device(mts[False], sc)
    assert mts[False].capacity_retries() == before       # the fused kernel's own answer
    assert status == (ORBFE_ERR_UNSUPPORTED if uns else 0)
    assert np.array_equal(ginv, inv)
    assert r == (nm, nto)
    assert np.array_equal(gfmp, fmp) and np.array_equal(gfobs, fobs)


def _sbp_local_device(mt, f, mps, th, nnratio, ids, fmp0, fobs0):
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    D = {k: up(v) for k, v in dict(inv=mps.track_in_view, bad=mps.is_bad, px=mps.proj_x,
                                   py=mps.proj_y, pxr=mps.proj_xr, pl=mps.pred_level,
                                   vc=mps.view_cos, desc=mps.desc, nobs=mps.n_obs, ids=ids,
                                   fmp=fmp0, fobs=fobs0).items()}
    d_keys, d_desc = up(f.keys.view(np.uint8)), up(f.desc)
    d_ur = up(f.u_right) if f.u_right is not None else None
    torch.cuda.synchronize()
    status = 0
    try:
        nm = mt.search_by_projection_local_device(
            f.n, d_keys.data_ptr(), d_desc.data_ptr(), d_ur.data_ptr() if d_ur is not None else None,
            S.W, S.H, f.scale_factors, mps.m, D["inv"].data_ptr(), D["bad"].data_ptr(),
            D["px"].data_ptr(), D["py"].data_ptr(), D["pxr"].data_ptr(), D["pl"].data_ptr(),
            D["vc"].data_ptr(), D["desc"].data_ptr(), D["nobs"].data_ptr(), D["ids"].data_ptr(),
            nnratio, th, D["fmp"].data_ptr(), D["fobs"].data_ptr())
    except OrbfeError as e:
        status, nm = e.status, e.results
    torch.cuda.synchronize()
    return nm, status, D["fmp"].cpu().numpy(), D["fobs"].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "csr"])
@pytest.mark.parametrize("name", ["identity", "seeded", "depth"])
def test_gpu_search_by_projection_local_device_built_cases(mts, name, path, monkeypatch):
    """The search alone on the restated isInFrustum outputs (NaN centres and levels outside the
    pyramid among them), on the fused path and with the CSR path forced."""
    if path == "csr":
        monkeypatch.setenv("ORBFE_SBP_DEVICE_CSR", "1")
    else:
        monkeypatch.delenv("ORBFE_SBP_DEVICE_CSR", raising=False)
    sc = scene(name, "all")
    inv, fmp, fobs, nm, nto, uns, mps = PC.restated_search_local_points(sc)
    lm = sc["lm"]
    gnm, status, gfmp, gfobs = _sbp_local_device(mts[False], sc["f"], mps, 1.0, 0.8, lm["ids"],
                                                 lm["frame_mp"], lm["frame_mp_obs"])
    assert uns and status == ORBFE_ERR_UNSUPPORTED and gnm == nm
    assert np.array_equal(gfmp, fmp) and np.array_equal(gfobs, fobs)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "csr"])
@pytest.mark.parametrize("th", PC.RADIUS_THS)
def test_gpu_local_radius_cases(mts, th, path, monkeypatch):
    """RadiusByViewingCos at (float)0.998 and `th != 1.0` at nextafter(1.0f): the host form and
    orbfe_search_by_projection_local_device."""
    if path == "csr":
        monkeypatch.setenv("ORBFE_SBP_DEVICE_CSR", "1")
    else:
        monkeypatch.delenv("ORBFE_SBP_DEVICE_CSR", raising=False)
    c = PC.radius_case(th)
    f, mps = c["f"], c["mps"]
    exp = G.restated_local(f, mps, c["th"], c["nnratio"], mp_ids=c["ids"])
    assert exp[2] >= 8
    got = mts[False].SearchByProjection(f, mps, c["th"], mp_ids=c["ids"])
    assert got[2] == exp[2] and same(got[:2], exp[:2])
    nm, status, fmp, fobs = _sbp_local_device(mts[False], f, mps, c["th"], c["nnratio"], c["ids"],
                                              np.full(f.n, -1, np.int32), np.zeros(f.n, np.int32))
    assert status == 0 and nm == exp[2] and same((fmp, fobs), exp[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [True, False])
def test_gpu_search_by_projection_last_built_cases(mts, ori):
    """tlc.z on +-mb and beside it, bMono on and off; u and v on the image bounds; -0.0f, zero
    and denormal depth: slots, Observations and nmatches of all thirteen cases."""
    for name, c in last_cases().items():
        exp = _last(c, check_ori=ori)
        got = mts[ori].SearchByProjectionLast(*G.last_args(c), c["th"], c["mono"], c["frame_mp"],
                                              c["frame_mp_obs"], c["last_ids"])
        assert got[2] == exp[2] >= 25, name
        assert same(got[:2], exp[:2]), name


def _gpu_keyframe(mt, c):
    status = 0
    try:
        r = mt.SearchByProjectionKeyFrame(
            c["cur"], c["tcw_cur"], c["cam"], c["log_scale"], c["kf_angle"], c["kf_valid"],
            c["kf_bad"], c["found"], c["kf_xyz"], c["kf_desc"], c["kf_min"], c["kf_max"], c["th"],
            c["orb_dist"], frame_mp=c["frame_mp"], kf_ids=c["kf_ids"])
    except OrbfeError as e:
        status, r = e.status, e.results
    return r, status


@pytest.mark.gpu
@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("levels", ["pyramid", "all"])
@pytest.mark.parametrize("name", ["identity", "seeded"])
def test_gpu_search_by_projection_keyframe_built_cases(mts, name, levels, ori):
    c = keyframe_case(name, levels)
    info = {}
    exp = K.restated(c, c["th"], c["orb_dist"], ori, info=info)
    r, status = _gpu_keyframe(mts[ori], c)
    assert status == (ORBFE_ERR_UNSUPPORTED if levels == "all" else 0)
    assert bool(info.get("unsupported")) == (levels == "all")
    assert r[1] == exp[1] >= 100 and np.array_equal(r[0], exp[0])


def _gpu_fuse(mt, c, th, mode):
    status = 0
    try:
        r = mt.FuseSearch(c["kf"], c["tcw"], c["cam"], c["log_scale"], c["inv_sigma2"], c["xyz"],
                          c["normal"], c["min_dist"], c["max_dist"], c["desc"], th=th, mode=mode,
                          skip=c["skip"])
    except OrbfeError as e:
        status, r = e.status, e.results
    return r, status


@pytest.mark.gpu
@pytest.mark.parametrize("mode,th", [(SE3, 3.0), (SIM3, 4.0)])
@pytest.mark.parametrize("levels", ["pyramid", "all"])
@pytest.mark.parametrize("name", ["identity", "seeded", "depth"])
def test_gpu_fuse_search_built_cases(mts, name, levels, mode, th):
    c = fuse_case(name, levels)
    exp = FC.restated(c, th, mode)
    assert exp[3] == (levels == "all")
    r, status = _gpu_fuse(mts[False], c, th, mode)
    assert status == (ORBFE_ERR_UNSUPPORTED if levels == "all" else 0)
    assert r[2] == exp[2] and np.array_equal(r[0], exp[0]) and np.array_equal(r[1], exp[1])


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,mode,th", [(1, SE3, 3.0), (39, SIM3, 4.0), (40, SE3, 3.0),
                                           (41, SIM3, 4.0), (80, SIM3, 4.0), (81, SE3, 3.0)])
def test_gpu_fuse_batch_seams(mts, n_kf, mode, th):
    """Batches around the 40 keyframes one launch carries: every keyframe's row against the host
    form called for it alone and against the restatement.  The poses differ, so a launch that
    lost its first keyframe's index answers for another keyframe and finds nothing."""
    from test_fuse import run_batch
    c, kfs, poses, skips = PC.fuse_batch(n_kf)
    bi, bd, st = run_batch(mts[False], c, kfs, poses, skips, th, mode)
    assert st == 0
    found = 0
    for k in range(n_kf):
        ck = dict(c, kf=kfs[k], tcw=poses[k], skip=skips[k])
        e = FC.restated(ck, th, mode)
        assert not e[3]
        assert np.array_equal(bi[k], e[0]) and np.array_equal(bd[k], e[1]), k
        (hbi, hbd, hnf), status = _gpu_fuse(mts[False], ck, th, mode)
        assert status == 0 and np.array_equal(bi[k], hbi) and np.array_equal(bd[k], hbd), k
        found += e[2]
    assert found >= 3 * n_kf
