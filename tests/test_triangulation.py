"""ORBmatcher::SearchForTriangulation (ORBmatcher.cc:660-826): orbfe_search_for_triangulation and
orbfe_search_for_triangulation_batch_device against the pure-Python restatement of
tests/triangulation_cases.py (the parity reference: the oracle has no such matcher).

CPU: every single-decision mutant of the restatement changes an answer on some built case, every
branch is reached at least five times over the case set, and bad arguments are refused without a
device.  GPU: vMatches12, nmatches and the pair list bit-exact on every built case under every
(check_ori, block_matched2, only_stereo), degenerate sizes, the register-slot seams of a node
(63 / 64 / 65 / 256 keyframe-2 features), the two error statuses, the device batch against the
host form pair by pair, and the batch fed straight from orbfe_bow_transform_batch_device.
"""
import functools

import numpy as np
import pytest

import triangulation_cases as TC
from orbslam_mapsave_amd.abi import (KEYPOINT_DTYPE, ORBFE_ERR_ARG, ORBFE_ERR_UNSUPPORTED, Frame,
                                     OrbfeError)

F32 = np.float32
CASES = sorted(TC.built_cases())

# every branch counter of the restatement that must be reached (>= 5 times over the case set)
BRANCHES = ("node_common", "node_skip1", "node_skip2", "kf1_has_mp", "kf1_not_stereo", "c2_blocked",
            "c2_has_mp", "c2_not_stereo", "dist_51", "dist_gt_th", "dist_gt_best", "tie_replace",
            "match_at_50", "epi_equal", "epi_reject", "epi_pass", "epi_near_pass",
            "epi_stereo_inside", "den0", "line_pass", "line_reject", "thr_double_differs", "match",
            "no_match", "rematched2", "rot_wrap", "bin30", "ori_dropped")


@functools.lru_cache(maxsize=None)
def expected(name, cfg):
    st = {}
    m12, n, pairs = TC.restated(TC.built_cases()[name], *cfg, stats=st)
    return m12, n, pairs, st


def test_restatement_is_consistent():
    for name in CASES:
        for cfg in TC.CONFIGS:
            m12, n, pairs, _ = expected(name, cfg)
            assert n == int((m12 >= 0).sum()) == len(pairs)
            assert np.array_equal(pairs[:, 1], m12[pairs[:, 0]]) and (np.diff(pairs[:, 0]) > 0).all()
            if cfg[1]:   # with the blocking, a keyframe-2 feature is matched at most once
                assert len(set(pairs[:, 1].tolist())) == n
    # the literal source matches some keyframe-2 features several times
    assert expected("pose0", (False, False, False))[3]["rematched2"] > 20
    assert expected("pose0", (False, False, False))[1] > 150
    assert expected("den0", (True, True, False))[1] == 0
    assert expected("threshold", (False, True, False))[1] == 7


@pytest.mark.parametrize("mutant", TC.MUTANTS)
def test_each_mutant_changes_an_answer(mutant):
    """A restatement with one decision flipped must disagree somewhere: otherwise the built cases
    could not tell a kernel with that mistake from a correct one."""
    for name in CASES:
        c = TC.built_cases()[name]
        for cfg in TC.CONFIGS:
            m12, n, _, _ = expected(name, cfg)
            g12, gn, _ = TC.restated(c, *cfg, mutant=mutant)
            if gn != n or not np.array_equal(g12, m12):
                return
    pytest.fail(f"mutant {mutant} gives the reference's answer on every built case")


def test_every_branch_is_reached():
    tot = {}
    for name in CASES:
        for cfg in TC.CONFIGS:
            for k, v in expected(name, cfg)[3].items():
                tot[k] = tot.get(k, 0) + v
    short = {k: tot.get(k, 0) for k in BRANCHES if tot.get(k, 0) < 5}
    assert not short, short
    # matches the orientation filter drops whose keyframe-2 feature a later keyframe-1 feature of
    # the node would otherwise take: answers that change when the filter releases the blocking
    changed = 0
    for name in CASES:
        m12 = expected(name, (True, True, False))[0]
        g12 = TC.restated(TC.built_cases()[name], True, True, False, mutant="block_released")[0]
        changed += int((g12 != m12).sum())
    assert changed >= 5, changed


def test_threshold_case_separates_double_from_float():
    c = TC.threshold_case()
    m12 = TC.restated(c, False, True, False)[0]
    f12 = TC.restated(c, False, True, False, mutant="thr_float")[0]
    assert (m12[:6] >= 0).all() and (f12[:6] == -1).all()      # dsqr == (float)3.84f
    assert m12[6] == -1 and f12[6] == -1 and m12[7] >= 0 and f12[7] >= 0


def test_null_and_bad_arguments():
    from orbslam_mapsave_amd import native
    lib = native.lib()
    assert lib.orbfe_search_for_triangulation(
        None, 0, 0, 0, None, None, 0, None, None, None, None, None, 0, None, None, None, None,
        None, None, None, None) == ORBFE_ERR_ARG
    assert lib.orbfe_search_for_triangulation_batch_device(
        None, 0, 0, 0, 0, None, None, None, None, None, None, None, None, None, -1, None, None,
        None, None, None, None, 0, None, None, None) == ORBFE_ERR_ARG


# ---- GPU ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mts():
    from orbslam_mapsave_amd.native import ORBmatcher
    m = {ori: ORBmatcher(0.6, ori, device=0) for ori in (False, True)}
    yield m
    for x in m.values():
        x.close()


def gpu_search(mts, c, cfg):
    ori, blk, st = cfg
    mt = mts[ori]
    pairs, n = mt.SearchForTriangulation(c["kf1"], c["mp1"], c["fv1"], c["kf2"], c["mp2"], c["fv2"],
                                         c["F12"], c["epipole"], c["sigma2"], bOnlyStereo=st,
                                         block_matched2=blk)
    return mt.vMatches12, n, pairs


def check(got, exp, what=""):
    m12, n, pairs = got
    assert np.array_equal(m12, exp[0]), (what, np.flatnonzero(m12 != exp[0])[:10])
    assert n == exp[1], what
    assert np.array_equal(pairs, exp[2]), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_host_form(mts, name):
    c = TC.built_cases()[name]
    for cfg in TC.CONFIGS:
        check(gpu_search(mts, c, cfg), expected(name, cfg), cfg)


@pytest.mark.gpu
def test_gpu_host_form_monocular(mts):
    """u_right NULL on both sides: every feature is monocular, so the epipole test always runs
    and bOnlyStereo leaves nothing."""
    c = TC.monocular(TC.tri_case(1))
    for cfg in TC.CONFIGS:
        exp = TC.restated(c, *cfg)
        assert (exp[1] == 0) == cfg[2]
        check(gpu_search(mts, c, cfg), exp, cfg)


def _empty_side(c, side):
    kf = Frame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), TC.W, TC.H, TC.SCALE)
    fv = tuple(np.zeros(k, np.int32) for k in (0, 1, 0))
    return dict(c, **{"kf" + side: kf, "mp" + side: np.zeros(0, np.uint8), "fv" + side: fv})


def degenerate_cases():
    base = TC.band_case((5, 3), seed=2)
    apart = dict(base, fv2=(base["fv2"][0] + 1, base["fv2"][1], base["fv2"][2]))
    return {"n1=0": _empty_side(base, "1"), "n2=0": _empty_side(base, "2"), "no common node": apart,
            "every kf1 feature has a MapPoint": TC.band_case((5, 3), seed=2, all_mp1=True),
            "one feature per side": TC.band_case((1,), seed=3)}


def test_degenerate_cases_restated():
    d = degenerate_cases()
    for name, c in d.items():
        n = TC.restated(c, True, True, False)[1]
        assert n == (1 if name == "one feature per side" else 0), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(degenerate_cases()))
def test_gpu_degenerate(mts, name):
    c = degenerate_cases()[name]
    for cfg in ((True, True, False), (False, False, False)):
        check(gpu_search(mts, c, cfg), TC.restated(c, *cfg), cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [63, 64, 65, 256])
def test_gpu_node_size_seams(mts, size):
    """A node of `size` keyframe-2 features (4 register slots of 64 lanes), every one of them the
    winner of two keyframe-1 features in turn, beside two small nodes."""
    c = TC.band_case((3, size, 7), seed=size, dup=True)
    for cfg in ((True, True, False), (False, False, False)):
        exp = TC.restated(c, *cfg)
        assert exp[1] == (size + 10 if cfg[1] else 2 * (size + 10))
        check(gpu_search(mts, c, cfg), exp, cfg)


@pytest.mark.gpu
def test_gpu_node_over_256_is_unsupported(mts):
    """257 keyframe-2 features in a common node: ORBFE_ERR_UNSUPPORTED, that node skipped, the
    other nodes' results intact; the status does not stick to the matcher."""
    c = TC.band_case((4, 257, 6), seed=5)
    ids2, off2, feat2 = c["fv2"]
    assert off2[2] - off2[1] == 257
    skipped = dict(c, fv2=(ids2 + np.array([0, 1, 0], np.int32), off2, feat2))
    exp = TC.restated(skipped, True, True, False)
    assert exp[1] == 10
    with pytest.raises(OrbfeError) as e:
        gpu_search(mts, c, (True, True, False))
    assert e.value.status == ORBFE_ERR_UNSUPPORTED
    assert np.array_equal(mts[True].vMatches12, exp[0])
    assert e.value.results[1] == exp[1] and np.array_equal(e.value.results[0], exp[2])
    ok = TC.band_case((4, 256, 6), seed=5)
    check(gpu_search(mts, ok, (True, True, False)), TC.restated(ok, True, True, False))


@pytest.mark.gpu
def test_gpu_octave_outside_pyramid_is_bad_argument(mts):
    """A keyframe-2 octave equal to nlevels (where the reference indexes mvScaleFactors and
    mvLevelSigma2 out of range): ORBFE_ERR_ARG, that candidate skipped, every other result valid."""
    c = TC.band_case((6, 9), seed=6)
    victim = int(c["fv2"][2][2])
    keys = c["kf2"].keys.copy()
    keys["octave"][victim] = TC.NLEVELS
    bad = dict(c, kf2=Frame(keys, c["kf2"].desc, TC.W, TC.H, TC.SCALE))
    mp2 = c["mp2"].copy()
    mp2[victim] = 1                                     # skipped like a feature with a MapPoint
    exp = TC.restated(dict(c, mp2=mp2), False, True, False)
    assert exp[1] == 14
    with pytest.raises(OrbfeError) as e:
        gpu_search(mts, bad, (False, True, False))
    assert e.value.status == ORBFE_ERR_ARG
    assert np.array_equal(mts[False].vMatches12, exp[0]) and e.value.results[1] == exp[1]


@pytest.mark.gpu
def test_gpu_repeated_feature_index_is_bad_argument(mts):
    c = TC.band_case((6, 9), seed=6)
    ids, off, feat = c["fv2"]
    feat = feat.copy()
    feat[1] = feat[0]
    with pytest.raises(OrbfeError) as e:
        gpu_search(mts, dict(c, fv2=(ids, off, feat)), (False, True, False))
    assert e.value.status == ORBFE_ERR_ARG


def _prefix(kf, mp, fv, n):
    """The keyframe cut to its first n features (its FeatureVector without the others)."""
    ids, off, feat = fv
    nodes = np.full(kf.n, -1)
    for k in range(len(ids)):
        nodes[feat[off[k]:off[k + 1]]] = ids[k]
    ur = None if kf.u_right is None else kf.u_right[:n]
    return (Frame(kf.keys[:n], kf.desc[:n], TC.W, TC.H, TC.SCALE, ur), mp[:n],
            TC.feature_vector(nodes[:n], n))


def slabs(slots, cap, dev, stereo=True):
    """[(Frame, has_mp, fv)] -> device arrays in orbfe_bow_transform_batch_device's layout plus
    the keypoint, mvuRight and map-point-flag slabs; unused entries hold poison."""
    import torch
    ns = len(slots)
    keys = np.zeros((ns, cap), KEYPOINT_DTYPE)
    keys["octave"] = 99
    desc = np.full((ns, cap, 32), 0xAB, np.uint8)
    ur = np.full((ns, cap), 7.0, F32)
    mp = np.full((ns, cap), 0, np.uint8)
    n = np.zeros(ns, np.int32)
    nn = np.zeros(ns, np.int32)
    nid = np.full((ns, cap), -5, np.int32)
    off = np.full((ns, cap + 1), -5, np.int32)
    feat = np.full((ns, cap), -5, np.int32)
    for s, (kf, m, fv) in enumerate(slots):
        keys[s, :kf.n], desc[s, :kf.n], mp[s, :kf.n] = kf.keys, kf.desc, m
        if stereo:
            ur[s, :kf.n] = kf.u_right
        n[s], nn[s] = kf.n, len(fv[0])
        nid[s, :len(fv[0])], off[s, :len(fv[1])], feat[s, :len(fv[2])] = fv
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    return dict(keys=up(keys), desc=up(desc), ur=up(ur) if stereo else None, mp=up(mp), n=up(n),
                nn=up(nn), nid=up(nid), off=up(off), feat=up(feat))


def run_batch(mt, d, cap, pairs, f12, epi, blk, st, scale=TC.SCALE, sigma2=TC.SIGMA2):
    import torch
    dev = d["keys"].device
    P = len(pairs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    p1, p2 = up(np.array([p[0] for p in pairs], np.int32)), up(np.array([p[1] for p in pairs], np.int32))
    df, de = up(np.stack(f12).astype(F32)), up(np.stack(epi).astype(F32))
    out = torch.full((P * cap,), -7, dtype=torch.int32, device=dev)
    nm = torch.full((P,), -7, dtype=torch.int32, device=dev)
    stt = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    mt.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    mt.search_for_triangulation_batch_device(
        cap, d["keys"].data_ptr(), d["desc"].data_ptr(), d["ur"].data_ptr() if d["ur"] is not None else None,
        d["mp"].data_ptr(), d["n"].data_ptr(), d["nn"].data_ptr(), d["nid"].data_ptr(),
        d["off"].data_ptr(), d["feat"].data_ptr(), P, p1.data_ptr(), p2.data_ptr(), df.data_ptr(),
        de.data_ptr(), scale, sigma2, out.data_ptr(), nm.data_ptr(), stt.data_ptr(),
        bOnlyStereo=st, block_matched2=blk)
    torch.cuda.synchronize()
    mt.set_stream(None)
    return out.cpu().numpy().reshape(P, cap), nm.cpu().numpy(), int(stt.cpu()[0])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(True, True, False), (False, False, True), (True, False, False)])
def test_gpu_batch_device(mts, cfg):
    """One keyframe against 12 neighbours of different feature counts, plus a second keyframe 1
    against four of them, in slots of a capacity above every count: every pair equals the host
    form of the same pair, unused tail entries are -1."""
    import torch
    dev = torch.device("cuda", 0)
    ori, blk, st = cfg
    c0, c1 = TC.tri_case(0), TC.tri_case(1)
    slots = [(c0["kf1"], c0["mp1"], c0["fv1"])]
    slots += [_prefix(c0["kf2"], c0["mp2"], c0["fv2"], c0["kf2"].n - 17 * k) for k in range(12)]
    slots.append((c1["kf1"], c1["mp1"], c1["fv1"]))
    cap = 421
    assert all(s[0].n < cap for s in slots) and len({s[0].n for s in slots}) >= 13
    pairs = [(0, s) for s in range(1, 13)] + [(13, s) for s in (1, 5, 9, 12)]
    src = [c0] * 12 + [c1] * 4
    d = slabs(slots, cap, dev)
    out, nm, status = run_batch(mts[ori], d, cap, pairs, [c["F12"] for c in src],
                                [c["epipole"] for c in src], blk, st)
    assert status == 0
    total = 0
    for p, (s1, s2) in enumerate(pairs):
        c = dict(src[p], kf1=slots[s1][0], mp1=slots[s1][1], fv1=slots[s1][2], kf2=slots[s2][0],
                 mp2=slots[s2][1], fv2=slots[s2][2])
        h12, hn, _ = gpu_search(mts, c, cfg)
        n1 = slots[s1][0].n
        assert np.array_equal(out[p, :n1], h12) and nm[p] == hn, p
        assert (out[p, n1:] == -1).all(), p
        total += hn
    assert total > 300
    exp = TC.restated(c0, *cfg)     # pair 0 is the built case itself
    assert np.array_equal(out[0, :c0["kf1"].n], exp[0]) and nm[0] == exp[1]


@pytest.mark.gpu
def test_gpu_batch_device_errors_leave_other_pairs_valid(mts):
    """A pair whose common node holds 257 keyframe-2 features sets the status; the other pair of
    the same call is untouched."""
    import torch
    dev = torch.device("cuda", 0)
    big, ok = TC.band_case((4, 257, 6), seed=5), TC.band_case((3, 64, 7), seed=64, dup=True)
    slots = [(big["kf1"], big["mp1"], big["fv1"]), (big["kf2"], big["mp2"], big["fv2"]),
             (ok["kf1"], ok["mp1"], ok["fv1"]), (ok["kf2"], ok["mp2"], ok["fv2"])]
    cap = 300
    d = slabs(slots, cap, dev, stereo=False)
    out, nm, status = run_batch(mts[True], d, cap, [(0, 1), (2, 3)], [TC.BAND_F12] * 2,
                                [big["epipole"]] * 2, True, False)
    assert status == ORBFE_ERR_UNSUPPORTED
    exp = TC.restated(ok, True, True, False)
    assert np.array_equal(out[1, :ok["kf1"].n], exp[0]) and nm[1] == exp[1] == 74
    assert nm[0] == 10


@pytest.mark.gpu
def test_gpu_batch_reads_bow_transform_layout(mts, tmp_path):
    """orbfe_bow_transform_batch_device's outputs fed unchanged to the batch search: two extracted
    640 x 480 frames (the second the first shifted by two rows), a synthetic vocabulary, and the
    restatement run on the FeatureVectors downloaded from the device."""
    import torch

    import scenarios as S
    from orbslam_mapsave_amd.native import Vocabulary
    from orbslam_mapsave_amd.synth import synthetic_vocabulary_text
    dev = torch.device("cuda", 0)
    fr = [S.extract_frame(0, 1000, ini=20), S.extract_frame(0, 1000, shift=(2, -3), ini=20)]
    path = str(tmp_path / "voc.txt")
    synthetic_vocabulary_text(path, 10, 4, seed=0, anchors=fr[0].desc[::37])
    gv = Vocabulary(path, device=0)
    cap = max(f.n for f in fr) + 30
    desc = np.zeros((2, cap, 32), np.uint8)
    keys = np.zeros((2, cap), KEYPOINT_DTYPE)
    for i, f in enumerate(fr):
        desc[i, :f.n], keys[i, :f.n] = f.desc, f.keys
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    D, N = torch.from_numpy(desc).to(dev), torch.from_numpy(np.array([f.n for f in fr], np.int32)).to(dev)
    wid = torch.zeros((2, cap), dtype=torch.int32, device=dev)
    val = torch.zeros((2, cap), dtype=torch.float64, device=dev)
    nid = torch.zeros((2, cap), dtype=torch.int32, device=dev)
    off = torch.zeros((2, cap + 1), dtype=torch.int32, device=dev)
    feat = torch.zeros((2, cap), dtype=torch.int32, device=dev)
    nw = torch.zeros(2, dtype=torch.int32, device=dev)
    nn = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    gv.set_stream(stream)
    gv.transform_batch_device(2, D.data_ptr(), N.data_ptr(), cap, 2, wid.data_ptr(), val.data_ptr(),
                              nw.data_ptr(), nid.data_ptr(), off.data_ptr(), feat.data_ptr(),
                              nn.data_ptr())
    d = dict(keys=up(keys), desc=D, ur=None, mp=torch.zeros(2 * cap, dtype=torch.uint8, device=dev),
             n=N, nn=nn, nid=nid, off=off, feat=feat)
    scale = fr[0].scale_factors
    sigma2 = (scale * scale).astype(F32)
    # the second image is the first rolled by (2, -3): y2 = y1 + 2, the line test with c = -y1 - 2
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, -2]], F32)
    epi = np.array([-5000, -5000], F32)
    out, nm, status = run_batch(mts[True], d, cap, [(0, 1)], [F], [epi], True, False, scale, sigma2)
    gv.close()
    assert status == 0
    fvs = []
    for i in range(2):
        k = int(nn[i])
        o = off[i, :k + 1].cpu().numpy()
        fvs.append((nid[i, :k].cpu().numpy(), o, feat[i, :o[-1]].cpu().numpy()))
    c = dict(kf1=fr[0], kf2=fr[1], mp1=np.zeros(fr[0].n, np.uint8), mp2=np.zeros(fr[1].n, np.uint8),
             fv1=fvs[0], fv2=fvs[1], F12=F, epipole=epi, sigma2=sigma2)
    exp = TC.restated(c, True, True, False)
    assert exp[1] > 200
    assert np.array_equal(out[0, :fr[0].n], exp[0]) and nm[0] == exp[1]
    assert (out[0, fr[0].n:] == -1).all()
