"""The loop-closing matchers on the GPU, bit-exact against the restatements of
tests/loop_cases.py: SearchByProjection(pKF, Scw, ...), SearchBySim3 and SearchByBoW(pKF1, pKF2)
(host form and the batch over keyframe slots)."""
from __future__ import annotations

import numpy as np
import pytest

import loop_cases as L
import scenarios as S
from orbslam_mapsave_amd.abi import ORBFE_ERR_UNSUPPORTED, Frame, OrbfeError
from orbslam_mapsave_amd.synth import synthetic_vocabulary_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt():
    from orbslam_mapsave_amd.native import ORBmatcher
    m = ORBmatcher(0.75, True, device=0)
    yield m
    m.close()


# ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) -------------------------------------

def gpu_sbp(mt, c, **kw):
    return mt.SearchByProjectionSim3(c["kf"], c["tcw"], c["cam"], c["log_scale"], c["xyz"],
                                     c["normal"], c["min_dist"], c["max_dist"], c["desc"],
                                     th=c["th"], skip=c["skip"], mp_ids=c["ids"],
                                     kf_matched=c["matched0"], **kw)


def check_sbp(mt, c):
    exp = L.loop_sbp(c, c["th"])
    assert not exp[3]
    got, n = gpu_sbp(mt, c)
    assert n == exp[1]
    assert np.array_equal(got, exp[0])
    return exp


def test_sbp_built_case(mt):
    c = L.sbp_case(0)
    matched, n, dec, _ = check_sbp(mt, c)
    assert n >= 40
    # the point listed twice: its id sits in two slots
    got, _ = gpu_sbp(mt, c)
    ids, cnt = np.unique(got[(got >= 7000) & (got < 20000) & (c["matched0"] < 0)],
                         return_counts=True)
    assert (cnt == 2).any()
    # without ids the list index is written
    noid = dict(c, ids=None, skip=c["bad"])
    check_sbp(mt, noid)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5])
def test_sbp_few_points(mt, n):
    c = L.sbp_case(0)
    live = np.flatnonzero(L.loop_sbp(c, c["th"])[2] >= 0)[:n]
    check_sbp(mt, L.sbp_subset(c, live))


def test_sbp_empty_keyframe(mt):
    c = L.sbp_case(0)
    kf = c["kf"]
    empty = Frame(kf.keys[:0], kf.desc[:0], S.W, S.H, kf.scale_factors)
    got, n = gpu_sbp(mt, dict(c, kf=empty, matched0=np.zeros(0, np.int32)))
    assert n == 0 and len(got) == 0


def test_sbp_chain_takes_rounds(mt):
    c = L.chain_case()
    check_sbp(mt, c)
    assert mt.last_rounds() >= 3


def test_sbp_dense_case_reruns_on_the_csr_path(mt):
    c = L.sbp_dense_case(0)
    pts = L.sbp_points(c, c["th"])
    assert max(len(p["idx"]) for p in pts if p and p["reject"] is None) > 16
    before = mt.capacity_retries()
    exp = L.loop_sbp(c, c["th"], points=pts)
    got, n = gpu_sbp(mt, c)
    assert mt.capacity_retries() > before
    assert n == exp[1] >= 40 and np.array_equal(got, exp[0])


def test_sbp_all_slots_held(mt):
    c = L.sbp_case(0)
    held = np.arange(c["kf"].n, dtype=np.int32) + 40000
    got, n = gpu_sbp(mt, dict(c, matched0=held))
    assert n == 0 and np.array_equal(got, held)


def test_sbp_level_outside_pyramid(mt):
    c = L.sbp_unsupported_case(0)
    exp = L.loop_sbp(c, c["th"])
    assert exp[3]
    with pytest.raises(OrbfeError) as e:
        gpu_sbp(mt, c)
    assert e.value.status == ORBFE_ERR_UNSUPPORTED
    got, n = e.value.results
    assert n == exp[1] and np.array_equal(got, exp[0])


# ---- SearchBySim3 ------------------------------------------------------------------------------

def gpu_sim3(mt, c, search=None):
    _, _, s1, s2 = L.masks(c)
    if search is not None:
        s1, s2 = search(s1, s2)
    S12, S21 = L.sim3_mats(c["s12"], c["R12"], c["t12"])
    p1, p2 = c["pts1"], c["pts2"]
    return mt.SearchBySim3(c["kf1"], c["kf2"], c["cam1"], c["T1w"], c["T2w"], S12, S21,
                           c["log1"], c["log2"],
                           (s1, p1["xyz"], p1["min_dist"], p1["max_dist"], p1["desc"]),
                           (s2, p2["xyz"], p2["min_dist"], p2["max_dist"], p2["desc"]),
                           th=c["th"])


def check_sim3(mt, c):
    exp = L.sim3(c)
    assert not exp[4]
    m12, vn1, vn2, nf = gpu_sim3(mt, c)
    assert np.array_equal(vn1, exp[1])
    assert np.array_equal(vn2, exp[2])
    assert np.array_equal(m12, exp[0]) and nf == exp[3]
    return exp


@pytest.mark.parametrize("mixed", [False, True], ids=["same", "mixed"])
def test_sim3_built_case(mt, mixed):
    assert check_sim3(mt, L.sim3_case(0, mixed=mixed))[3] >= 40


@pytest.mark.parametrize("n1,n2", [(0, 0), (1, 1), (3, 3), (4, 4), (5, 5), (5, 0), (0, 5),
                                   (700, 5)])
def test_sim3_few_features(mt, n1, n2):
    check_sim3(mt, L.sim3_subset(L.sim3_case(0), n1, n2))


@pytest.mark.parametrize("side", [1, 2])
def test_sim3_nothing_to_search_on_one_side(mt, side):
    c = L.sim3_case(0)

    def zero(s1, s2):
        return (np.zeros_like(s1), s2) if side == 1 else (s1, np.zeros_like(s2))
    m12, vn1, vn2, nf = gpu_sim3(mt, c, zero)
    exp = L.sim3(c)
    assert nf == 0 and (m12 == -1).all()
    if side == 1:
        assert (vn1 == -1).all() and np.array_equal(vn2, exp[2])
    else:
        assert (vn2 == -1).all() and np.array_equal(vn1, exp[1])


def test_sim3_level_outside_pyramid(mt):
    c = L.sim3_unsupported_case(0)
    exp = L.sim3(c)
    assert exp[4]
    with pytest.raises(OrbfeError) as e:
        gpu_sim3(mt, c)
    assert e.value.status == ORBFE_ERR_UNSUPPORTED
    m12, vn1, vn2, nf = e.value.results
    assert np.array_equal(vn1, exp[1]) and np.array_equal(vn2, exp[2])
    assert np.array_equal(m12, exp[0]) and nf == exp[3]


def test_sim3_nan_and_inf_positions_reject_that_point_only(mt):
    c = dict(L.sim3_case(0))
    base = L.sim3(c)
    hit = np.flatnonzero(base[0] >= 0)[:6]
    xyz = c["pts1"]["xyz"].copy()
    xyz[hit[0]] = np.nan
    xyz[hit[1], 2] = np.nan
    xyz[hit[2]] = np.inf
    xyz[hit[3], 0] = -np.inf
    xyz[hit[4], 2] = np.inf
    xyz[hit[5], 2] = -np.inf
    c["pts1"] = dict(c["pts1"], xyz=xyz)
    exp = check_sim3(mt, c)
    assert (exp[1][hit] == -1).all()
    others = np.setdiff1d(np.arange(len(xyz)), hit)
    assert np.array_equal(exp[1][others], base[1][others]) and np.array_equal(exp[2], base[2])


# ---- SearchByBoW(pKF1, pKF2) -------------------------------------------------------------------

def gpu_bow(m, c):
    return m.SearchByBoWKeyFrames(*L.bow_item(c, 1), *L.bow_item(c, 2))


@pytest.fixture(scope="module")
def mts():
    from orbslam_mapsave_amd.native import ORBmatcher
    ms = {ori: ORBmatcher(0.75, ori, device=0) for ori in (True, False)}
    yield ms
    for m in ms.values():
        m.close()


@pytest.mark.parametrize("ori", [True, False])
def test_bow_built_case(mts, ori):
    c = L.bow_case(0)
    exp = L.bow_kk(c, 0.75, ori)
    got, n = gpu_bow(mts[ori], c)
    assert n == exp[1] >= 40 and np.array_equal(got, exp[0])


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("ny", [63, 64, 65, 256])
def test_bow_node_seams(mts, ori, ny):
    c = L.bow_seam_case(ny)
    exp = L.bow_kk(c, 0.75, ori)
    got, n = gpu_bow(mts[ori], c)
    assert n == exp[1] and np.array_equal(got, exp[0])


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("k", [0, 1, 3, 4, 5])
def test_bow_few_nodes(mts, ori, k):
    """KF1's FeatureVector cut to its first k nodes (a workgroup serves four)."""
    c = dict(L.bow_case(0))
    ids, off, feat = c["fv1"]
    c["fv1"] = (ids[:k], off[:k + 1], feat[:off[k]])
    exp = L.bow_kk(c, 0.75, ori)
    got, n = gpu_bow(mts[ori], c)
    assert n == exp[1] and np.array_equal(got, exp[0])
    assert k == 0 or (exp[0] >= 0).any()


def test_bow_node_over_the_limit(mts):
    c = L.bow_seam_case(257)
    with pytest.raises(OrbfeError) as e:
        gpu_bow(mts[True], c)
    assert e.value.status == ORBFE_ERR_UNSUPPORTED


def test_bow_rotation_bin_beyond_the_histogram(mts):
    """An angle difference of 1000 lands in bin 33, past rotHist: the call
    returns ORBFE_ERR_UNSUPPORTED, that match is dropped and every other result stands."""
    c = dict(L.bow_seam_case(64))
    base = L.bow_kk(c, 0.75, True)
    victim = int(np.flatnonzero(base[0] >= 0)[0])
    c["angle1"] = c["angle1"].copy()
    c["angle1"][victim] = 1000.0
    exp = L.bow_kk(c, 0.75, True)
    assert exp[0][victim] == -1 and exp[1] == base[1] - 1
    with pytest.raises(OrbfeError) as e:
        gpu_bow(mts[True], c)
    assert e.value.status == ORBFE_ERR_UNSUPPORTED
    got, n = e.value.results
    assert n == exp[1] and np.array_equal(got, exp[0])
    got, n = gpu_bow(mts[False], c)                      # no histogram without the filter
    assert n == base[1] and np.array_equal(got, base[0])


@pytest.mark.parametrize("side", [1, 2])
def test_bow_empty_keyframe(mts, side):
    c = dict(L.bow_case(0))
    c["desc%d" % side] = np.zeros((0, 32), np.uint8)
    c["angle%d" % side] = np.zeros(0, np.float32)
    c["ok%d" % side] = np.zeros(0, np.uint8)
    c["fv%d" % side] = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    got, n = gpu_bow(mts[True], c)
    assert n == 0 and (got == -1).all() and len(got) == len(c["desc1"])


def pack_slots(items, cap):
    """(desc, angle, ok, fv) per slot -> arrays in orbfe_bow_transform_batch_device's layout."""
    n = len(items)
    desc = np.zeros((n, cap, 32), np.uint8)
    ang = np.zeros((n, cap), np.float32)
    ok = np.zeros((n, cap), np.uint8)
    nn = np.zeros(n, np.int32)
    nid = np.zeros((n, cap), np.int32)
    off = np.zeros((n, cap + 1), np.int32)
    feat = np.zeros((n, cap), np.int32)
    for s, (d, a, o, (ids, noff, fe)) in enumerate(items):
        desc[s, :len(d)] = d
        ang[s, :len(a)] = a
        ok[s, :len(o)] = o
        nn[s] = len(ids)
        nid[s, :len(ids)] = ids
        off[s, :len(noff)] = noff
        feat[s, :len(fe)] = fe
    return desc, ang, ok, nn, nid, off, feat


def run_batch(m, dev_slots, pairs, cap):
    import torch
    dev = torch.device("cuda", 0)
    p1 = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=dev)
    p2 = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=dev)
    P = len(pairs)
    out = torch.full((P, cap), 7, dtype=torch.int32, device=dev)
    nm = torch.full((P,), 9, dtype=torch.int32, device=dev)
    st = torch.full((1,), 9, dtype=torch.int32, device=dev)
    m.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        desc, ang, ok, nn, nid, off, feat = dev_slots
        m.search_by_bow_keyframes_batch_device(
            P, p1.data_ptr(), p2.data_ptr(), cap, desc.data_ptr(), ang.data_ptr(), ok.data_ptr(),
            nn.data_ptr(), nid.data_ptr(), off.data_ptr(), feat.data_ptr(), out.data_ptr(),
            nm.data_ptr(), st.data_ptr())
        torch.cuda.synchronize()
    finally:
        m.set_stream(None)
    return out.cpu().numpy(), nm.cpu().numpy(), int(st[0])


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("npairs", [1, 2, 5])
def test_bow_batch_equals_host_form(mts, ori, npairs):
    """ComputeSim3's candidate loop: the current keyframe (slot 0) against every candidate."""
    import torch
    c = L.bow_case(0)
    kf1 = L.bow_item(c, 1)
    empty = (np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.uint8),
             (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32)))
    cands = [L.bow_item(c, 2), L.bow_item(L.bow_case(1), 2), empty,
             L.bow_item(L.bow_seam_case(65), 2), L.bow_item(c, 1)][:npairs]
    items = [kf1] + cands
    cap = 300
    assert max(len(it[0]) for it in items) <= cap
    dev = torch.device("cuda", 0)
    slots = [torch.from_numpy(x).to(dev) for x in pack_slots(items, cap)]
    pairs = [(0, 1 + k) for k in range(npairs)]
    got, gnm, st = run_batch(mts[ori], slots, pairs, cap)
    assert st == 0
    n1 = len(kf1[0])
    for p, cand in enumerate(cands):
        pc = dict(desc1=kf1[0], angle1=kf1[1], ok1=kf1[2], fv1=kf1[3],
                  desc2=cand[0], angle2=cand[1], ok2=cand[2], fv2=cand[3])
        exp = L.bow_kk(pc, 0.75, ori)
        host = mts[ori].SearchByBoWKeyFrames(*kf1, *cand)
        assert gnm[p] == exp[1] == host[1], p
        assert np.array_equal(got[p, :n1], exp[0]) and np.array_equal(host[0], exp[0]), p
        assert (got[p, n1:] == -1).all()
    assert gnm[0] >= 40


def test_bow_batch_from_the_device_transform(mts, tmp_path):
    """Keyframe slots written by orbfe_bow_transform_batch_device go straight into the batch."""
    import torch
    from orbslam_mapsave_amd.native import Vocabulary
    frames = [S.extract_frame(0, 600, ini=20), S.extract_frame(0, 600, shift=(2, -3), ini=20),
              S.extract_frame(1, 600, ini=20)]
    path = str(tmp_path / "voc.txt")
    synthetic_vocabulary_text(path, 10, 4, seed=0, scoring=0, weighting=0,
                              anchors=frames[0].desc[::37])
    gv = Vocabulary(path, device=0)
    cap = 700
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(17))
    d = np.zeros((3, cap, 32), np.uint8)
    ang = np.zeros((3, cap), np.float32)
    ok = np.zeros((3, cap), np.uint8)
    for i, f in enumerate(frames):
        d[i, :f.n] = f.desc
        ang[i, :f.n] = f.keys["angle"]
        ok[i, :f.n] = rng.uniform(size=f.n) < 0.85
    D, A, OK = (torch.from_numpy(x).to(dev) for x in (d, ang, ok))
    N = torch.tensor([f.n for f in frames], dtype=torch.int32, device=dev)
    wid = torch.zeros((3, cap), dtype=torch.int32, device=dev)
    val = torch.zeros((3, cap), dtype=torch.float64, device=dev)
    nid = torch.zeros((3, cap), dtype=torch.int32, device=dev)
    off = torch.zeros((3, cap + 1), dtype=torch.int32, device=dev)
    feat = torch.zeros((3, cap), dtype=torch.int32, device=dev)
    nw = torch.zeros(3, dtype=torch.int32, device=dev)
    nn = torch.zeros(3, dtype=torch.int32, device=dev)
    gv.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    gv.transform_batch_device(3, D.data_ptr(), N.data_ptr(), cap, 2, wid.data_ptr(),
                              val.data_ptr(), nw.data_ptr(), nid.data_ptr(), off.data_ptr(),
                              feat.data_ptr(), nn.data_ptr())
    pairs = [(0, 1), (0, 2), (1, 0)]
    got, gnm, st = run_batch(mts[True], (D, A, OK, nn, nid, off, feat), pairs, cap)
    gv.close()
    assert st == 0
    fvs = []
    for i in range(3):
        k = int(nn[i])
        o = off[i, :k + 1].cpu().numpy()
        fvs.append((nid[i, :k].cpu().numpy(), o, feat[i, :o[-1]].cpu().numpy()))
    for p, (a, b) in enumerate(pairs):
        fa, fb = frames[a], frames[b]
        pc = dict(desc1=fa.desc, angle1=ang[a, :fa.n], ok1=ok[a, :fa.n], fv1=fvs[a],
                  desc2=fb.desc, angle2=ang[b, :fb.n], ok2=ok[b, :fb.n], fv2=fvs[b])
        exp = L.bow_kk(pc, 0.75, True)
        assert gnm[p] == exp[1], p
        assert np.array_equal(got[p, :fa.n], exp[0]) and (got[p, fa.n:] == -1).all(), p
    assert gnm[0] >= 40
