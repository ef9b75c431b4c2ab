"""ORBmatcher::Fuse, both overloads (ORBmatcher.cc:828-978, 980-1103), as a batched device
search plus an ordered host walk.

CPU: the restatement in fuse_cases.py against oracle.is_in_frustum where the two compute the same
quantities, the scenario's coverage of every branch, and the decomposition claim -- batched
search + ordered walk with a live skip test == the sequential loop -- on a model of the map.
GPU: orbfe_fuse_search / orbfe_fuse_search_batch_device bit-exact on best_idx, best_dist and
n_found against the restatement.

Scenario figures (fuse_case, restatement): seed 0 has 1,305 points, seed 1 1,309; SE3 th 3
matches 398 / 371 of them (376 / 348 distinct keypoints), Sim3 th 4 606 / 592 (592 / 574); every
rejection branch (skip, depth, image, distance, angle) takes at least 41 points and chi-square
drops 404 / 441 candidates.
"""
import functools

import numpy as np
import pytest

import fuse_cases as FC
import oracle
import scenarios as S
from orbslam_mapsave_amd.abi import ORBFE_ERR_ARG, ORBFE_ERR_UNSUPPORTED, Frame, OrbfeError

F32 = np.float32
SE3, SIM3 = FC.SE3, FC.SIM3
CASES = [(0, 3.0, SE3), (1, 3.0, SE3), (0, 4.0, SIM3), (1, 4.0, SIM3)]


@functools.lru_cache(maxsize=None)
def case(seed, stereo=True):
    return FC.fuse_case(seed, stereo)


@functools.lru_cache(maxsize=None)
def expected(seed, th, mode, stereo=True, use_skip=True):
    stats = {}
    r = FC.restated(case(seed, stereo), th, mode, use_skip, stats)
    return r, stats


# ---- CPU ---------------------------------------------------------------------------------------

def test_projection_block_vs_oracle_frustum():
    """pc, dist3D, the viewing dot product and the predicted level are the quantities Fuse and
    Frame::isInFrustum compute alike: for every point the oracle has in view the restatement's
    level is the oracle's and (float)(dot / dist3D) is its mTrackViewCos; u, v differ only by the
    order of the products (fx * (x * invz) against fx * x * invz: a few ulp of 640)."""
    fc = S.frustum_case(0)
    inv, px, py, pxr, pl, vc = oracle.is_in_frustum(**fc)
    empty = Frame(np.zeros(0, S.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), S.W, S.H, FC.SCALE)
    c = dict(kf=empty, tcw=fc["tcw"], cam=fc["cam"], log_scale=fc["log_scale"], xyz=fc["xyz"],
             normal=fc["normal"], min_dist=fc["min_dist"], max_dist=fc["max_dist"])
    seen = 0
    for i in np.flatnonzero(inv):
        p = FC.project(c, int(i))
        if p["reject"] == "image":   # strict upper bound / product order, on the border only
            assert abs(float(p["u"]) - px[i]) < 1e-3 and abs(float(p["v"]) - py[i]) < 1e-3
            continue
        assert p["reject"] is None, (i, p)
        assert p["lvl"] == pl[i]
        assert F32(p["dot"] / float(p["dist"])) == vc[i]
        assert abs(float(p["u"]) - px[i]) < 1e-3 and abs(float(p["v"]) - py[i]) < 1e-3
        assert abs(float(p["ur"]) - pxr[i]) < 1e-3
        seen += 1
    assert seen > 1000


@pytest.mark.parametrize("seed,th,mode", CASES)
def test_scenario_reaches_every_branch(seed, th, mode):
    (bi, bd, nf, bad), stats = expected(seed, th, mode)
    print(seed, th, mode, len(bi), nf, len(set(bi[bi >= 0].tolist())), stats)
    assert not bad
    assert nf > 100
    assert len(set(bi[bi >= 0].tolist())) < nf  # points share a keypoint: the occupied branch
    for k in ("skip", "depth", "image", "distance", "angle"):
        assert stats.get(k, 0) >= 37, (k, stats)
    if mode == SE3:
        assert stats.get("chi2", 0) > 400
    assert ((bd > FC.TH_LOW) & (bd < 256)).any()  # a winner above TH_LOW: no match


@pytest.mark.parametrize("seed,th,mode", [(0, 3.0, SE3), (1, 4.0, SIM3)])
def test_walk_equals_sequential_loop_model(seed, th, mode):
    """Batched search + ordered walk == the sequential loop, with the restatement as the search:
    the list repeats points, so an entry's skip test changes during the walk."""
    c, pid = FC.walk_case(seed)
    ow = FC.camera_center(c["tcw"].astype(F32))
    seq = FC.MapModel(c["kf"].n, pid, seed)
    n_seq = FC.sequential(seq, lambda i: FC.search_point(c, i, th, mode, ow)[0], mode)
    dec = FC.MapModel(c["kf"].n, pid, seed)
    c2 = dict(c, skip=dec.static_skip())
    bi, _, _, _ = FC.restated(c2, th, mode)
    n_dec = FC.walk(dec, bi, mode)
    assert n_seq == n_dec > 30
    assert seq.result() == dec.result() and seq.calls == dec.calls
    assert any(k == "O" for k, _, _ in dec.calls) and any(k == "E" for k, _, _ in dec.calls)
    # the live skip test matters: a static one fuses the repeated entries twice
    stat = FC.MapModel(c["kf"].n, pid, seed)
    sk = stat.static_skip()
    n_stat = sum(1 for i in range(len(pid)) if not sk[i] and bi[i] >= 0)
    assert n_stat > n_dec


def test_null_and_bad_arguments():
    import ctypes as C
    from orbslam_mapsave_amd import native
    lib = native.lib()
    assert lib.orbfe_fuse_search(None, None, None, None, C.c_float(0), None, 0, None, None, None,
                                 None, None, None, C.c_float(3), 0, None, None,
                                 None) == ORBFE_ERR_ARG
    assert lib.orbfe_fuse_search_batch_device(
        None, -1, None, C.c_size_t(0), None, C.c_size_t(0), None, 0, None, None, None,
        C.c_float(0), C.c_float(0), C.c_float(0), C.c_float(0), None, None, 0, C.c_float(0), -1,
        None, None, None, None, None, None, C.c_float(3), 0, None, None, None) == ORBFE_ERR_ARG


# ---- GPU ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mt():
    from orbslam_mapsave_amd.native import ORBmatcher
    m = ORBmatcher(0.9, True, device=0)
    yield m
    m.close()


def gpu_search(mt, c, th, mode, skip=True):
    return mt.FuseSearch(c["kf"], c["tcw"], c["cam"], c["log_scale"], c["inv_sigma2"], c["xyz"],
                         c["normal"], c["min_dist"], c["max_dist"], c["desc"], th, mode,
                         skip=c["skip"] if skip else None)


def check(got, exp):
    bi, bd, nf = got
    ebi, ebd, enf = exp[:3]
    assert nf == enf
    assert np.array_equal(bi, ebi), np.flatnonzero(bi != ebi)[:10]
    assert np.array_equal(bd, ebd), np.flatnonzero(bd != ebd)[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,th,mode", CASES)
def test_gpu_fuse_search(mt, seed, th, mode):
    (exp, _) = expected(seed, th, mode)
    assert exp[2] > 100 and len(set(exp[0][exp[0] >= 0].tolist())) < exp[2]
    check(gpu_search(mt, case(seed), th, mode), exp)


@pytest.mark.gpu
def test_gpu_fuse_search_monocular(mt):
    (exp, stats) = expected(0, 3.0, SE3, stereo=False)
    assert exp[2] > 100 and stats["chi2"] > 0  # the 5.99 branch drops 44 candidates
    check(gpu_search(mt, case(0, stereo=False), 3.0, SE3), exp)


@pytest.mark.gpu
def test_gpu_fuse_search_skip_null(mt):
    (exp, _) = expected(1, 3.0, SE3, use_skip=False)
    assert exp[2] > expected(1, 3.0, SE3)[0][2]
    check(gpu_search(mt, case(1), 3.0, SE3, skip=False), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("n_mp", [0, 1, 63, 64, 65])
def test_gpu_fuse_search_point_counts(mt, n_mp):
    (ebi, ebd, _, _), _ = expected(0, 3.0, SE3)
    first = int(np.flatnonzero(ebi >= 0)[0])  # start at a point that matches
    idx = np.arange(first, first + n_mp)
    bi, bd, nf = gpu_search(mt, FC.subset(case(0), idx), 3.0, SE3)
    assert np.array_equal(bi, ebi[idx]) and np.array_equal(bd, ebd[idx])
    assert nf == int((ebi[idx] >= 0).sum()) and (n_mp == 0 or nf >= 1)


@pytest.mark.gpu
def test_gpu_fuse_search_empty_keyframe(mt):
    c = case(0)
    kf = Frame(np.zeros(0, S.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), S.W, S.H, FC.SCALE,
               np.zeros(0, F32))
    bi, bd, nf = gpu_search(mt, dict(c, kf=kf), 3.0, SE3)
    assert nf == 0 and (bi == -1).all() and (bd == 256).all()


GRID_BLOCK = 1024             # grid_kernel's workgroup: thread t holds keypoints t + 1024 j
GRID_LDS_MAX = 8 * GRID_BLOCK  # keypoints whose items list grid_kernel orders in LDS


@functools.lru_cache(maxsize=None)
def big_case(copies):
    """A keyframe of `copies` frames' keypoints, the first of them the scenario's own keyframe and
    the others shifted copies.  Five (5,035 keypoints): the grid kernel's LDS form with five of
    a thread's register slots in use; ten (10,070): past the 8,192 it orders in LDS, the
    in-place form."""
    frames = [S.extract_frame(0, 1000, u_right=True)] + [
        S.extract_frame(0, 1000, shift=(s, 2 * s), u_right=True) for s in range(1, copies)]
    kf = Frame(np.concatenate([f.keys for f in frames]), np.concatenate([f.desc for f in frames]),
               S.W, S.H, FC.SCALE, np.concatenate([f.u_right for f in frames]))
    if copies == 10:
        assert kf.n > GRID_LDS_MAX
    else:
        assert 4 * GRID_BLOCK < kf.n <= GRID_LDS_MAX
    return FC.subset(FC.fuse_case(0, kf=kf), slice(0, 500))


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [5, 10])
@pytest.mark.parametrize("th,mode", [(3.0, SE3), (4.0, SIM3)])
def test_gpu_fuse_search_keyframe_past_lds_grid(mt, th, mode, copies):
    c = big_case(copies)
    exp = FC.restated(c, th, mode)
    assert exp[2] > 100
    check(gpu_search(mt, c, th, mode), exp)


def level_case():
    """Two points of the scenario moved out of the pyramid: mfMaxDistance set so that
    MapPoint::PredictScale gives -1 (dist3D within a few ulp of 1.2 mfMaxDistance, still inside
    the distance test) and nlevels (mfMaxDistance = 1.2^7.5 dist3D, mfMinDistance lowered)."""
    c = dict(case(0))
    for k in ("min_dist", "max_dist", "skip", "normal"):
        c[k] = c[k].copy()
    (ebi, _, _, _), _ = expected(0, 3.0, SE3)
    lo, hi = (int(i) for i in np.flatnonzero(ebi >= 0)[:2])
    d_lo, d_hi = FC.project(c, lo)["dist"], FC.project(c, hi)["dist"]
    found = False
    cand = F32(d_lo / F32(1.2))
    for _ in range(16):
        cand = np.nextafter(cand, F32(0))
    for _ in range(32):
        c["max_dist"][lo] = cand
        c["min_dist"][lo] = cand / FC.SCALE[7]
        p = FC.project(c, lo)
        if p["reject"] is None and p["lvl"] == -1:
            found = True
            break
        cand = np.nextafter(cand, F32(np.inf))
    assert found, "no mfMaxDistance puts the predicted level at -1"
    c["max_dist"][hi] = F32(float(d_hi) * 1.2 ** 7.5)
    c["min_dist"][hi] = F32(float(d_hi) * 0.5)
    assert FC.project(c, hi)["reject"] is None and FC.project(c, hi)["lvl"] == 8
    c["skip"][[lo, hi]] = 0
    return c, lo, hi


def test_level_case_leaves_the_pyramid():
    c, lo, hi = level_case()
    bi, bd, nf, bad = FC.restated(c, 3.0, SE3)
    assert bad and bi[lo] == -1 and bi[hi] == -1 and bd[lo] == 256 and bd[hi] == 256


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [SE3, SIM3])
def test_gpu_fuse_search_level_out_of_range(mt, mode):
    c, lo, hi = level_case()
    exp = FC.restated(c, 3.0, mode)
    assert exp[3] and exp[2] > 100
    with pytest.raises(OrbfeError) as e:
        gpu_search(mt, c, 3.0, mode)
    assert e.value.status == ORBFE_ERR_UNSUPPORTED
    check(e.value.results, exp)
    # the same matcher afterwards: the status does not stick
    check(gpu_search(mt, case(0), 3.0, mode), FC.restated(case(0), 3.0, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,th,stereo", [(SE3, 3.0, True), (SIM3, 4.0, True),
                                             (SE3, 3.0, False)])
def test_gpu_fuse_search_batch_device(mt, mode, th, stereo):
    """Three keyframes with different keypoint counts and poses in slabs with non-tight pitches,
    a per-pair skip matrix: each keyframe's row equals the host form's result for it alone."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.Generator(np.random.PCG64(5))
    c = FC.subset(case(0), slice(0, 700))
    n_mp = len(c["xyz"])
    full = c["kf"]
    counts = [full.n, 0, full.n - 137]
    kfs = [Frame(full.keys[:n], full.desc[:n], S.W, S.H, FC.SCALE, full.u_right[:n])
           for n in counts]
    poses = [c["tcw"], S.pose(rng, 0.002, 0.01), S.pose(rng, 0.003, 0.02)]
    skips = (rng.uniform(size=(3, n_mp)) < 0.15).astype(np.uint8)
    n_kf, kp_cap = 3, full.n + 9
    keys_pitch, desc_pitch = kp_cap + 5, (kp_cap + 3) * 32 + 16
    keys = np.zeros((n_kf, keys_pitch), S.KEYPOINT_DTYPE)
    desc = np.full((n_kf, desc_pitch), 0xAB, np.uint8)
    ur = np.full((n_kf, kp_cap), 7.0, F32)
    for k, f in enumerate(kfs):
        keys[k, :f.n] = f.keys
        desc[k, :f.n * 32] = f.desc.reshape(-1)
        ur[k, :f.n] = f.u_right
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    d_keys, d_desc, d_ur = up(keys), up(desc), up(ur)
    d_n = up(np.array(counts, np.int32))
    d_xyz, d_nrm = up(c["xyz"]), up(c["normal"])
    d_min, d_max, d_md = up(c["min_dist"]), up(c["max_dist"]), up(c["desc"])
    d_skip = up(skips)
    d_bi = torch.full((n_kf * n_mp,), -7, dtype=torch.int32, device=dev)
    d_bd = torch.full((n_kf * n_mp,), -7, dtype=torch.int32, device=dev)
    d_st = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    mt.fuse_search_batch_device(
        n_kf, d_keys.data_ptr(), keys_pitch, d_desc.data_ptr(), desc_pitch,
        d_ur.data_ptr() if stereo else None, kp_cap, d_n.data_ptr(), np.stack(poses), c["cam"],
        (0.0, float(S.W), 0.0, float(S.H)), FC.SCALE, c["inv_sigma2"], c["log_scale"], n_mp,
        d_xyz.data_ptr(), d_nrm.data_ptr(), d_min.data_ptr(), d_max.data_ptr(), d_md.data_ptr(),
        d_skip.data_ptr(), th, mode, d_bi.data_ptr(), d_bd.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    bi = d_bi.cpu().numpy().reshape(n_kf, n_mp)
    bd = d_bd.cpu().numpy().reshape(n_kf, n_mp)
    assert int(d_st.cpu()[0]) == 0
    total = 0
    for k, f in enumerate(kfs):
        if not stereo:
            f = Frame(f.keys, f.desc, S.W, S.H, FC.SCALE)
        hbi, hbd, hnf = gpu_search(mt, dict(c, kf=f, tcw=poses[k], skip=skips[k]), th, mode)
        assert np.array_equal(bi[k], hbi) and np.array_equal(bd[k], hbd), k
        total += hnf
    assert total > 100 and (bi[1] == -1).all() and (bd[1] == 256).all()
    # keyframe 0 of the batch is the scenario's keyframe and pose: the restatement's answer too
    e = FC.restated(dict(c, skip=skips[0], kf=kfs[0] if stereo else Frame(
        full.keys, full.desc, S.W, S.H, FC.SCALE)), th, mode)
    assert np.array_equal(bi[0], e[0]) and np.array_equal(bd[0], e[1])


@pytest.mark.gpu
@pytest.mark.parametrize("seed,th,mode", [(0, 3.0, SE3), (1, 4.0, SIM3)])
def test_gpu_walk_equals_sequential_loop(mt, seed, th, mode):
    """The fully sequential reference loop (search and apply interleaved, restatement) against
    the device search + ordered walk: final slots, replaced / added lists, nFused."""
    c, pid = FC.walk_case(seed)
    ow = FC.camera_center(c["tcw"].astype(F32))
    seq = FC.MapModel(c["kf"].n, pid, seed)
    n_seq = FC.sequential(seq, lambda i: FC.search_point(c, i, th, mode, ow)[0], mode)
    dec = FC.MapModel(c["kf"].n, pid, seed)
    bi, _, _ = gpu_search(mt, dict(c, skip=dec.static_skip()), th, mode)
    n_dec = FC.walk(dec, bi, mode)
    assert n_seq == n_dec > 30
    assert seq.result() == dec.result() and seq.calls == dec.calls


# ---- the batch form's seams: 40 keyframes per launch, d_best_dist NULL, the in-place grid fill ----

def run_batch(mt, c, kfs, poses, skips, th, mode, with_dist=True, stereo=True):
    """orbfe_fuse_search_batch_device over the keyframes `kfs` (slabs with non-tight pitches) ->
    (best_idx, best_dist or None, status), one row per keyframe."""
    import torch
    dev = torch.device("cuda", 0)
    n_kf, n_mp = len(kfs), len(c["xyz"])
    kp_cap = max(f.n for f in kfs) + 3
    keys_pitch, desc_pitch = kp_cap + 2, (kp_cap + 1) * 32 + 16
    keys = np.zeros((n_kf, keys_pitch), S.KEYPOINT_DTYPE)
    desc = np.full((n_kf, desc_pitch), 0xAB, np.uint8)
    ur = np.full((n_kf, kp_cap), 7.0, F32)
    for k, f in enumerate(kfs):
        keys[k, :f.n] = f.keys
        desc[k, :f.n * 32] = f.desc.reshape(-1)
        ur[k, :f.n] = f.u_right
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    d_keys, d_desc, d_ur = up(keys), up(desc), up(ur)
    d_n = up(np.array([f.n for f in kfs], np.int32))
    d_xyz, d_nrm = up(c["xyz"]), up(c["normal"])
    d_min, d_max, d_md = up(c["min_dist"]), up(c["max_dist"]), up(c["desc"])
    d_skip = up(skips)
    d_bi = torch.full((n_kf * n_mp,), -7, dtype=torch.int32, device=dev)
    d_bd = torch.full((n_kf * n_mp,), -7, dtype=torch.int32, device=dev)
    d_st = torch.full((1,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    mt.fuse_search_batch_device(
        n_kf, d_keys.data_ptr(), keys_pitch, d_desc.data_ptr(), desc_pitch,
        d_ur.data_ptr() if stereo else None, kp_cap, d_n.data_ptr(), np.stack(poses), c["cam"],
        (0.0, float(S.W), 0.0, float(S.H)), FC.SCALE, c["inv_sigma2"], c["log_scale"], n_mp,
        d_xyz.data_ptr(), d_nrm.data_ptr(), d_min.data_ptr(), d_max.data_ptr(), d_md.data_ptr(),
        d_skip.data_ptr(), th, mode, d_bi.data_ptr(), d_bd.data_ptr() if with_dist else None,
        d_st.data_ptr())
    torch.cuda.synchronize()
    bd = d_bd.cpu().numpy().reshape(n_kf, n_mp)
    assert with_dist or (bd == -7).all()
    return d_bi.cpu().numpy().reshape(n_kf, n_mp), bd if with_dist else None, int(d_st.cpu()[0])


@functools.lru_cache(maxsize=None)
def seam_case():
    """200 points of the scenario, the ones that match one of its keyframe's first 150 keypoints
    first, and that keyframe cut to 300 keypoints: every prefix of 150-300 of them is a cheap
    keyframe with matches."""
    c = case(0)
    (ebi, _, _, _), _ = expected(0, 3.0, SE3)
    near = np.flatnonzero((ebi >= 0) & (ebi < 150))
    rest = np.setdiff1d(np.arange(len(ebi)), near)
    idx = np.sort(np.concatenate([near, rest])[:200])
    assert len(near) >= 20
    return FC.subset(c, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,mode,th", [(40, SE3, 3.0), (41, SIM3, 4.0), (81, SE3, 3.0)])
def test_gpu_fuse_search_batch_launch_seams(mt, n_kf, mode, th):
    """The search kernel takes 40 keyframes' poses per launch as arguments and indexes them by
    blockIdx.y, everything else by kf0 + blockIdx.y: keyframes 0, 39, 40, 41 and 80 -- distinct
    poses, keypoint counts and skip rows, each with matches -- equal the host form's result for
    that keyframe alone, keyframes 0 and 40 the restatement's too.  d_best_dist = NULL leaves
    best_idx unchanged."""
    c = seam_case()
    n_mp = len(c["xyz"])
    full = c["kf"]
    rng = np.random.Generator(np.random.PCG64(40 + n_kf))
    counts = [150 + (37 * k) % 151 for k in range(n_kf)]
    kfs = [Frame(full.keys[:n], full.desc[:n], S.W, S.H, FC.SCALE, full.u_right[:n]) for n in counts]
    poses = [c["tcw"]] + [S.pose(rng, 0.001 + 0.0002 * (k % 5), 0.004) for k in range(1, n_kf)]
    skips = (rng.uniform(size=(n_kf, n_mp)) < 0.15).astype(np.uint8)
    bi, bd, st = run_batch(mt, c, kfs, poses, skips, th, mode)
    assert st == 0
    seam = [k for k in (0, 39, 40, 41, 80) if k < n_kf]
    for a in seam:
        for b in seam:
            assert a == b or not np.array_equal(poses[a], poses[b])
    for k in seam:
        hbi, hbd, hnf = gpu_search(mt, dict(c, kf=kfs[k], tcw=poses[k], skip=skips[k]), th, mode)
        assert hnf > 0, k
        assert np.array_equal(bi[k], hbi) and np.array_equal(bd[k], hbd), k
    for k in (0, 40):
        if k < n_kf:
            e = FC.restated(dict(c, kf=kfs[k], tcw=poses[k], skip=skips[k]), th, mode)
            assert e[2] > 0 and np.array_equal(bi[k], e[0]) and np.array_equal(bd[k], e[1]), k
    bi2, _, st2 = run_batch(mt, c, kfs, poses, skips, th, mode, with_dist=False)
    assert st2 == 0 and np.array_equal(bi2, bi)


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [5, 10])
@pytest.mark.parametrize("th,mode", [(3.0, SE3), (4.0, SIM3)])
def test_gpu_fuse_search_batch_big_keyframe_second(mt, th, mode, copies):
    """A batch whose keyframe 1 is a big one, between two small keyframes: its grid lands at
    keyframe 1's offset of the batch's item slab, copied out of LDS (five copies) or, with more
    than 8,192 keypoints (ten), filled in place there."""
    c = FC.subset(big_case(copies), slice(0, 200))
    big = c["kf"]
    small = case(0)["kf"]
    kfs = [Frame(small.keys[:n], small.desc[:n], S.W, S.H, FC.SCALE, small.u_right[:n])
           for n in (300, 211)]
    kfs.insert(1, big)
    assert (kfs[1].n > GRID_LDS_MAX) == (copies == 10)
    rng = np.random.Generator(np.random.PCG64(11))
    poses = [S.pose(rng, 0.001, 0.004), c["tcw"], S.pose(rng, 0.002, 0.004)]
    skips = (rng.uniform(size=(3, len(c["xyz"]))) < 0.1).astype(np.uint8)
    bi, bd, st = run_batch(mt, c, kfs, poses, skips, th, mode)
    assert st == 0
    for k in range(3):
        hbi, hbd, hnf = gpu_search(mt, dict(c, kf=kfs[k], tcw=poses[k], skip=skips[k]), th, mode)
        assert hnf > (30 if k == 1 else 0), k
        assert np.array_equal(bi[k], hbi) and np.array_equal(bd[k], hbd), k
