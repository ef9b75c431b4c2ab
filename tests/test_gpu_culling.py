"""The culling calls on the device (orbfe_map_cull_points and its companions, native.LocalMap)
against the restatement of tests/culling_cases.py: after every culling operation of every script
the whole state (every keyframe's mvpMapPoints and bad flag; every point's bad flag, observation
row with its indices, nObs, found, visible, first id) is read back through the getters and
compared exactly, with the operation's own output; on the built cases, on seeded walks and at the
shapes where a kernel can break; the batch forms against the same sequence of single calls on a
second handle; the error contract; and a chain into the calls that existed before."""
import ctypes as C

import numpy as np
import pytest

import culling_cases as Q
from orbslam_mapsave_amd import abi, native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    m = native.LocalMap(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def lm2():
    m = native.LocalMap(0)
    yield m
    m.close()


def check(m, script, batch="batch", want=None):
    m.clear()
    want = Q.run_script(script) if want is None else want
    got = Q.LibraryRunner(m, batch).run(script)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w and isinstance(w, tuple) and len(w) == 2 and isinstance(w[1], tuple):
            assert g[0] == w[0], (i, g[0], w[0])
            for part in (0, 1, 2):
                bad = sorted(n for n in w[1][part] if g[1][part].get(n) != w[1][part][n])[:4]
                assert not bad, (i, part, [(n, g[1][part].get(n), w[1][part][n]) for n in bad])
        assert g == w, i
    return want


def both(lm, lm2, script):
    want = check(lm, script, "batch")
    check(lm2, script, "single", want)
    return want


@pytest.mark.parametrize("case", sorted(Q.CASES))
def test_built_cases(lm, lm2, case):
    for v in Q.VARIANTS:
        both(lm, lm2, Q.CASES[case](v))


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_seeded_walks(lm, lm2, seed):
    both(lm, lm2, Q.seeded_script(seed))


def test_observation_rows(lm):
    """Observation rows of 0, 1, 2, 3, 4, 63, 64, 65 and 200 observers (a wave's stride and its
    tail), set bad in one call and culled in one call."""
    want = check(lm, Q.script_observation_rows())
    assert len(want[-1][0][1]) == 9


def test_keyframe_slots(lm):
    """Keyframes of 0, 1, 63, 64, 65, 1,024, 1,025 and 8,192 slots: features, TrackedMapPoints at
    min_obs 0, 1, 2 and 4, SetBadFlag of the point at the last slot."""
    want = check(lm, Q.script_keyframe_slots())
    assert want[-1][0] > 5000


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_cull_lists(lm, n):
    """MapPointCulling over lists of every size around a wave, the workgroup's 1,024 and beyond it,
    with points that repeat."""
    check(lm, Q.script_cull_list(n, n % 2))


def test_tracked_map_points_min_obs(lm):
    s = Q.case_counters(0)
    kf = [op[1] for op in s if op[0] == "kf"][0]
    cut = [i for i, op in enumerate(s) if op[0] == "tracked"][0]
    want = check(lm, s[:cut] + [("tracked", kf, mo) for mo in (0, 1, 2, 3, 4)])
    assert len({w[0] for w in want[-5:]}) >= 3


def test_increase_counters_device(lm, lm2):
    """The device form (a device array of point slots with -1 entries and repeats, with and without
    a byte mask) against the host form on a second handle and against the restatement; an entry out
    of range is refused on the device with nothing added."""
    import torch
    s = Q.case_counters(1)
    cut = [i for i, op in enumerate(s) if op[0] == "inc"][0]
    lm.clear()
    lm2.clear()
    m = Q.Model()
    r, r2 = Q.LibraryRunner(lm), Q.LibraryRunner(lm2)
    for op in s[:cut]:
        m.run(op)
        r.apply(op)
        r2.apply(op)
    rng = np.random.default_rng(5)
    n_mp = lm.size()[1]
    for n in (1, 64, 65, 300):
        slots = rng.integers(-1, n_mp, n).astype(np.int32)
        mask = (rng.random(n) < 0.6).astype(np.uint8)
        d_s, d_m = torch.from_numpy(slots).cuda(), torch.from_numpy(mask).cuda()
        for kind, name, use_mask in ((native.MAP_FOUND, "found", True), (native.MAP_VISIBLE, "visible", False)):
            lm.increase_counters_device(kind, n, d_s.data_ptr(), d_m.data_ptr() if use_mask else None)
            torch.cuda.synchronize()
            live = [int(x) for x, k in zip(slots, mask) if x >= 0 and (k or not use_mask)]
            op = ("inc", name, [r.mp_names[x] for x in live], None)
            assert r2.apply(op) == m.run(op)
            assert r.state() == m.state()
    before = r.state()
    for bad in (n_mp, -2):
        d_s = torch.tensor([0, 1, bad, 2], dtype=torch.int32).cuda()
        with pytest.raises(abi.OrbfeError) as e:
            lm.increase_counters_device(native.MAP_FOUND, 4, d_s.data_ptr())
        assert e.value.status == abi.ORBFE_ERR_ARG
        assert r.state() == before


def test_bad_arguments(lm):
    lm.clear()
    r = Q.LibraryRunner(lm)
    s = Q.case_cullpoints(0)
    r.run(s[:[i for i, op in enumerate(s) if op[0] == "cullpoints"][0]])
    before = r.state()
    L = native.lib()
    n_kf, n_mp = lm.size()
    E = abi.ORBFE_ERR_ARG
    n, nc = C.c_int32(0), C.c_int32(0)
    out = np.zeros(4, np.int32)
    p = abi.ptr
    for lst in ([0, n_mp], [-1], [1, 2, -5]):
        a = np.asarray(lst, np.int32)
        assert L.orbfe_map_cull_points(lm._h, 5, 0, p(a), len(a), C.byref(n), p(out), C.byref(nc)) == E
        assert L.orbfe_map_set_point_bad_flag(lm._h, len(a), p(a)) == E
        assert L.orbfe_map_increase_counters(lm._h, native.MAP_FOUND, len(a), p(a), None) == E
        assert L.orbfe_map_get_point_counters(lm._h, len(a), p(a), p(out), None, None, None) == E
    a = np.asarray([0, 1], np.int32)
    for cur in (-1, 1 << 31, 1 << 40):
        assert L.orbfe_map_cull_points(lm._h, cur, 0, p(a), 2, C.byref(n), p(out), C.byref(nc)) == E
    assert L.orbfe_map_cull_points(lm._h, 5, 0, p(a), 2, None, p(out), C.byref(nc)) == E
    assert L.orbfe_map_cull_points(lm._h, 5, 0, p(a), 2, C.byref(n), None, C.byref(nc)) == E
    assert L.orbfe_map_increase_counters(lm._h, 2, 2, p(a), None) == E
    assert L.orbfe_map_add_observations_idx(lm._h, 2, p(a), p(a), None) == E
    big = np.asarray([40, 0], np.int32)      # the keyframes have 40 slots
    assert L.orbfe_map_add_observations_idx(lm._h, 2, p(a), p(a), p(big)) == E
    assert L.orbfe_map_erase_observation(lm._h, n_mp, 0, None) == E
    assert L.orbfe_map_erase_observation(lm._h, 0, n_kf, None) == E
    assert L.orbfe_map_tracked_map_points(lm._h, n_kf, 0, C.byref(n)) == E
    assert L.orbfe_map_tracked_map_points(lm._h, 0, 0, None) == E
    f = np.zeros(40, np.float32)
    o = np.zeros(40, np.int32)
    assert L.orbfe_map_set_keyframe_features(lm._h, 0, 39, p(o), p(f), p(f), 1.0) == E
    o[7] = 128
    assert L.orbfe_map_set_keyframe_features(lm._h, 0, 40, p(o), p(f), p(f), 1.0) == E
    o[7] = -1
    assert L.orbfe_map_set_keyframe_features(lm._h, 0, 40, p(o), p(f), p(f), 1.0) == E
    assert L.orbfe_map_get_keyframe_points(lm._h, 0, p(out), 4, C.byref(n)) == abi.ORBFE_ERR_CAPACITY
    assert n.value == 40
    assert L.orbfe_map_get_observations(lm._h, 0, p(out), None, 1, C.byref(n)) == abi.ORBFE_ERR_CAPACITY
    assert n.value == 4
    assert r.state() == before
    assert L.orbfe_map_cull_points(lm._h, 5, 0, None, 0, C.byref(n), None, C.byref(nc)) == abi.ORBFE_OK
    assert L.orbfe_map_set_point_bad_flag(lm._h, 0, None) == abi.ORBFE_OK
    assert lm.get_keyframe_features(0)[0][7] == 7        # the refused calls wrote nothing


def test_features_default_and_clear():
    """A keyframe that never had set_keyframe_features reads as octave 0, no right coordinate,
    depth -1; so does a keyframe that takes the place of one that had, after clear."""
    m = native.LocalMap(0, 0, 0)
    try:
        for round_ in (0, 1):
            first = m.add_points(3)
            a = m.add_keyframe(100, 5, [first, -1, first + 1, -1, first + 2])
            b = m.add_keyframe(50, 70)
            o, r, d, th = m.get_keyframe_features(a)
            assert (o == 0).all() and not r.any() and (d == -1).all() and th == 0 and len(o) == 5
            m.set_keyframe_features(a, [1, 2, 3, 4, 127], [0.0, -0.0, -1e-30, np.nan, np.inf],
                                    [np.nan, -0.0, 1.5, np.inf, -2.0], 2.5)
            o, r, d, th = m.get_keyframe_features(a)
            assert list(o) == [1, 2, 3, 4, 127] and list(r) == [True, True, False, False, True] and th == 2.5
            assert np.array_equal(d, np.asarray([np.nan, -0.0, 1.5, np.inf, -2.0], np.float32), equal_nan=True)
            assert np.signbit(d[1])
            o, r, d, th = m.get_keyframe_features(b)
            assert (o == 0).all() and not r.any() and (d == -1).all() and len(o) == 70
            m.AddObservation([first, first + 1, first + 2], [a, a, a], [0, 2, 4])
            assert list(m.get_point_counters([first, first + 1, first + 2])[0]) == [2, 1, 2]
            m.clear()
    finally:
        m.close()


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_seeded_keyframe_culling(lm, seed):
    """Dense seeded maps: calls that cull none, one, two and more keyframes, deferred ones, the
    tournament with ties."""
    check(lm, Q.seeded_kf_script(seed))


def test_keyframe_culling_decisions(lm):
    """What the built cases pin, named: nMPs 10 with 9 (kept) and 10 (culled), 20 with 18 and 19,
    nMPs 0, a point held twice (19 of 21), a cull that flips a later keyframe to kept and one that
    flips a later one to culled, the listed mnId == 0 keyframe, a deferred keyframe culled by
    SetErase, the depth edges in stereo against mono, an unknown index."""
    want = check(lm, Q.case_cullkfs(0))
    outs = [w[0] for w in want if isinstance(w, tuple) and len(w) == 2 and isinstance(w[1], tuple) and w[0] is not None]
    lists = [dict(zip(o[0], o[1])) for o in outs if isinstance(o, tuple) and len(o) == 4]
    assert lists[0] == {"D2": 0}
    assert lists[1] == {"B9": 0, "D18": 0, "E0": 0, "Z": 0} and lists[2]["Z"] == 1 and lists[2]["D2"] == 1
    assert outs[4][1] == [0, 2, 0, 2] and outs[5] == (1, [], []) and outs[6][0] == 2
    assert lists[5] == {"B9": 0, "A": 1, "F": 0, "D18": 0, "A2": 0, "G": 1, "Z": 0} and outs[7][2] == ["g_q"]
    assert lists[-1] == {"B9": 1} and outs[-1] == "error"
    want = check(lm, Q.case_cullkfs(1))
    assert [w[0] for w in want if isinstance(w, tuple) and len(w) == 2 and isinstance(w[1], tuple) and
            isinstance(w[0], tuple) and len(w[0]) == 4][1][1] == [0, 0, 0, 1]     # mono: Z culled


@pytest.mark.parametrize("n", [0, 1, 64, 65, 130])
def test_keyframe_lists(lm, n):
    """Lists of 0, 1, 64, 65 and 130 keyframes (all but the helpers redundant: every second one is
    culled, since each cull takes an observer from its neighbours)."""
    check(lm, Q.script_kf_list(n))


def test_all_and_none_culled(lm):
    want = check(lm, Q.script_kf_list(12, share=False))
    assert want[-1][0][1] == [1] * 12
    want = check(lm, Q.script_kf_list(12, octave=3))
    assert want[-1][0][1] == [0] * 12


def test_list_capacity(lm):
    """4,097 listed keyframes: ORBFE_ERR_CAPACITY with nothing changed; 4,096 run."""
    s = Q.script_kf_list(3)
    names = [op[1] for op in s if op[0] == "kf"]
    cut = s[:-1]
    want = check(lm, cut + [("cullkfs", names[0], [names[-1 - i % 3] for i in range(4097)], None, True),
                            ("cullkfs", names[0], [names[-1 - i % 3] for i in range(4096)], None, True)])
    assert want[-2][0] == "capacity" and len(want[-1][0][1]) == 4096


@pytest.mark.parametrize("nc", [0, 1, 64, 65])
def test_children_counts(lm, nc):
    """A SetBadFlag whose keyframe has 0, 1, 64 and 65 children: some find the parent, some a
    child that left before them, some nobody."""
    want = check(lm, Q.script_kf_children(nc))
    assert len(want[-1][0][2]) == nc


def test_big_keyframe_bad_flag(lm):
    """SetBadFlag and KeyFrameCulling of an 8,192-slot keyframe (16 waves striding it, several
    workgroups of erases)."""
    want = check(lm, Q.script_kf_big())
    assert want[-1][0][0] == Q.DONE and len(want[-1][0][1]) > 1000


def test_hints_of_zero_clear_and_reuse():
    m = native.LocalMap(0, 0, 0)
    try:
        for v in (0, 1):
            check(m, Q.case_cullpoints(v))
            check(m, Q.case_observations(v))
            check(m, Q.case_kfbadflag(v))
            check(m, Q.seeded_kf_script(40 + v))
    finally:
        m.close()


def test_chain_with_the_existing_calls(lm):
    """A scripted LocalMapping cycle: a new keyframe, its observations with indices,
    MapPointCulling, UpdateConnections, UpdateLocalMap, against the same chain on the restatement:
    the calls that existed before see what the new ones changed (entries NULLed, points set bad,
    observation rows cleared)."""
    for v in (0, 1):
        s, names, pts = Q._map(v, 6, 60)
        s.append(("obsidx", [(p, n, j) for j, p in enumerate(pts) for n in names[:5] if (j + len(n)) % 7]))
        s.append(("update_batch", names[:5]))
        new = list(pts)
        s.append(("obsidx", [(p, names[5], j) for j, p in enumerate(new)]))
        s.append(("counters", pts[:20], None, [0] * 20, [3] * 20, None))       # ratio 0: culled
        s.append(("counters", pts[20:30], [3] * 10, None, None, [1] * 10))     # few observations
        s.append(("cullpoints", pts[:45] + pts[:5], 3, False))
        s.append(("update", names[5]))
        s.append(("update_batch", names))
        for n in names:
            s.append(("features", n, None, None, None, 0.0))       # one octave: what is left is redundant
        s.append(("cullkfs", names[5], None, names[0], True))
        s.append(("localmap", 9, pts[25:40] + [None, pts[0]]))
        s.append(("tracked", names[5], 3))
        s.append(("update_batch", names))
        want = check(lm, s)
        culled = want[-13][0][1]
        assert len(culled) == 32 and 0 < dict(want[-12][names[5]][0])[names[0]] <= 30
        assert Q.CULLED in want[-4][0][1] and want[-4][0][1][want[-4][0][0].index(names[0])] == Q.KEPT
        assert want[-3][3][-1] is None     # the bad point in the frame was NULLed


def test_increase_counters_from_search_local_points(lm):
    """The device form fed from orbfe_search_local_points_device's own outputs, as
    Tracking::SearchLocalPoints / TrackLocalMap use them: IncreaseVisible over the gathered local
    point list masked by in_view, IncreaseFound over the frame's points after the search (-1
    entries skipped); the expected counters are counted with numpy from the arrays the search
    returned, and the host form on the same lists must agree."""
    import torch
    import localmap_cases as LK
    import scenarios as S
    from orbslam_mapsave_amd.synth import synthetic_local_map
    dev = torch.device("cuda", 0)
    f = S.extract_frame(0, 1000)
    M, nkf = 3000, 8
    world = synthetic_local_map(f.keys, f.desc, M, seed=4)
    rng = np.random.default_rng(12)
    lm.clear()
    r = LK.LibraryRunner(lm)
    r.apply(("points", [f"p{i}" for i in range(M)]))
    for k in range(nkf):
        held = rng.choice(M // 2 + k * 150, 500, replace=False)
        mps = [f"p{i}" for i in held]
        r.apply(("kf", f"k{k}", LK.BASE + 64 * k, mps))
        lm.AddObservation([r.mp[p] for p in mps], [k] * len(mps), list(range(len(mps))))
    r.apply(("mpbad", [f"p{i}" for i in np.flatnonzero(world["bad"])], True))
    frame_mp = np.array([rng.integers(0, M // 2) if rng.uniform() < 0.15 else -1 for _ in range(f.n)], np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_fmp, d_fobs = up(frame_mp), up(np.where(frame_mp >= 0, 2, 0).astype(np.int32))
    torch.cuda.synchronize()
    _, _, n = lm.update_local_device(12, f.n, d_fmp.data_ptr())
    assert n > 1000
    src = {k: up(world[w]) for k, w in (("xyz", "xyz"), ("normal", "normal"), ("min_dist", "min_dist"),
                                        ("max_dist", "max_dist"), ("desc", "desc"), ("n_obs", "nobs"),
                                        ("skip", "skip"))}
    dst = {"xyz": torch.zeros((n, 3), dtype=torch.float32, device=dev),
           "normal": torch.zeros((n, 3), dtype=torch.float32, device=dev),
           "min_dist": torch.zeros(n, dtype=torch.float32, device=dev),
           "max_dist": torch.zeros(n, dtype=torch.float32, device=dev),
           "desc": torch.zeros((n, 32), dtype=torch.uint8, device=dev),
           "n_obs": torch.zeros(n, dtype=torch.int32, device=dev),
           "skip": torch.zeros(n, dtype=torch.uint8, device=dev),
           "mp_ids": torch.zeros(n, dtype=torch.int32, device=dev),
           "bad": torch.ones(n, dtype=torch.uint8, device=dev)}
    d_list, _ = lm.local_points_device()
    lm.gather_points_device(n, d_list, native.MapPointArrays(**{k: v.data_ptr() for k, v in src.items()}),
                            native.MapPointArrays(**{k: v.data_ptr() for k, v in dst.items()}))
    lm.get_local_points()
    d_inv = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_keys, d_desc = up(f.keys.view(np.uint8)), up(f.desc)
    mt = native.ORBmatcher(0.8, False, device=0)
    try:
        counts = mt.search_local_points_device(
            f.n, d_keys.data_ptr(), d_desc.data_ptr(), None, S.W, S.H, f.scale_factors,
            world["tcw"], S.camera(), float(np.log(np.float32(1.2)).astype(np.float32)), 0.5, n,
            dst["xyz"].data_ptr(), dst["normal"].data_ptr(), dst["min_dist"].data_ptr(),
            dst["max_dist"].data_ptr(), dst["desc"].data_ptr(), dst["n_obs"].data_ptr(),
            dst["bad"].data_ptr(), dst["skip"].data_ptr(), dst["mp_ids"].data_ptr(), 0.8, 3.0,
            d_fmp.data_ptr(), d_fobs.data_ptr(), d_inv.data_ptr())
        torch.cuda.synchronize()
    finally:
        mt.close()
    assert counts[0] > 0
    every = np.arange(M, dtype=np.int32)
    before = lm.get_point_counters(every)
    lm.increase_counters_device(native.MAP_VISIBLE, n, dst["mp_ids"].data_ptr(), d_inv.data_ptr())
    lm.increase_counters_device(native.MAP_FOUND, f.n, d_fmp.data_ptr())
    after = lm.get_point_counters(every)
    ids, inv, fmp = dst["mp_ids"].cpu().numpy(), d_inv.cpu().numpy(), d_fmp.cpu().numpy()
    visible = np.bincount(ids[inv != 0], minlength=M)
    found = np.bincount(fmp[fmp >= 0], minlength=M)
    assert visible.sum() > 100 and found.sum() > 100
    assert np.array_equal(after[2] - before[2], visible) and np.array_equal(after[1] - before[1], found)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[3], before[3])
    lm.IncreaseVisible(ids[inv != 0])
    lm.IncreaseFound(fmp[fmp >= 0])
    again = lm.get_point_counters(every)
    assert np.array_equal(again[2] - after[2], visible) and np.array_equal(again[1] - after[1], found)
