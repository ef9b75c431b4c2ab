"""MapPoint refresh on the device (orbfe_map_refresh_points and its companions, native.LocalMap)
against the restatement of tests/refresh_cases.py: after every operation of every script the whole
new state (every point's mpRefKF, normal, distances and descriptor) and the culling state are read
back and compared exactly, with the operation's own output; the host form, the device-list form
and the keyframe form against each other; at the observer counts where the kernel takes another
path; the error contract; and the chain into the calls that existed before."""
import numpy as np
import pytest

import refresh_cases as R
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


def check(m, script, form="host", desc_via="host", want=None):
    m.clear()
    want = R.run_script(script) if want is None else want
    got = R.LibraryRunner(m, "batch", form, desc_via).run(script)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w and isinstance(w, tuple) and len(w) == 2 and isinstance(w[1], tuple):
            assert g[0] == w[0], (i, g[0], w[0])
            for part in (0, 1, 2, 3, 4):
                bad = sorted(n for n in w[1][part] if g[1][part].get(n) != w[1][part][n])[:4]
                assert not bad, (i, part, [(n, g[1][part].get(n), w[1][part][n]) for n in bad])
        assert g == w, i
    return want


@pytest.mark.parametrize("case", [c.__name__[5:] for c in R.CASES])
def test_built_cases(lm, lm2, case):
    fn = [c for c in R.CASES if c.__name__[5:] == case][0]
    for v in range(5):
        want = check(lm, fn(v), "host")
        check(lm2, fn(v), ("device", "kf")[v % 2], "device", want)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 63, 64, 65, 200])
def test_observer_counts(lm, lm2, n):
    """The median index at each small N, the wave seam and the LDS staging seam, a row sorted in
    LDS; keys descending, shuffled and ascending against the slots."""
    for v in (0, 1, 2):
        want = check(lm, R.script_observer_count(n, v), "host")
        if v == 1:
            check(lm2, R.script_observer_count(n, v), "device", "device", want)


def test_observer_capacity(lm):
    """1,024 observers exactly; 1,025: capacity, the sentinel-filled arrays untouched."""
    want = check(lm, R.script_observer_count(1024, 1), "host")
    assert want[-1][0] == [R.ND | R.DESC, 0]
    want = check(lm, R.script_observer_count(1025, 1), "device")
    assert want[-1][0] == "capacity"
    normal, dists, desc = want[-1][1][4]["P"]
    assert desc == bytes([R.SENT_DESC]) * 32 and normal == R._fbits([R.SENT_NORMAL] * 3)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 257])
def test_lists(lm, lm2, n):
    """Lists shorter than, equal to and longer than a workgroup's waves, with -1, bad and repeated
    entries; the two list forms against each other."""
    want = check(lm, R.script_list(n), "host")
    check(lm2, R.script_list(n), "device", "host", want)


def _mid_script(extra):
    s, pts = R._world(1, 3, slots=4)
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(3) for j, p in enumerate(pts)]))
    s.append(("refkf", pts, ["K0", "K1", "K2", None]))
    return s + extra(pts), pts


def test_arithmetic_edges(lm):
    """A point at a camera centre (a = inf, NaN components); +-inf coordinates."""
    def extra(pts):
        return [("centers", ["K1"], [[1.5, -2.5, 3.5]]),
                ("xyz", pts, [[1.5, -2.5, 3.5], [float("inf"), 0.0, 1.0], [1.0, float("-inf"), 2.0],
                              [float("inf"), float("-inf"), float("inf")]]),
                ("refresh", R.ND | R.DESC, pts)]
    s, pts = _mid_script(extra)
    want = check(lm, s, "host")
    assert "nan" in want[-1][1][4][pts[0]][0]


def test_big_keyframe_last_index(lm):
    """An 8,192-slot keyframe observed at its last index: the descriptor pool's far end."""
    s = [("points", ["P"]), ("scale", R.SCALE8)]
    rows = R._desc_rows(4, 8192)
    for i, key in enumerate((R.BASE + 64, R.BASE + 32, R.BASE + 16)):
        s.append(("kf", f"K{i}", key, [None] * 8191 + ["P"]))
        s.append(("features", f"K{i}", [j % 8 for j in range(8192)], None, None, 40.0))
        d = rows.copy()
        d[8191, i] ^= 1 << i
        s.append(("descs", f"K{i}", d))
    s.append(("centers", ["K0", "K1", "K2"], [[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [-1.0, 0.25, 0.0]]))
    s.append(("xyz", ["P"], [[0.5, 0.5, 6.0]]))
    s.append(("obsidx", [("P", f"K{i}", 8191) for i in range(3)]))
    s.append(("refkf", ["P"], ["K1"]))
    s.append(("refreshkf", "K1", R.ND | R.DESC))
    check(lm, s, "kf", "device")


def test_refusals_leave_everything_untouched(lm):
    """Each refusal of the contract, one at a time, against the state before it."""
    def extra(pts):
        return [("refresh", R.ND | R.DESC, pts)]
    s, pts = _mid_script(extra)
    lm.clear()
    r = R.LibraryRunner(lm)
    m = R.Model()
    for op in s:
        m.run(op)
        r.apply(op)
    before = r.state()
    assert before == m.state()
    arr = r.arrays()
    E, Cap = abi.ORBFE_ERR_ARG, abi.ORBFE_ERR_CAPACITY

    def refused(status, fn):
        with pytest.raises(abi.OrbfeError) as e:
            fn()
        assert e.value.status == status
        assert r.state() == before

    n_mp = lm.size()[1]
    refused(E, lambda: lm.RefreshPoints(3, [0, n_mp], arr))             # outside [-1, points)
    refused(E, lambda: lm.RefreshPoints(3, [0, -2], arr))
    refused(E, lambda: lm.RefreshPoints(0, [0], arr))                   # no such `what`
    refused(E, lambda: lm.RefreshPoints(4, [0], arr))
    nul = native.MapPointArrays()
    refused(E, lambda: lm.RefreshPoints(3, [0], nul))                   # the arrays it writes
    odd = r.arrays()
    odd.desc += 8
    refused(E, lambda: lm.RefreshPoints(2, [0], odd))                   # desc not 16-byte aligned
    refused(E, lambda: lm.SetDescriptors(0, np.zeros((3, 32), np.uint8)))   # n != the slot count
    refused(E, lambda: lm.SetScaleFactors([]))
    refused(E, lambda: lm.SetScaleFactors([1.0] * 129))
    refused(E, lambda: lm.SetReferenceKeyFrame([0], [99]))
    refused(E, lambda: lm.SetCameraCenter([99], [[0, 0, 0]]))
    refused(Cap, lambda: lm.ProcessNewKeyFrame(0, arr, 0))              # every point is recent
    # a keyframe without descriptors among the observers; an observation without an index
    for op in (("points", ["X", "Y"]), ("kf", "U", R.BASE + 8, ["X", "Y"]),
               ("obsidx", [("X", "U", 0), ("X", "K0", 1)]), ("obs", [("Y", "K0")])):
        m.run(op)
        r.apply(op)
    before = r.state()
    assert before == m.state()
    arr = r.arrays()
    x, y = r.mp["X"], r.mp["Y"]
    refused(E, lambda: lm.RefreshPoints(2, [0, x], arr))
    refused(E, lambda: lm.RefreshPoints(1, [0, y], arr))
    # a new keyframe without descriptors: refused before its observations are added
    refused(E, lambda: lm.ProcessNewKeyFrame(r.kf["U"], arr))
    assert m.run(("process", "U")) == ("error", before)
    assert [int(v) for v in lm.RefreshPoints(1, [0, x], arr)] == [1, 0]  # X: no reference, nothing written
    # without a scale table the normal is refused, the descriptor is not
    lm.clear()
    r = R.LibraryRunner(lm)
    for op in s:
        if op[0] not in ("scale", "refresh"):
            r.apply(op)
    before = r.state()
    arr = r.arrays()
    refused(E, lambda: lm.RefreshPoints(1, [0], arr))
    refused(E, lambda: lm.RefreshKeyFramePoints(0, arr, 3))
    refused(E, lambda: lm.ProcessNewKeyFrame(0, arr))
    assert [int(v) for v in lm.RefreshPoints(2, [0], arr)] == [2]


def test_state_survives_growth_and_clear(lm):
    """The new columns and the descriptor pool are carried over when the map grows past its first
    capacities, and reset by clear."""
    lm.clear()
    r = R.LibraryRunner(lm)
    m = R.Model()
    s, pts = R._world(3, 3, slots=5)
    s.append(("obsidx", [(p, f"K{i}", j) for i in range(3) for j, p in enumerate(pts)]))
    s.append(("refkf", pts, ["K0", "K1", "K2", "K1", None]))
    for op in s:
        m.run(op)
        r.apply(op)
    descs = [lm.GetDescriptors(i)[0].tobytes() for i in range(3)]
    cents = lm.GetCameraCenter([0, 1, 2]).tobytes()
    more = [f"G{i}" for i in range(3000)]
    for op in [("points", more)] + [("kf", f"B{i}", R.BASE + 0x100000 + i, more[:1500]) for i in range(40)]:
        m.run(op)
        r.apply(op)
    assert [lm.GetDescriptors(i)[0].tobytes() for i in range(3)] == descs
    assert lm.GetCameraCenter([0, 1, 2]).tobytes() == cents
    d10, set10 = lm.GetDescriptors(10)
    assert d10.shape == (1500, 32) and not d10.any() and not set10
    op = ("refresh", 3, pts + more[:3])
    got, want = r.apply(op), m.run(op)
    assert got[0] == want[0] and got[1][3] == want[1][3] and got[1][4] == want[1][4]
    lm.clear()
    assert len(lm.GetScaleFactors()) == 0
    r = R.LibraryRunner(lm)
    r.apply(("points", ["A"]))
    r.apply(("kf", "K", 5, ["A"]))
    assert lm.GetReferenceKeyFrame(0) == -1
    assert lm.GetDescriptors(0)[1] is False and not lm.GetDescriptors(0)[0].any()
    assert lm.GetCameraCenter(0).tobytes() == bytes(12)


def test_chain_into_search_local_points(lm, lm2):
    """process_new_keyframe -> update_connections -> update_local -> gather_points_device ->
    orbfe_search_local_points_device, against the same chain fed from the restatement's arrays:
    the gathered inputs are the same bytes and the search answers the same."""
    import torch

    import scenarios as S
    s = R.case_process(1)
    cut = [i for i, op in enumerate(s) if op[0] == "process"][1]
    lm.clear()
    r = R.LibraryRunner(lm)
    m = R.Model()
    for op in s[:cut + 1]:
        m.run(op)
        r.apply(op)
    assert lm.size()[1] == len(m.mps)
    # the restatement's arrays, uploaded: what a caller that refreshes on its CPU would hold
    ref = {k: v.clone() for k, v in r.t.items()}
    for n, mp in m.mps.items():
        i = r.mp[n]
        ref["normal"][i] = torch.from_numpy(mp.normal).cuda()
        ref["min_dist"][i] = float(mp.mind)
        ref["max_dist"][i] = float(mp.maxd)
        ref["desc"][i] = torch.from_numpy(mp.desc).cuda()
    lm.UpdateConnections(r.kf["N"])
    frame = [r.mp[p] for p in ("P0", "P1", "S0")]
    kfs, refkf, pts, _ = lm.UpdateLocalMap(7, frame)
    assert len(pts) > 3
    d_list, n = lm.local_points_device()
    f = S.extract_frame(0, 1000)
    d_keys = torch.from_numpy(np.ascontiguousarray(f.keys.view(np.uint8))).cuda()
    d_desc = torch.from_numpy(np.ascontiguousarray(f.desc)).cuda()
    tcw = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    mt = native.ORBmatcher(0.8, False, device=0)
    outs = []
    for src_t in (r.t, ref):
        extra = {"n_obs": torch.full((r.cap,), 2, dtype=torch.int32, device="cuda"),
                 "skip": torch.zeros(r.cap, dtype=torch.uint8, device="cuda")}
        dst_t = {"xyz": torch.zeros(n, 3, device="cuda"), "normal": torch.zeros(n, 3, device="cuda"),
                 "min_dist": torch.zeros(n, device="cuda"), "max_dist": torch.zeros(n, device="cuda"),
                 "desc": torch.zeros(n, 32, dtype=torch.uint8, device="cuda"),
                 "n_obs": torch.zeros(n, dtype=torch.int32, device="cuda"),
                 "skip": torch.zeros(n, dtype=torch.uint8, device="cuda"),
                 "mp_ids": torch.zeros(n, dtype=torch.int32, device="cuda"),
                 "bad": torch.zeros(n, dtype=torch.uint8, device="cuda")}
        d_fmp = torch.full((f.n,), -1, dtype=torch.int32, device="cuda")
        d_fobs = torch.zeros(f.n, dtype=torch.int32, device="cuda")
        d_inv = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        src = native.MapPointArrays(**{k: v.data_ptr() for k, v in {**src_t, **extra}.items()})
        dst = native.MapPointArrays(**{k: v.data_ptr() for k, v in dst_t.items()})
        lm.gather_points_device(n, d_list, src, dst)
        lm.get_local_points()   # synchronises the handle's stream: the gather is complete
        a = dst_t
        counts = mt.search_local_points_device(
            f.n, d_keys.data_ptr(), d_desc.data_ptr(), None, S.W, S.H, f.scale_factors, tcw, S.camera(),
            float(np.log(np.float32(1.2)).astype(np.float32)), 0.5, n, a["xyz"].data_ptr(),
            a["normal"].data_ptr(), a["min_dist"].data_ptr(), a["max_dist"].data_ptr(), a["desc"].data_ptr(),
            a["n_obs"].data_ptr(), a["bad"].data_ptr(), a["skip"].data_ptr(), a["mp_ids"].data_ptr(), 0.8, 3.0,
            d_fmp.data_ptr(), d_fobs.data_ptr(), d_inv.data_ptr())
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy().tobytes() for k, v in dst_t.items()}
        out["search"] = (tuple(counts), d_inv.cpu().numpy().tobytes(), d_fmp.cpu().numpy().tobytes(),
                         d_fobs.cpu().numpy().tobytes())
        out["in view"] = int(d_inv.sum())
        outs.append(out)
    mt.close()
    assert outs[0] == outs[1]
    assert outs[0]["in view"] > 0      # the refreshed normal and distances decided something
