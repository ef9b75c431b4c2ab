"""Tracking::UpdateLocalMap on the device (orbfe_map_*, native.LocalMap) against the restatement
of tests/localmap_cases.py, bit for bit after every call: the keyframe list and its order, the
reference keyframe, the point list and its order, the updated frame points, and every keyframe's
and point's stamp; on the built cases, on seeded walks and at the shapes where a kernel can break;
the error contract; and the chain update_local_device -> gather_points_device ->
orbfe_search_local_points_device against the host chain on the restatement's list."""
import numpy as np
import pytest

import localmap_cases as K
import scenarios as S
from orbslam_mapsave_amd import abi, native
from orbslam_mapsave_amd.synth import synthetic_local_map

pytestmark = pytest.mark.gpu

FIELDS = ("local keyframes", "reference keyframe", "local points", "frame points", "keyframe stamps",
          "point stamps")


@pytest.fixture(scope="module")
def lm():
    m = native.LocalMap(0)
    yield m
    m.close()


def device_update(m, fid, frame):
    """The device form: frame_mp in HBM, the point list read back from the device."""
    import torch
    d = torch.tensor(list(frame) or [0], dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    kfs, ref, nmp = m.update_local_device(fid, len(frame), d.data_ptr())
    ptr, n = m.local_points_device()
    pts = m.get_local_points()
    assert n == nmp == len(pts) and (ptr != 0 or n == 0)
    return kfs, ref, pts, d.cpu().numpy()[:len(frame)]


def check(m, script, form="host"):
    m.clear()
    want = K.run_script(script)
    got = K.LibraryRunner(m, device_update if form == "device" else None).run(script)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for j, f in enumerate(FIELDS):
            assert g[j] == w[j], (i, f)
    return want


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("case", sorted(K.CASES))
def test_built_cases(lm, case, form):
    for v in K.VARIANTS:
        check(lm, K.CASES[case](v), form)


@pytest.mark.parametrize("seed,form", [(1, "host"), (2, "device"), (3, "host")])
def test_seeded_walks(lm, seed, form):
    want = check(lm, K.seeded_script(seed, 80), form)
    assert sum(1 for a in want if a[2]) > 10


@pytest.mark.parametrize("form", ["host", "device"])
def test_observation_sets_and_frame_sizes(lm, form):
    """Observation sets of 0, 1, 63, 64, 65 and 200 keyframes (a wave's stride and its tail) and
    frames of 0, 1, 63, 64, 65 and 257 keypoints (a workgroup of 16 waves and its tail)."""
    want = check(lm, K.script_observation_sets(), form)
    assert [len(a[0]) for a in want[:6]] == [0, 1, 63, 64, 65, 200]


@pytest.mark.parametrize("nv", [0, 1, 79, 80, 81])
def test_voted_keyframes_around_the_gate(lm, nv):
    want = check(lm, K.script_many_keyframes(nv), "device" if nv % 2 else "host")
    assert len(want[0][0]) == (nv + 1 if 0 < nv <= 80 else nv)


def test_children_counts(lm):
    """0, 1, 64 and 65 children (one ballot chunk, its end and the next) with the first eligible
    child last in key order; the second call finds them stamped."""
    want = check(lm, K.script_children(), "device")
    assert len(want[0][0]) == 7


def test_point_list_seams_and_the_largest_keyframe(lm):
    """Point lists that end one below, on and one above the compaction block and twice it, and a
    keyframe of 8192 slots."""
    want = check(lm, K.script_point_lists(1024), "device")
    assert [len(a[2]) for a in want[:7]] == [1023, 1024, 1025, 2047, 2048, 2049, 8192]


def _state(m, nk, nmp):
    return (m.get_local_keyframes()[0].tolist(), m.get_local_keyframes()[1],
            m.get_local_points().tolist(), m.get_stamps(0, list(range(nk))).tolist(),
            m.get_stamps(1, list(range(nmp))).tolist())


def test_4096_voted_keyframes_and_one_more(lm):
    """4096 voted keyframes are answered exactly; 4097 return ORBFE_ERR_CAPACITY with the number
    and every stamp, the lists and the reference keyframe untouched."""
    script = K.script_many_keyframes(K.MAX_VOTED, extra=3)
    want = check(lm, script)
    assert len(want[0][0]) == K.MAX_VOTED and len(want[0][2]) == K.MAX_VOTED
    # point 5 goes bad (its keyframe loses its only vote) and two of the three spare keyframes
    # are voted for: 4097
    nk, npt = lm.size()
    assert nk == K.MAX_VOTED + 3 and npt == nk
    before = _state(lm, nk, npt)
    frame = np.arange(K.MAX_VOTED + 2, dtype=np.int32)
    lm.SetBadFlagPoints([5])
    for update in (lambda: lm.UpdateLocalMap(77, frame),
                   lambda: device_update(lm, 78, frame)):
        with pytest.raises(abi.OrbfeError) as e:
            update()
        assert e.value.status == abi.ORBFE_ERR_CAPACITY and e.value.counts[0] == K.MAX_VOTED + 1
        assert _state(lm, nk, npt) == before
    # the handle still answers: the bad point is NULLed and its keyframe drops out
    kfs, ref, pts, f = lm.UpdateLocalMap(79, frame[:-2])
    assert len(kfs) == K.MAX_VOTED - 1 and f[5] == -1 and len(pts) == K.MAX_VOTED - 1


def test_refused_arguments_on_a_live_handle(lm):
    lm.clear()
    E = abi.ORBFE_ERR_ARG
    p0 = lm.add_points(4)
    a = lm.add_keyframe(1000, 4, [p0, -1, p0 + 1, p0 + 3])
    b = lm.add_keyframe(999, 0)
    assert (a, b, p0) == (0, 1, 0)

    def refused(fn, *args):
        with pytest.raises(abi.OrbfeError) as e:
            fn(*args)
        assert e.value.status == E, fn
    refused(lm.add_keyframe, 1000, 0)                                   # the key is taken
    refused(lm.add_keyframe, 5, K.MAX_KF_SLOTS + 1)
    refused(lm.add_keyframe, 5, 2, [0, 4])                              # point 4 does not exist
    refused(lm.UpdateBestCovisibles, a, [b] * 11)                       # an 11th neighbour
    refused(lm.UpdateBestCovisibles, a, [2])
    refused(lm.set_children, a, [b, 7])
    refused(lm.set_parent, a, 2)
    refused(lm.set_parent, 2, a)
    refused(lm.set_keyframe_points, a, 3, [0, 1])                       # past the keyframe's slots
    refused(lm.set_keyframe_points, a, 0, [-2])
    refused(lm.SetBadFlag, 2)
    refused(lm.SetBadFlagPoints, [0, 4])
    refused(lm.AddObservation, [0, 1], [0, 2])
    refused(lm.EraseObservation, [4], [0])
    refused(lm.set_stamps, 0, [2], [1])
    refused(lm.set_stamps, 2, [0], [1])
    refused(lm.get_stamps, 1, [4])
    refused(lm.set_local_keyframes, [0, 2], -1)
    refused(lm.set_local_keyframes, [0], 5)
    refused(lm.UpdateLocalMap, 3, [0, 4])
    assert lm.size() == (2, 4)
    # a device frame_mp with an entry outside the map is caught on the device, nothing written
    lm.AddObservation([0, 1], [0, 1])
    before = _state(lm, 2, 4)
    for bad in (4, -2, 1 << 30):
        with pytest.raises(abi.OrbfeError) as e:
            device_update(lm, 3, [0, bad, 1])
        assert e.value.status == E and _state(lm, 2, 4) == before
    kfs, ref, pts, f = device_update(lm, 3, [0, -1, 1])
    assert kfs.tolist() == [1, 0] and ref == 1 and pts.tolist() == [0, 1, 3]


def test_small_buffers_report_the_true_counts(lm):
    """A buffer that is too small: ORBFE_ERR_CAPACITY, the true counts, nothing copied; the
    handle's state has advanced as after a successful call."""
    script = K.case_points(0)
    first = next(i for i, op in enumerate(script) if op[0] == "update")
    lm.clear()
    r = K.LibraryRunner(lm)
    for op in script[:first]:
        r.apply(op)
    want = K.run_script(script[:first + 1])[0]
    fid, frame = script[first][1], r._mps(script[first][2])
    with pytest.raises(abi.OrbfeError) as e:
        lm.UpdateLocalMap(fid, frame, kf_cap=len(want[0]) - 1)
    assert e.value.status == abi.ORBFE_ERR_CAPACITY
    assert e.value.counts == (len(want[0]), len(want[2]))
    kfs, ref = lm.get_local_keyframes()
    assert [r.kf_names[s] for s in kfs] == want[0] and r.kf_names[ref] == want[1]
    assert [r.mp_names[s] for s in lm.get_local_points()] == want[2]
    assert {n: int(v) for n, v in zip(r.mp_names, lm.get_stamps(1, list(range(len(r.mp_names)))))} == want[5]
    # the next frame (OLD's archived stamp no longer matches: one point more)
    want2 = K.run_script(script[:first + 1] + [("update", fid + 1, script[first][2])])[1]
    assert len(want2[2]) == len(want[2]) + 1
    with pytest.raises(abi.OrbfeError) as e:
        lm.UpdateLocalMap(fid + 1, frame, mp_cap=len(want2[2]) - 1)
    assert e.value.status == abi.ORBFE_ERR_CAPACITY
    assert e.value.counts == (len(want2[0]), len(want2[2]))
    assert [r.mp_names[s] for s in lm.get_local_points()] == want2[2]


def test_storage_grows_inside_the_mutators():
    """A handle created without hints, filled past every first allocation; stamps survive the
    growth, set and get round-trip, clear starts over."""
    m = native.LocalMap(0)
    script = K.seeded_script(9, 30, nkf=70, npts=2500, slots=40)
    check(m, script, "device")
    nk, npt = m.size()
    assert nk == 70 and npt == 2500
    big = (1 << 63) + 12345
    m.set_stamps(native.MAP_POINTS, [0, 2499], [big, 7])
    m.set_stamps(native.MAP_KEYFRAMES, [69], [big + 1])
    first = m.add_points(5000)
    assert first == 2500
    for i in range(40):
        assert m.add_keyframe(10**9 + i, 3, [first + i, -1, 0]) == 70 + i
    assert m.get_stamps(native.MAP_POINTS, [0, 2499, 2500, 7499]).tolist() == [big, 7, 0, 0]
    assert m.get_stamps(native.MAP_KEYFRAMES, [69, 70, 109]).tolist() == [big + 1, 0, 0]
    m.clear()
    assert m.size() == (0, 0) and m.get_local_keyframes()[0].tolist() == []
    check(m, K.case_votes(1))
    m.close()


def test_chain_to_search_local_points(lm):
    """update_local_device -> gather_points_device -> orbfe_search_local_points_device on data
    that never leaves the device, against the same search fed from the host with the
    restatement's list: the local map of scenarios' frame, a few thousand points."""
    import torch
    dev = torch.device("cuda", 0)
    f = S.extract_frame(0, 1000)
    M, nkf = 4000, 12
    world = synthetic_local_map(f.keys, f.desc, M, seed=4)     # map-wide arrays, by point slot
    rng = np.random.default_rng(11)
    script = [("points", [f"p{i}" for i in range(M)])]
    keys = rng.permutation(nkf)
    for k in range(nkf):
        held = rng.choice(M // 2 + k * 150, 600, replace=False)   # overlapping sets, 1000 points unheld
        mps = [f"p{i}" if rng.uniform() < 0.9 else None for i in held]
        script.append(("kf", f"k{k}", K.BASE + 64 * int(keys[k]), mps))
        script.append(("obs", [(p, f"k{k}") for p in mps if p is not None]))
    script.append(("mpbad", [f"p{i}" for i in np.flatnonzero(world["bad"])], True))
    frame = [f"p{rng.integers(0, M // 2)}" if rng.uniform() < 0.15 else None for _ in range(f.n)]
    script.append(("update", 12, frame))
    want = K.run_script(script)[0]
    assert 2000 < len(want[2]) < M and len(want[0]) >= 10
    lm.clear()
    r = K.LibraryRunner(lm)
    for op in script[:-1]:
        r.apply(op)
    frame_mp = np.array(r._mps(frame), np.int32)
    frame_obs = np.where(frame_mp >= 0, 2, 0).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_keys, d_desc = up(f.keys.view(np.uint8)), up(f.desc)
    mt = native.ORBmatcher(0.8, False, device=0)

    def search(arr, n, d_fmp, d_fobs):
        d_inv = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        counts = mt.search_local_points_device(
            f.n, d_keys.data_ptr(), d_desc.data_ptr(), None, S.W, S.H, f.scale_factors,
            world["tcw"], S.camera(), float(np.log(np.float32(1.2)).astype(np.float32)), 0.5, n,
            arr["xyz"].data_ptr(), arr["normal"].data_ptr(), arr["min_dist"].data_ptr(),
            arr["max_dist"].data_ptr(), arr["desc"].data_ptr(), arr["n_obs"].data_ptr(),
            arr["bad"].data_ptr(), arr["skip"].data_ptr(), arr["mp_ids"].data_ptr(), 0.8, 3.0,
            d_fmp.data_ptr(), d_fobs.data_ptr(), d_inv.data_ptr())
        return counts, d_inv.cpu().numpy(), d_fmp.cpu().numpy(), d_fobs.cpu().numpy()

    # the host chain: the restatement's list, gathered with numpy
    lst = np.array([r.mp[n] for n in want[2]], np.int32)
    fm = np.array([-1 if n is None else r.mp[n] for n in want[3]], np.int32)
    host = {"xyz": world["xyz"][lst], "normal": world["normal"][lst], "min_dist": world["min_dist"][lst],
            "max_dist": world["max_dist"][lst], "desc": world["desc"][lst], "n_obs": world["nobs"][lst],
            "skip": world["skip"][lst], "mp_ids": lst, "bad": world["bad"][lst]}
    assert not host["bad"].any()
    ref = search({k: up(v) for k, v in host.items()}, len(lst), up(fm), up(frame_obs))
    # the device chain
    src = {k: up(world[w]) for k, w in (("xyz", "xyz"), ("normal", "normal"), ("min_dist", "min_dist"),
                                        ("max_dist", "max_dist"), ("desc", "desc"), ("n_obs", "nobs"),
                                        ("skip", "skip"))}
    d_fmp, d_fobs = up(frame_mp), up(frame_obs)
    torch.cuda.synchronize()
    kfs, refkf, n = lm.update_local_device(12, f.n, d_fmp.data_ptr())
    assert [r.kf_names[s] for s in kfs] == want[0] and r.kf_names[refkf] == want[1] and n == len(lst)
    dst = {"xyz": torch.zeros((n, 3), dtype=torch.float32, device=dev),
           "normal": torch.zeros((n, 3), dtype=torch.float32, device=dev),
           "min_dist": torch.zeros(n, dtype=torch.float32, device=dev),
           "max_dist": torch.zeros(n, dtype=torch.float32, device=dev),
           "desc": torch.zeros((n, 32), dtype=torch.uint8, device=dev),
           "n_obs": torch.zeros(n, dtype=torch.int32, device=dev),
           "skip": torch.zeros(n, dtype=torch.uint8, device=dev),
           "mp_ids": torch.zeros(n, dtype=torch.int32, device=dev),
           "bad": torch.ones(n, dtype=torch.uint8, device=dev)}
    torch.cuda.synchronize()
    d_list, n2 = lm.local_points_device()
    assert n2 == n
    lm.gather_points_device(n, d_list, native.MapPointArrays(**{k: v.data_ptr() for k, v in src.items()}),
                            native.MapPointArrays(**{k: v.data_ptr() for k, v in dst.items()}))
    lm.get_local_points()  # synchronises the handle's stream: the gather is complete
    for k, v in host.items():
        assert np.array_equal(dst[k].cpu().numpy(), v), k
    got = search(dst, n, d_fmp, d_fobs)
    assert got[0] == ref[0] and got[0][0] > 50
    for g, w in zip(got[1:], ref[1:]):
        assert np.array_equal(g, w)
    mt.close()
