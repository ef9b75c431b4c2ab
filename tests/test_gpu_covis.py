"""The covisibility graph on the device (orbfe_map_update_connections and its companions,
native.LocalMap) against the restatement of tests/covis_cases.py: after every operation of every
script the complete graph state of every keyframe (weights in key order, the ordered list with
its weights, parent, children, flag) is read back through the getters; on the built cases, on
seeded walks and at the shapes where a kernel can break; the batch form against the same sequence
of single calls on a second handle; the error contract; and the chain update_connections ->
orbfe_map_update_local."""
import numpy as np
import pytest

import covis_cases as K
import localmap_cases as LK
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
    want = K.run_script(script) if want is None else want
    got = K.LibraryRunner(m, batch).run(script)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            state_g, state_w = (g[0], w[0]) if isinstance(g, tuple) and len(g) == 2 else (g, w)
            if isinstance(state_w, dict):
                bad = sorted(n for n in state_w if state_g.get(n) != state_w[n])[:4]
                assert not bad, (i, [(n, state_g.get(n), state_w[n]) for n in bad])
        assert g == w, i
    return want


def both(lm, lm2, script):
    """The batch form, and the same sequence as single calls on a second handle."""
    want = check(lm, script, "batch")
    check(lm2, script, "single", want)
    return want


@pytest.mark.parametrize("case", sorted(K.CASES))
def test_built_cases(lm, lm2, case):
    for v in K.VARIANTS:
        both(lm, lm2, K.CASES[case](v))


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_seeded_walks(lm, lm2, seed):
    both(lm, lm2, K.seeded_script(seed, n_ops=14))


def test_observation_sets(lm):
    """Observation sets of 0, 1, 63, 64, 65 and 200 keyframes (a wave's stride and its tail), and a
    keyframe that counts 200 neighbours."""
    want = check(lm, K.script_observation_sets())
    assert len(want[6]["R"][0]) == 200


def test_big_keyframe(lm, lm2):
    """8,192 slots (16 waves striding them), a point at 100 indices."""
    want = both(lm, lm2, K.script_big_keyframe())
    assert dict(want[0]["G"][0])["C"] == 4046


@pytest.mark.parametrize("order", ["asc", "desc", "shuffled"])
@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 130])
def test_batches(lm, lm2, n, order):
    """Batches of every keyframe of a sliding-window map, in ascending, descending and shuffled key
    order, with keyframes that have empty counters and asymmetric observations."""
    both(lm, lm2, K.script_batches(n, order, v=n % 2))


def test_partial_batches(lm, lm2):
    s = K.script_batches(70, "shuffled")[:-1]
    names = [op[1] for op in s if op[0] == "kf"]
    for k in (1, 2, 5, 64, 65):
        s.append(("update_batch", names[3:3 + k]))
        s.append(("update_batch", names[::-1][:k]))
    both(lm, lm2, s)


def test_children_counts(lm, lm2):
    """A parent that already has 0, 1, 64 and 65 children."""
    want = both(lm, lm2, K.script_children())
    assert [len(want[0][f"P{i}"][3]) for i in range(4)] == [1, 2, 65, 66]


def test_counter_capacity(lm):
    """4,096 distinct neighbours: exact.  4,097: ORBFE_ERR_CAPACITY, every keyframe's state as it
    was."""
    s = K.script_many_neighbours(K.MAX_CONNECTIONS) + [("update", "Q")]
    want = check(lm, s)
    assert len(want[0]["Q"][0]) == K.MAX_CONNECTIONS and want[0]["W"][0] == [("Q", 15)]
    s = K.script_many_neighbours(K.MAX_CONNECTIONS + 1)
    lm.clear()
    r = K.LibraryRunner(lm)
    r.run(s + [("addconn", "W", "K1", 3), ("setordered", "Q", [("K2", 9)])])
    before = r.graph()
    for batch in ([r.kf["Q"]], [r.kf["W"], r.kf["Q"], r.kf["K0"]]):
        with pytest.raises(abi.OrbfeError) as e:
            lm.UpdateConnections(batch)
        assert e.value.status == abi.ORBFE_ERR_CAPACITY
        assert r.graph() == before


def test_neighbour_capacity(lm):
    """A neighbour whose weight map holds 4,096 entries and would get a 4,097th: capacity, nothing
    changed, in the single calls and in a batch; the same neighbour when the key is already there:
    OK."""
    n = K.MAX_CONNECTIONS
    s = []
    K._kfs(s, ["Z"] + [f"K{i}" for i in range(n)], 0)
    pts = [f"p{i}" for i in range(16)]
    s += [("points", pts), ("kf", "T", K.BASE - 64, []), ("kf", "A", K.BASE - 128, pts[:15]),
          ("kf", "B", K.BASE - 192, pts), ("obs", [(p, "T") for p in pts]),
          ("setconn", "T", [(f"K{i}", 1 + i % 20) for i in range(n)])]
    lm.clear()
    r = K.LibraryRunner(lm)
    r.run(s)
    before = r.graph()
    assert len(before["T"][0]) == n
    for call in (lambda: lm.UpdateConnections(r.kf["A"]), lambda: lm.AddConnection(r.kf["T"], r.kf["A"], 15),
                 lambda: lm.UpdateConnections([r.kf["B"], r.kf["A"]])):
        with pytest.raises(abi.OrbfeError) as e:
            call()
        assert e.value.status == abi.ORBFE_ERR_CAPACITY
        assert r.graph() == before
    m = K.Model()
    for op in s:
        m.run(op)
    for op in (("eraseconn", "T", "K7"), ("addconn", "T", "A", 3), ("update", "A"), ("best", "T")):
        assert r.apply(op) == m.run(op), op
    assert ("A", 15) in m.graph()["T"][0] and len(m.graph()["T"][0]) == n


def test_single_mutators(lm):
    """Each of the four single mutators on a present key, an absent key and an equal-weight key,
    over a thresholded list."""
    base = [op for op in K.case_addconn(2)[:K.case_addconn(2).index(("addconn", "A", "B", 17))]]
    for ops in ([("addconn", "A", "B", 3)], [("addconn", "A", "Z", 40)], [("addconn", "A", "B", 17)],
                [("eraseconn", "A", "B")], [("eraseconn", "A", "Z")], [("eraseconn", "A", "D")],
                [("best", "A")], [("best", "Z")], [("addconn", "A", "B", 17), ("best", "A")],
                [("erasekf", "A")], [("erasekf", "Z")], [("setconn", "B", [("C", 15)]), ("erasekf", "A")]):
        want = check(lm, base + ops)
        assert len(want) == 1 + len(ops)


def test_hints_of_zero_clear_and_reuse():
    m = native.LocalMap(0, 0, 0)
    try:
        for v in (0, 1):
            check(m, K.script_batches(40, "shuffled", v))
            check(m, K.case_asymmetric(v))
    finally:
        m.close()


def test_bad_arguments(lm):
    lm.clear()
    r = K.LibraryRunner(lm)
    r.run(K.case_threshold(0)[:-2])
    before = r.graph()
    L = native.lib()
    n_kf = lm.size()[0]
    for slots in ([0, 1, 0], [n_kf], [-1], [2, n_kf, 3]):
        a = np.asarray(slots, np.int32)
        assert L.orbfe_map_update_connections(lm._h, len(a), abi.ptr(a), None, None, None) == abi.ORBFE_ERR_ARG
    a = np.asarray([1, 1], np.int32)
    assert L.orbfe_map_set_connections(lm._h, 0, 2, abi.ptr(a), abi.ptr(a)) == abi.ORBFE_ERR_ARG
    assert L.orbfe_map_add_connection(lm._h, 0, n_kf, 1) == abi.ORBFE_ERR_ARG
    assert L.orbfe_map_add_connection(lm._h, 0, 1, LK.MAX_KF_SLOTS + 1) == abi.ORBFE_ERR_ARG
    assert L.orbfe_map_erase_connection(lm._h, n_kf, 0) == abi.ORBFE_ERR_ARG
    assert L.orbfe_map_update_best_covisibles(lm._h, -1) == abi.ORBFE_ERR_ARG
    assert L.orbfe_map_erase_keyframe_connections(lm._h, n_kf) == abi.ORBFE_ERR_ARG
    assert r.graph() == before
    import ctypes as C
    n = C.c_int32(0)
    a = np.zeros(2, np.int32)
    s = r.kf["A"]
    assert L.orbfe_map_get_connections(lm._h, s, abi.ptr(a), abi.ptr(a), 2, C.byref(n)) == abi.ORBFE_ERR_CAPACITY
    assert n.value == 4
    assert L.orbfe_map_update_connections(lm._h, 0, None, None, None, None) == abi.ORBFE_OK


def test_set_covisibility_writes_the_ten_neighbours_only(lm):
    lm.clear()
    r = K.LibraryRunner(lm)
    r.run(K.case_threshold(0)[:-2])
    before = r.graph()
    lm.UpdateBestCovisibles(r.kf["A"], [r.kf["B"]])
    assert r.graph() == before


def test_chain_into_update_local(lm, lm2):
    """update_connections, then orbfe_map_update_local, against a second handle that is fed the
    restatement's lists through set_covisibility / set_parent / set_children."""
    for v in (0, 1):
        s = K.script_batches(30, "shuffled", v)
        frame = [op[3][0] for op in s if op[0] == "kf" and op[3]][:6]
        lm.clear()
        lm2.clear()
        m = K.Model()
        r, r2 = K.LibraryRunner(lm), LK.LibraryRunner(lm2)
        for op in s:
            m.run(op)
            r.apply(op)
            if op[0] not in K.OPS:
                r2.apply(op)
        g = m.graph()
        for n, (_, ordered, parent, children, _) in g.items():
            r2.apply(("covis", n, [o for o, _ in ordered]))
            r2.apply(("parent", n, parent))
            r2.apply(("children", n, children))
        for fid in (5, 6):
            want = m.update(fid, frame)
            got = r.apply(("localmap", fid, frame))
            got2 = r2.apply(("update", fid, frame))
            assert got == want and got2 == want
            assert len(want[0]) > len({n for p in frame for n in m.mps[p].obs})   # neighbours were added
