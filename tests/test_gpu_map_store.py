"""The seams of the device map's store (csrc/orbfe_map_store.hip) crossed on a handle made with
hints of zero: the keyframe columns at 16 -> 17 and 32 -> 33, the point columns at 1,024 -> 1,025,
kf_mp's pool at its first 4,096 ints with keyframe features in its side pools, a covisibility row
at 8 -> 16 entries and the graph's pool at its first 65,536 ints; with the covisibility and culling
groups made before the crossing (they grow with their contents) and after it (they catch up with
the map as it then is); then clear and the same script again on the same handle.  Every expected
value is the restatement's (tests/culling_cases.py)."""
import pytest

import culling_cases as Q
from orbslam_mapsave_amd import native

pytestmark = pytest.mark.gpu

KEY0 = 0x7f3a00000000


def replay(lm, script):
    """The script on the restatement and on the library, answer by answer; then what no script
    answer holds: every keyframe's features, every stamp, the counters of every point."""
    model, r = Q.Model(), Q.LibraryRunner(lm, "batch")
    answers = []
    for i, op in enumerate(script):
        want, got = model.run(op), r.apply(op)
        assert got == want, (i, op[0])
        answers.append(want)
    for n, kf in model.kfs.items():
        o, right, d, th = lm.get_keyframe_features(r.kf[n])
        assert [int(x) for x in o] == list(kf.octave), n
        assert [bool(x) for x in right] == list(kf.right), n
        assert Q._bits(d) == Q._bits(kf.depth) and float(th) == kf.th_depth, n
    kn, pn = r.kf_names, r.mp_names
    assert [int(v) for v in lm.get_stamps(0, list(range(len(kn))))] == [model.kfs[n].stamp for n in kn]
    assert [int(v) for v in lm.get_stamps(1, list(range(len(pn))))] == [model.mps[n].stamp for n in pn]
    o, f, v, first = lm.get_point_counters(list(range(len(pn))))
    assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(o, f, v, first)] == \
        [(model.mps[n].nobs, model.mps[n].found, model.mps[n].visible, model.mps[n].first) for n in pn]
    return answers


def _keyframes(s, names, pts, start):
    """Keyframes that all hold `pts`; returns the observations, one with its index per slot."""
    for i, n in enumerate(names):
        s.append(("kf", n, KEY0 + 64 * (997 * (start + i) % 1009), list(pts)))
    return [(p, n, j) for n in names for j, p in enumerate(pts)]


def _touch(s, names, pts, tag):
    """Covisibility and culling calls on `names`: connections and the spanning tree, an erase
    flag, features, counters, stamps."""
    s.append(("update_batch", list(names)))
    s.append(("noterase", names[1], True))
    for i, n in enumerate(names[:3]):
        s.append(("features", n, [(i + j) % 8 for j in range(len(pts))],
                  [float(j) if (i + j) % 3 == 0 else -1.0 for j in range(len(pts))],
                  [0.25 * j + i for j in range(len(pts))], 30.0 + i))
    s.append(("counters", pts[:6], None, [5 + tag] * 6, [9] * 6, [2] * 6))
    s.append(("stamps", "kf", list(names[:2]), [100 + tag, 200 + tag]))
    s.append(("stamps", "mp", pts[:3], [7, 8, 9 + tag]))


def column_script(groups_first):
    """34 keyframes and 1,100 points on capacities of 16 and 1,024.  groups_first: the covisibility
    and the culling group exist before each crossing and grow with their contents; else their
    first calls (an observation is one) come after the last crossing and they cover the map as it
    then is."""
    shared = [f"p{j}" for j in range(20)]
    under, above = [f"q{j}" for j in range(1000)], [f"r{j}" for j in range(80)]
    a, b, c = ([f"K{i}" for i in range(lo, hi)] for lo, hi in ((0, 16), (16, 32), (32, 34)))
    s = [("points", shared)]
    if groups_first:
        s.append(("obsidx", _keyframes(s, a, shared, 0)))
        _touch(s, a, shared, 0)
        s.append(("obsidx", _keyframes(s, b, shared, 16)))               # 16 -> 17
        _touch(s, b, shared, 1)
        s.append(("obsidx", _keyframes(s, c, shared, 32)))               # 32 -> 33
        _touch(s, c + ["K0"], shared, 2)
        s.append(("points", under))                                      # 1,020 points: under the seam
        s.append(("counters", under[-3:], [4, 5, 6], [2, 3, 4], [7, 8, 9], [1, 2, 3]))
        s.append(("points", above))                                      # 1,024 -> 1,025
    else:
        obs = _keyframes(s, a, shared, 0) + _keyframes(s, b, shared, 16) + _keyframes(s, c, shared, 32)
        s.append(("points", under))
        s.append(("points", above))
        s.append(("obsidx", obs))
        _touch(s, a[:2] + b[:2] + c, shared, 0)
    top = above[60:]
    s.append(("kf", "Z", KEY0 + 64 * 2000, top))
    s.append(("obsidx", [(p, "Z", j) for j, p in enumerate(top)]))
    s.append(("counters", top[:4], None, [0, 1, 1, 1], [9, 9, 1, 1], [0, 0, 0, 5]))
    s.append(("cullpoints", top[:6] + shared[:4], 6, False))             # a point above the seam culled
    s.append(("localmap", 11, top[4:8] + [None, shared[5]]))
    s.append(("kfbadflag", "K17"))
    s.append(("tracked", "Z", 0))
    return s


@pytest.mark.parametrize("groups_first", [True, False])
def test_column_seams_clear_and_reuse(groups_first):
    m = native.LocalMap(0, 0, 0)
    try:
        s = column_script(groups_first)
        first = replay(m, s)
        assert first[-4][0][1]                      # cull_points culled something above the seam
        m.clear()
        assert replay(m, s) == first
    finally:
        m.close()


def pool_script():
    """kf_mp's pool over its first 4,096 ints after features were set; a covisibility row from 8 to
    16 entries and the graph's pool over its first 65,536 ints after a keyframe was connected."""
    pts = [f"p{j}" for j in range(30)]
    s = [("points", pts)]
    small = [f"K{i}" for i in range(4)]
    for i, n in enumerate(small):
        s.append(("kf", n, KEY0 + 64 * (i + 1), pts[:10 + i]))           # regions of 16 ints
        s.append(("features", n, [(i + j) % 8 for j in range(10 + i)], [float(j % 2) - 0.5 for j in range(10 + i)],
                  [1.5 * j for j in range(10 + i)], 20.0 + i))
    s.append(("kf", "BIG", KEY0 + 64 * 900, [pts[j % 30] if j % 100 == 0 else None for j in range(4090)]))
    s.append(("kf", "AFTER", KEY0 + 64 * 901, pts[:12]))                  # reads defaults
    many = [f"N{i}" for i in range(300)]
    for i, n in enumerate(many):
        s.append(("kf", n, KEY0 + 64 * (1000 + (i * 7919) % 1201), []))
    s.append(("setconn", "K0", [(n, 3 + i) for i, n in enumerate(many[:8])]))   # a region of 8
    s.append(("best", "K0"))
    s.append(("addconn", "K0", many[8], 40))                             # 8 -> 16, contents kept
    return s, many


def test_pool_seams_clear_and_reuse():
    m = native.LocalMap(0, 0, 0)
    try:
        s, many = pool_script()
        # 33 rows of 257 and more entries: regions of 4 x 512 ints, 67,584 in all, set without
        # reading the graph back after each; the addconn that closes the script reads all of it
        rows = [("setconn", many[i], [(o, 1 + (i + j) % 50) for j, o in enumerate(many) if j != i][:257 + i])
                for i in range(33)]
        for round_ in (0, 1):
            model, r = Q.Model(), Q.LibraryRunner(m, "batch")
            for i, op in enumerate(s):
                assert r.apply(op) == model.run(op), (i, op[0])
            k0 = model.graph()["K0"]
            assert len(k0[0]) == 9 and len(k0[1]) == 9
            for op in rows:
                model.kfs[op[1]].weights = dict(op[2])
                m.set_connections(r.kf[op[1]], [r.kf[o] for o, _ in op[2]], [w for _, w in op[2]])
            last = ("addconn", many[40], "K0", 5)
            want = model.run(last)
            assert r.apply(last) == want
            assert want["K0"][:2] == k0[:2]                              # unchanged across the crossing
            for n in ("K0", "K3", "BIG", "AFTER"):
                kf = model.kfs[n]
                o, right, d, th = m.get_keyframe_features(r.kf[n])
                assert [int(x) for x in o] == list(kf.octave) and [bool(x) for x in right] == list(kf.right), n
                assert Q._bits(d) == Q._bits(kf.depth) and float(th) == kf.th_depth, n
            assert not model.kfs["AFTER"].right[0] and model.kfs["K3"].octave[5] == 0  # (3 + 5) % 8
            m.clear()
    finally:
        m.close()
