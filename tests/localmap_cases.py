"""Tracking::UpdateLocalMap restated in plain Python from the reference's lines
(Tracking.cc:1455-1599: UpdateLocalKeyFrames :1491-1599, UpdateLocalPoints :1465-1488) over a
scripted map model, with branch counters and single-decision mutants; the built cases that
tests/test_localmap.py proves non-trivial and tests/test_gpu_localmap.py runs against the library;
and the driver that replays a script on a ``native.LocalMap``.

A script is a list of operations on keyframes and map points named by strings:
    ("points", [names])                     new MapPoints
    ("kf", name, key, [point names|None])   a new KeyFrame at heap address `key`, its mvpMapPoints
    ("kfpoints", name, first, [names|None]) KeyFrame::AddMapPoint / EraseMapPointMatch
    ("kfbad", name, flag)                   KeyFrame::SetBadFlag
    ("covis", name, [names|None])           mvpOrderedConnectedKeyFrames, whole (None: a keyframe
                                            the mirror does not hold); the reference reads 10
    ("children", name, [names])             mspChildrens
    ("parent", name, parent|None)           mpParent
    ("mpbad", [names], flag)                MapPoint::SetBadFlag
    ("obs", [(point, kf), ...])             MapPoint::AddObservation
    ("unobs", [(point, kf), ...])           MapPoint::EraseObservation
    ("stamps", kind, [names], [values])     mnTrackReferenceForFrame, kind "kf" or "mp"
    ("setlocal", [kf names], ref|None)      mvpLocalKeyFrames / mpReferenceKF assigned
    ("clear",)                              Tracking::Reset
    ("update", frame_id, [names|None])      UpdateLocalMap with mCurrentFrame.mvpMapPoints
An update's answer is (local keyframes, reference keyframe, local points, frame points after,
keyframe stamps, point stamps), everything by name.
"""
from __future__ import annotations

import random

MUTANTS = ("kf_order_slot", "child_order_slot", "max_ge", "bad_kf_max", "bad_kf_listed",
           "limit_ge", "phase2_visits_appended", "neigh_no_break", "neigh_11", "parent_bad_test",
           "parent_break_inner", "empty_clears", "bad_point_kept", "bad_point_votes",
           "point_stamp_ignored", "point_last_wins", "bad_point_listed", "bad_kf_points_skipped")

MAX_VOTED = 4096      # ORBFE_MAP_MAX_VOTED
MAX_KF_SLOTS = 8192   # ORBFE_MAP_MAX_KF_SLOTS


def _bump(stats, key):
    if stats is not None:
        stats[key] = stats.get(key, 0) + 1


class KF:
    def __init__(self, name, key, slot, mps):
        self.name, self.key, self.slot = name, key, slot
        self.bad = False
        self.stamp = 0          # mnTrackReferenceForFrame (KeyFrame.cc:35)
        self.mps = list(mps)
        self.conn = []
        self.children = set()
        self.parent = None


class MP:
    def __init__(self, name, slot):
        self.name, self.slot = name, slot
        self.bad = False
        self.stamp = 0          # mnTrackReferenceForFrame (MapPoint.cc:36)
        self.obs = set()


class Model:
    def __init__(self):
        self.clear()

    def clear(self):
        self.kfs, self.mps = {}, {}
        self.local, self.ref = [], None

    def apply(self, op):
        k = op[0]
        if k == "points":
            for n in op[1]:
                assert n not in self.mps
                self.mps[n] = MP(n, len(self.mps))
        elif k == "kf":
            assert op[1] not in self.kfs and all(op[2] != f.key for f in self.kfs.values())
            self.kfs[op[1]] = KF(op[1], op[2], len(self.kfs), op[3])
        elif k == "kfpoints":
            self.kfs[op[1]].mps[op[2]:op[2] + len(op[3])] = op[3]
        elif k == "kfbad":
            self.kfs[op[1]].bad = bool(op[2])
        elif k == "covis":
            self.kfs[op[1]].conn = list(op[2])
        elif k == "children":
            self.kfs[op[1]].children = set(op[2])
        elif k == "parent":
            self.kfs[op[1]].parent = op[2]
        elif k == "mpbad":
            for n in op[1]:
                self.mps[n].bad = bool(op[2])
        elif k == "obs":
            for p, f in op[1]:
                self.mps[p].obs.add(f)
        elif k == "unobs":
            for p, f in op[1]:
                self.mps[p].obs.discard(f)
        elif k == "stamps":
            t = self.kfs if op[1] == "kf" else self.mps
            for n, v in zip(op[2], op[3]):
                t[n].stamp = v
        elif k == "setlocal":
            self.local, self.ref = list(op[1]), op[2]
        elif k == "clear":
            self.clear()
        else:
            raise ValueError(k)

    # ---- Tracking.cc:1491-1599
    def update_local_keyframes(self, fid, frame, mutant=None, st=None):
        counter = {}
        for i, name in enumerate(frame):                                   # :1495
            if name is None:
                _bump(st, "frame_null")
                continue
            mp = self.mps[name]
            if not mp.bad or mutant == "bad_point_votes":                  # :1500
                _bump(st, "frame_live")
                for f in mp.obs:                                           # :1503
                    counter[f] = counter.get(f, 0) + 1
                    _bump(st, "vote")
            if mp.bad:
                _bump(st, "frame_bad")
                if mutant != "bad_point_kept":
                    frame[i] = None                                        # :1508
        if not counter:                                                    # :1513
            _bump(st, "empty_return")
            if mutant == "empty_clears":
                self.local = []
            return
        mx, kfmax = 0, None
        self.local = []                                                    # :1519
        by = (lambda n: self.kfs[n].slot) if mutant == "kf_order_slot" else (lambda n: self.kfs[n].key)
        for name in sorted(counter, key=by):                               # :1523, pointer order
            kf, c = self.kfs[name], counter[name]
            if kf.bad:                                                     # :1527
                _bump(st, "p1_bad")
                if mutant == "bad_kf_max" and c > mx:
                    mx, kfmax = c, name
                if mutant == "bad_kf_listed":
                    self.local.append(name)
                    kf.stamp = fid
                continue
            if c > mx or (mutant == "max_ge" and c >= mx):                 # :1530
                _bump(st, "p1_newmax")
                mx, kfmax = c, name
            elif c == mx:
                _bump(st, "p1_tie")
            else:
                _bump(st, "p1_below")
            self.local.append(name)                                        # :1536
            kf.stamp = fid
        if not self.local:
            _bump(st, "p1_all_bad")
        n1 = len(self.local)                                               # itEndKF, taken once (:1542)
        it = 0
        while it < (len(self.local) if mutant == "phase2_visits_appended" else n1):
            if len(self.local) >= 80 if mutant == "limit_ge" else len(self.local) > 80:   # :1545
                _bump(st, "limit_break")
                break
            kf = self.kfs[self.local[it]]
            it += 1
            before = len(self.local)
            for nb in kf.conn[:11 if mutant == "neigh_11" else 10]:        # :1550
                if nb is None:
                    _bump(st, "neigh_absent")
                    continue
                n = self.kfs[nb]
                if n.bad:                                                  # :1555
                    _bump(st, "neigh_bad")
                    continue
                if n.stamp == fid:                                         # :1557
                    _bump(st, "neigh_stamped")
                    continue
                _bump(st, "neigh_pushed")
                self.local.append(nb)
                n.stamp = fid
                if mutant != "neigh_no_break":
                    break                                                  # :1561
            if len(self.local) == before:
                _bump(st, "neigh_none")
            before = len(self.local)
            cby = (lambda n: self.kfs[n].slot) if mutant == "child_order_slot" else (lambda n: self.kfs[n].key)
            for ch in sorted(kf.children, key=cby):                        # :1567, pointer order
                c = self.kfs[ch]
                if c.bad:                                                  # :1570
                    _bump(st, "child_bad")
                    continue
                if c.stamp == fid:                                         # :1572
                    _bump(st, "child_stamped")
                    continue
                _bump(st, "child_pushed")
                self.local.append(ch)
                c.stamp = fid
                break                                                      # :1576
            if len(self.local) == before:
                _bump(st, "child_none")
            if kf.parent is None:                                          # :1582
                _bump(st, "parent_none")
                continue
            p = self.kfs[kf.parent]
            if p.stamp == fid:                                             # :1584
                _bump(st, "parent_stamped")
                continue
            if mutant == "parent_bad_test" and p.bad:
                continue
            _bump(st, "parent_bad_pushed" if p.bad else "parent_pushed")
            self.local.append(kf.parent)
            p.stamp = fid
            if mutant != "parent_break_inner":
                break                                                      # :1588: the whole loop
        if kfmax is not None:                                              # :1594
            _bump(st, "ref_set")
            self.ref = kfmax
        else:
            _bump(st, "ref_kept")

    # ---- Tracking.cc:1465-1488
    def update_local_points(self, fid, mutant=None, st=None):
        pts = []
        for name in self.local:                                            # :1469
            kf = self.kfs[name]
            if kf.bad:
                _bump(st, "pt_kf_bad")
                if mutant == "bad_kf_points_skipped":
                    continue
            for mpn in kf.mps:                                             # :1474
                if mpn is None:                                            # :1477
                    _bump(st, "pt_null")
                    continue
                mp = self.mps[mpn]
                if mp.stamp == fid and mutant not in ("point_stamp_ignored", "point_last_wins"):
                    _bump(st, "pt_stamped")                                # :1479
                    continue
                if mp.bad and mutant != "bad_point_listed":                # :1481
                    _bump(st, "pt_bad")
                    continue
                _bump(st, "pt_pushed")
                pts.append(mpn)
                if mutant != "point_last_wins":
                    mp.stamp = fid                                         # :1484
        if mutant == "point_last_wins":
            last = {n: i for i, n in enumerate(pts)}
            pts = [n for i, n in enumerate(pts) if last[n] == i]
            for n in pts:
                self.mps[n].stamp = fid
        return pts

    def update(self, fid, frame, mutant=None, st=None):
        frame = list(frame)
        self.update_local_keyframes(fid, frame, mutant, st)
        pts = self.update_local_points(fid, mutant, st)
        return (list(self.local), self.ref, pts, frame,
                {n: f.stamp for n, f in self.kfs.items()}, {n: p.stamp for n, p in self.mps.items()})


def run_script(script, mutant=None, stats=None):
    """The answers of the script's updates, in order."""
    m, out = Model(), []
    for op in script:
        if op[0] == "update":
            out.append(m.update(op[1], op[2], mutant, stats))
        else:
            m.apply(op)
    return out


class LibraryRunner:
    """Replays a script on a ``native.LocalMap`` (names <-> slots).  `update` is
    ``lambda lm, fid, frame_slots -> (kf slots, ref slot, point slots, frame slots after)``, the
    host form by default."""

    def __init__(self, lm, update=None):
        self.lm = lm
        self.update = update or (lambda lm, fid, f: lm.UpdateLocalMap(fid, f))
        self.kf, self.mp, self.kf_names, self.mp_names = {}, {}, [], []

    def _mps(self, names):
        return [-1 if n is None else self.mp[n] for n in names]

    def apply(self, op):
        k, lm = op[0], self.lm
        if k == "points":
            first = lm.add_points(len(op[1]))
            for i, n in enumerate(op[1]):
                self.mp[n] = first + i
                self.mp_names.append(n)
            assert first + len(op[1]) == len(self.mp_names)
        elif k == "kf":
            s = lm.add_keyframe(op[2], len(op[3]), self._mps(op[3]))
            assert s == len(self.kf_names)
            self.kf[op[1]] = s
            self.kf_names.append(op[1])
        elif k == "kfpoints":
            lm.set_keyframe_points(self.kf[op[1]], op[2], self._mps(op[3]))
        elif k == "kfbad":
            lm.SetBadFlag(self.kf[op[1]], op[2])
        elif k == "covis":
            lm.UpdateBestCovisibles(self.kf[op[1]], [-1 if n is None else self.kf[n] for n in op[2][:10]])
        elif k == "children":
            lm.set_children(self.kf[op[1]], [self.kf[n] for n in op[2]])
        elif k == "parent":
            lm.set_parent(self.kf[op[1]], -1 if op[2] is None else self.kf[op[2]])
        elif k == "mpbad":
            lm.SetBadFlagPoints(self._mps(op[1]), op[2])
        elif k == "obs":
            lm.AddObservation([self.mp[p] for p, _ in op[1]], [self.kf[f] for _, f in op[1]])
        elif k == "unobs":
            lm.EraseObservation([self.mp[p] for p, _ in op[1]], [self.kf[f] for _, f in op[1]])
        elif k == "stamps":
            t = self.kf if op[1] == "kf" else self.mp
            lm.set_stamps(0 if op[1] == "kf" else 1, [t[n] for n in op[2]], op[3])
        elif k == "setlocal":
            lm.set_local_keyframes([self.kf[n] for n in op[1]], -1 if op[2] is None else self.kf[op[2]])
        elif k == "clear":
            lm.clear()
            self.kf, self.mp, self.kf_names, self.mp_names = {}, {}, [], []
        elif k == "update":
            kfs, ref, pts, frame = self.update(lm, op[1], self._mps(op[2]))
            ks = lm.get_stamps(0, list(range(len(self.kf_names))))
            ps = lm.get_stamps(1, list(range(len(self.mp_names))))
            return ([self.kf_names[s] for s in kfs], None if ref < 0 else self.kf_names[ref],
                    [self.mp_names[s] for s in pts],
                    [None if s < 0 else self.mp_names[s] for s in frame],
                    {n: int(v) for n, v in zip(self.kf_names, ks)},
                    {n: int(v) for n, v in zip(self.mp_names, ps)})
        else:
            raise ValueError(k)
        return None

    def run(self, script):
        return [a for a in (self.apply(op) for op in script) if a is not None]


# ---- built cases ---------------------------------------------------------------------------
BASE = 0x7f3a00000000


def keys_for(n, v):
    """n distinct heap-like addresses; the order against the slots depends on the variant:
    opposite (even variants) or shuffled."""
    idx = list(range(n))
    if v % 2 == 0:
        idx.reverse()
    else:
        random.Random(100 + v).shuffle(idx)
    return [BASE + 0x1d0 * (i + 1) for i in idx]


def _world(s, nkf, v, pts_per_kf=3):
    """nkf keyframes K0.. with private points Ki_j, each observed by its keyframe."""
    keys = keys_for(nkf, v)
    names = []
    for i in range(nkf):
        ps = [f"K{i}_{j}" for j in range(pts_per_kf)]
        s.append(("points", ps))
        s.append(("kf", f"K{i}", keys[i], ps))
        s.append(("obs", [(p, f"K{i}") for p in ps]))
        names.append(f"K{i}")
    return names


def case_votes(v):
    """Order by key, ties, the strict maximum, bad keyframes voted for, bad and NULL frame points,
    the empty return, the same frame id twice."""
    s = []
    _world(s, 6, v)
    s.append(("points", ["S0", "S1", "S2", "B0", "B1"]))
    # S0 seen by K1, K3 (tie at the top together with their own points), S1 by K5 (bad, most votes)
    s.append(("obs", [("S0", "K1"), ("S0", "K3"), ("S1", "K5"), ("S2", "K5"), ("B0", "K4"), ("B1", "K2")]))
    s.append(("kfpoints", "K1", 1, ["S0"]))
    s.append(("kfpoints", "K3", 0, ["S0", None]))
    s.append(("kfbad", "K5", True))
    s.append(("mpbad", ["B0", "B1"], True))
    s.append(("kfpoints", "K0", 2, ["B1"]))
    f1 = ["K1_0", None, "S0", "K3_0", "B0", "K5_0", "S1", "S2", "K0_0"]
    s.append(("update", 10 + v, f1))
    s.append(("update", 10 + v, f1))                      # the same frame id: every point is stamped
    s.append(("update", 20 + v, [None, "B0", None]))      # empty vote: the old list, new stamps
    s.append(("update", 30 + v, ["K5_0", "K5_1", "B1"]))  # every voted keyframe bad
    s.append(("update", 40 + v, ["B0"] + ([] if v % 3 else ["K2_0"])))
    s.append(("update", 50 + v, ["K0_0", "K2_1", "K4_2", "K4_1"]))
    s.append(("update", 0, ["K0_0"]))                     # frame id 0: the stamp of a new object
    return s


def case_neighbours(v):
    """The covisibility loop: absent, bad and stamped neighbours, the first eligible one, its
    break, the 11th entry; appended keyframes are not visited."""
    s = []
    _world(s, 14, v, pts_per_kf=2)
    s.append(("kfbad", "K6", True))
    # K0: absent, bad, stamped (K1 is voted), then K7, K8 both eligible: only K7
    s.append(("covis", "K0", [None, "K6", "K1", "K7", "K8"]))
    # K1: ten entries that cannot be taken, the 11th could
    s.append(("covis", "K1", [None, "K6", "K0", "K2", None, "K6", "K0", "K2", "K6", None, "K9"]))
    # K2: nothing to take at all
    s.append(("covis", "K2", ["K0", "K1"] if v % 2 else []))
    # K7 (appended) has an eligible neighbour no voted keyframe names
    s.append(("covis", "K7", ["K10"]))
    s.append(("covis", "K8", ["K11"]))
    s.append(("kfpoints", "K7", 0, ["K0_0"]))
    s.append(("update", 5 + v, ["K0_0", "K1_0", "K2_0", "K1_1"]))
    s.append(("covis", "K2", ["K12", "K13"][: 1 + v % 2]))
    s.append(("update", 15 + v, ["K0_0", "K1_0", "K2_0", "K2_1"]))
    s.append(("update", 15 + v, ["K0_0", "K2_0"]))         # again: K7, K12 are stamped, K8 is next
    return s


def case_family(v):
    """Children in key order, bad and stamped children, the parent without an isBad test and its
    break of the whole loop, at the first iteration and later."""
    s = []
    # slot order against key order: A < B < C by key, C, B, A by slot; E1 < E2 by key, E2, E1 by slot
    spec = [("C", 30), ("B", 20), ("A", 10), ("E2", 50), ("E1", 40), ("XB", 5), ("NA", 60),
            ("NB", 61), ("NC", 62), ("CC", 63), ("PB", 64), ("P2", 65)]
    npts = 1 + v % 3
    for name, rank in spec:
        ps = [f"{name}_{j}" for j in range(npts)]
        s.append(("points", ps))
        s.append(("kf", name, BASE + (0x90 + 16 * v) * rank, ps))
        s.append(("obs", [(p, name) for p in ps]))
    frame = ["C_0", "A_0", "B_0"]
    # A's children by key: a bad one, a stamped one (B is voted), then E1 before E2
    s.append(("kfbad", "XB", True))
    s.append(("children", "A", ["E2", "XB", "E1", "B"]))
    s.append(("covis", "A", ["NA"]))
    s.append(("covis", "B", ["NB"]))
    s.append(("covis", "C", ["NC"]))
    s.append(("children", "C", ["CC"]))
    # B's parent is bad and unstamped: pushed, and the loop ends before C
    s.append(("kfbad", "PB", True))
    s.append(("parent", "B", "PB"))
    s.append(("parent", "A", "B"))                          # stamped in phase 1: no push, no break
    s.append(("update", 7 + v, frame))
    # now a parent sits at the first iteration: three pushes, then the break
    s.append(("parent", "A", "P2"))
    s.append(("update", 17 + v, frame))
    # and nobody has an unstamped parent: every iteration runs
    s.append(("parent", "A", None))
    s.append(("parent", "B", "C"))
    s.append(("children", "B", ["XB"]))
    s.append(("update", 27 + v, frame + ["C_0"]))
    return s


def case_gate(v):
    """The `> 80` gate on both sides: 78 .. 81 voted keyframes with neighbours, children and a
    parent available, including an iteration that pushes three entries."""
    s = []
    nv = 81
    names = _world(s, nv + 12, v, pts_per_kf=1)
    keys = keys_for(nv + 12, v)
    extra = names[nv:]
    for n_voted, fid in ((78, 100), (79, 200), (80, 300), (81, 400), (79, 500)):
        voted = sorted(names[:n_voted], key=lambda n: keys[int(n[1:])])
        if fid == 500:  # the first keyframe also has a parent: three pushes, then the break
            s.append(("parent", voted[0], extra[6 + v % 3]))
        for j, n in enumerate(voted[:3]):
            s.append(("covis", n, [extra[2 * j]]))
            s.append(("children", n, [extra[2 * j + 1]]))
        s.append(("update", fid + v, [f"{n}_0" for n in names[:n_voted]]))
        for n in voted[:3]:
            s.append(("covis", n, []))
            s.append(("children", n, []))
    return s


def case_points(v):
    """UpdateLocalPoints: first occurrence wins, in list and slot order; NULL, stamped and bad
    points; a bad keyframe's points are listed; a point held by every local keyframe."""
    s = []
    _world(s, 5, v, pts_per_kf=4)
    s.append(("points", ["ALL", "X", "Y", "BAD", "OLD"]))
    for i in range(5):
        s.append(("kfpoints", f"K{i}", 1, ["ALL"]))
    s.append(("kfpoints", "K0", 3, ["X"]))
    s.append(("kfpoints", "K1", 0, ["Y"]))
    s.append(("kfpoints", "K2", 2, ["X" if v % 2 else "Y", "BAD"]))
    s.append(("kfpoints", "K3", 2, [None, "OLD"]))
    s.append(("mpbad", ["BAD"], True))
    s.append(("stamps", "mp", ["OLD"], [60 + v]))
    s.append(("obs", [("ALL", f"K{i}") for i in range(4)]))
    s.append(("kfbad", "K4", True))
    s.append(("parent", "K3", "K4"))                        # K4: bad, pushed as a parent
    s.append(("update", 60 + v, ["ALL", "K0_0", None]))
    s.append(("setlocal", ["K2", "K0", "K2"], "K2"))        # assigned list, a keyframe twice
    s.append(("update", 70 + v, [None]))
    s.append(("unobs", [("ALL", "K0"), ("ALL", "K3")]))
    s.append(("obs", [("ALL", "K1")]))                      # already there: no second vote
    s.append(("update", 80 + v, ["ALL", "ALL", "K1_0"]))    # two keypoints hold one point: two votes
    s.append(("clear",))
    _world(s, 2, v)
    s.append(("update", 80 + v, ["K1_0"]))
    return s


CASES = {"votes": case_votes, "neighbours": case_neighbours, "family": case_family,
         "gate": case_gate, "points": case_points}
VARIANTS = range(6)


def built_scripts():
    for name, fn in CASES.items():
        for v in VARIANTS:
            yield f"{name}-{v}", fn(v)


def seeded_script(seed, n_ops=60, nkf=40, npts=300, slots=24):
    """A random map and a random walk of mutations and updates."""
    r = random.Random(seed)
    s = []
    pts = [f"p{i}" for i in range(npts)]
    s.append(("points", pts))
    keys = r.sample(range(1, 1 << 20), nkf)
    kfs = [f"k{i}" for i in range(nkf)]
    for i, n in enumerate(kfs):
        mps = [r.choice(pts) if r.random() < 0.8 else None for _ in range(r.randrange(0, slots))]
        s.append(("kf", n, BASE + 16 * keys[i], mps))
        s.append(("obs", [(p, n) for p in mps if p is not None]))
    for n in kfs:
        s.append(("covis", n, [r.choice(kfs + [None]) for _ in range(r.randrange(0, 13))]))
        s.append(("children", n, r.sample(kfs, r.randrange(0, 4))))
        s.append(("parent", n, r.choice(kfs + [None, None])))
    fid = 1
    for _ in range(n_ops):
        c = r.random()
        if c < 0.15:
            s.append(("kfbad", r.choice(kfs), r.random() < 0.7))
        elif c < 0.3:
            s.append(("mpbad", r.sample(pts, 5), r.random() < 0.7))
        elif c < 0.4:
            s.append(("unobs", [(r.choice(pts), r.choice(kfs)) for _ in range(8)]))
        elif c < 0.5:
            s.append(("obs", [(r.choice(pts), r.choice(kfs)) for _ in range(8)]))
        else:
            fid += r.randrange(0, 2)
            s.append(("update", fid, [r.choice(pts) if r.random() < 0.7 else None
                                      for _ in range(r.choice((0, 1, 3, 20, 63, 64, 65)))]))
    return s


# ---- the shapes at which a kernel can break (tests/test_gpu_localmap.py) ------------------------
def script_many_keyframes(nv, extra=3):
    """nv voted keyframes, one point each, keys against slots; K0's point is seen by all."""
    s = []
    names = _world(s, nv + extra, 0, pts_per_kf=1)
    s.append(("covis", names[0], [names[nv]] if extra else []))
    s.append(("update", 9, [f"{n}_0" for n in names[:nv]]))
    s.append(("update", 11, [f"{names[1]}_0"] if nv > 1 else []))
    return s


def script_observation_sets(sizes=(0, 1, 63, 64, 65, 200), v=1):
    """One point per observation-set size; frames of 0, 1, 63, 64, 65 and 257 keypoints."""
    s = []
    nkf = max(sizes)
    names = _world(s, nkf, v, pts_per_kf=1)
    pts = [f"O{n}" for n in sizes]
    s.append(("points", pts))
    for p, n in zip(pts, sizes):
        s.append(("obs", [(p, names[(7 * i) % nkf]) for i in range(n)]))
    fid = 3
    for p in pts:
        s.append(("update", fid, [p]))
        fid += 1
    for n in (0, 1, 63, 64, 65, 257):
        s.append(("update", fid, [(pts + [None, "K0_0", "K5_0"])[(i * 5) % (len(pts) + 3)] for i in range(n)]))
        fid += 1
    return s


def script_children(counts=(0, 1, 64, 65), v=0):
    """A keyframe with 0, 1, 64 and 65 children of which only the last in key order is eligible."""
    s = []
    total = sum(counts) + len(counts)
    names = _world(s, total, v, pts_per_kf=1)
    keys = keys_for(total, v)
    heads, rest = names[:len(counts)], names[len(counts):]
    frame = []
    for h, c in zip(heads, counts):
        ch, rest = rest[:c], rest[c:]
        s.append(("children", h, ch))
        for x in sorted(ch, key=lambda n: keys[int(n[1:])])[:-1]:
            s.append(("kfbad", x, True))
        frame.append(f"{h}_0")
    s.append(("update", 21, frame))
    s.append(("update", 21, frame))
    return s


def script_point_lists(block=1024):
    """Local point lists that end one below, on and one above the compaction block and twice it,
    and a keyframe of 8192 slots."""
    s = []
    n = 2 * block + 1
    pts = [f"q{i}" for i in range(MAX_KF_SLOTS)]
    s.append(("points", pts))
    fid = 31
    for i, m in enumerate((block - 1, block, block + 1, 2 * block - 1, 2 * block, n, MAX_KF_SLOTS)):
        s.append(("kf", f"L{i}", BASE - 64 * (i + 1), pts[:m]))
        s.append(("obs", [(pts[0], f"L{i}")]))
        s.append(("setlocal", [f"L{i}"], None))
        s.append(("update", fid, []))
        fid += 1
    s.append(("update", fid, [pts[0]]))     # all seven: the first claims everything it holds
    return s
