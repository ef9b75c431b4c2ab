"""The covisibility graph restated in plain Python from the reference's lines (KeyFrame.cc:
UpdateConnections :1010-1100, AddConnection :844-857, UpdateBestCovisibles :859-878,
GetCovisiblesByWeight :905-920, the connection part of SetBadFlag :1188-1199, EraseConnection
:1295-1309) over the scripted map model of tests/localmap_cases.py, with branch counters and
single-decision mutants; the closed form of a sequential batch as a pure function; the built cases
that tests/test_covis.py proves non-trivial and tests/test_gpu_covis.py runs against the library;
and the driver that replays a script on a ``native.LocalMap``.

The script operations of localmap_cases that build a map (points, kf, kfpoints, kfbad, mpbad, obs,
unobs, children, parent, clear) are kept; its "update" is ("localmap", frame_id, frame) here.  New:
    ("update", name[, allow])               KeyFrame::UpdateConnections; allow = `mnId != 0`
                                            (default: the keyframe is not the map's first)
    ("update_batch", [names][, [allow]])    the same on every name, in that order
    ("addconn", name, other, weight)        AddConnection
    ("eraseconn", name, other)              EraseConnection
    ("best", name)                          UpdateBestCovisibles
    ("erasekf", name)                       the connection part of SetBadFlag
    ("setconn", name, [(other, weight)])    mConnectedKeyFrameWeights assigned
    ("setordered", name, [(other, weight)]) mvpOrderedConnectedKeyFrames / mvOrderedWeights assigned
    ("setfirst", name, flag)                mbFirstConnection
    ("byweight", name, w)                   GetCovisiblesByWeight
The answer of each of them is the whole graph state of every keyframe afterwards (``graph``);
byweight answers (state, the returned list); localmap answers as in localmap_cases.
"""
from __future__ import annotations

import random

import localmap_cases as L
from localmap_cases import BASE, _bump, keys_for

MUTANTS = ("self_counted", "bad_point_counted", "dup_point_once", "bad_observer_skipped", "th_gt",
           "max_ge", "max_always_added", "weights_thresholded", "ordered_full", "tie_ascending_key",
           "order_ascending", "parent_every_time", "parent_for_id0", "parent_back", "first_flag_kept",
           "empty_clears", "neighbour_not_told", "add_same_weight_resorts", "add_never_resorts",
           "resort_thresholded", "erase_absent_resorts", "erasekf_keeps_own", "by_weight_all")

OPS = ("update", "update_batch", "addconn", "eraseconn", "best", "erasekf", "setconn", "setordered",
       "setfirst", "byweight")
MAX_CONNECTIONS = L.MAX_VOTED   # entries of a counter / a weight map
TH = 15                         # KeyFrame.cc:1051


class Model(L.Model):
    """localmap_cases.Model plus, per keyframe: weights (dict), ordered (list of names), oweights,
    first (mbFirstConnection); parent and children are the base model's."""

    def apply(self, op):
        if op[0] == "kf":
            super().apply(op)
            kf = self.kfs[op[1]]
            kf.weights, kf.ordered, kf.oweights, kf.first = {}, [], [], True   # KeyFrame.cc:41
        else:
            super().apply(op)

    def key(self, name):
        return self.kfs[name].key

    def _set_ordered(self, kf, pairs):
        kf.ordered = [n for _, n in pairs]
        kf.oweights = [w for w, _ in pairs]
        kf.conn = list(kf.ordered)      # what UpdateLocalKeyFrames reads ten of

    def _sorted(self, pairs, mutant):
        """sort(vPairs) on pair<int, KeyFrame*>, then push_front (:1075-1082, :867-874)."""
        if mutant == "tie_ascending_key":
            out = sorted(pairs, key=lambda p: (p[0], -self.key(p[1])))
        else:
            out = sorted(pairs, key=lambda p: (p[0], self.key(p[1])))
        if mutant != "order_ascending":
            out.reverse()
        return out

    # ---- KeyFrame.cc:859-878
    def best(self, name, mutant=None, st=None):
        kf = self.kfs[name]
        pairs = [(w, o) for o, w in kf.weights.items()
                 if mutant != "resort_thresholded" or w >= TH]
        _bump(st, "best_sub_threshold" if any(w < TH for w in kf.weights.values()) else "best_all_over")
        self._set_ordered(kf, self._sorted(pairs, mutant))

    # ---- KeyFrame.cc:844-857
    def add_connection(self, name, other, w, mutant=None, st=None, via_update=False):
        kf = self.kfs[name]
        if other not in kf.weights:                                        # :848
            _bump(st, "add_insert")
            kf.weights[other] = w
        elif kf.weights[other] != w:                                       # :850
            _bump(st, "add_overwrite")
            kf.weights[other] = w
        else:
            _bump(st, "add_equal")
            if mutant != "add_same_weight_resorts":
                return                                                     # :853
        if mutant == "add_never_resorts":
            return
        if via_update:
            _bump(st, "told_changed")
        self.best(name, mutant, st)                                        # :856

    # ---- KeyFrame.cc:1295-1309
    def erase_connection(self, name, other, mutant=None, st=None):
        kf = self.kfs[name]
        update = False
        if other in kf.weights:                                            # :1300
            _bump(st, "erase_present")
            del kf.weights[other]
            update = True
        else:
            _bump(st, "erase_absent")
        if update or mutant == "erase_absent_resorts":
            self.best(name, mutant, st)                                    # :1308

    # ---- KeyFrame.cc:1188-1189, :1198-1199
    def erase_keyframe(self, name, mutant=None, st=None):
        kf = self.kfs[name]
        for o in sorted(kf.weights, key=self.key):                         # :1188
            self.erase_connection(o, name, mutant, st)
        _bump(st, "erasekf")
        if mutant != "erasekf_keeps_own":
            kf.weights = {}                                                # :1198
            self._set_ordered(kf, [])                                      # :1199

    # ---- KeyFrame.cc:905-920
    def by_weight(self, name, w, mutant=None, st=None):
        kf = self.kfs[name]
        if not kf.ordered:                                                 # :909
            _bump(st, "byw_empty")
            return []
        it = len(kf.oweights)
        for i, ow in enumerate(kf.oweights):   # upper_bound with weightComp(a, b) = a > b
            if w > ow:
                it = i
                break
        if it == len(kf.oweights):                                         # :913
            _bump(st, "byw_end")
            return list(kf.ordered) if mutant == "by_weight_all" else []
        _bump(st, "byw_some")
        return kf.ordered[:it]

    # ---- KeyFrame.cc:1023-1041
    def counter(self, name, mutant=None, st=None):
        kf = self.kfs[name]
        c, seen = {}, set()
        for mpn in kf.mps:                                                 # :1023, the vector
            if mpn is None:                                                # :1027
                _bump(st, "slot_null")
                continue
            mp = self.mps[mpn]
            if mp.bad and mutant != "bad_point_counted":                   # :1030
                _bump(st, "slot_bad")
                continue
            if mpn in seen:
                _bump(st, "slot_twice")
                if mutant == "dup_point_once":
                    continue
            seen.add(mpn)
            if name not in mp.obs:
                _bump(st, "held_unobserved")
            for o in mp.obs:                                               # :1035
                if o == name and mutant != "self_counted":                 # :1037
                    _bump(st, "obs_self")
                    continue
                if self.kfs[o].bad:
                    _bump(st, "obs_bad_kf")
                    if mutant == "bad_observer_skipped":
                        continue
                if mpn not in self.kfs[o].mps:
                    _bump(st, "obs_not_holding")
                c[o] = c.get(o, 0) + 1                                     # :1039
        return c

    # ---- KeyFrame.cc:1010-1100
    def update_connections(self, name, allow=None, mutant=None, st=None):
        kf = self.kfs[name]
        if allow is None:
            allow = kf.slot != 0                                           # mnId != 0
        c = self.counter(name, mutant, st)
        if not c:                                                          # :1044
            _bump(st, "counter_empty")
            if mutant == "empty_clears":
                kf.weights = {}
                self._set_ordered(kf, [])
            return
        nmax, kfmax, pairs = 0, None, []
        for o in sorted(c, key=self.key):                                  # :1055, pointer order
            n = c[o]
            if n > nmax or (mutant == "max_ge" and n >= nmax):             # :1057
                _bump(st, "max_new" if n > nmax else "max_mutant")
                nmax, kfmax = n, o
            elif n == nmax:
                _bump(st, "max_tie")
            if (n > TH) if mutant == "th_gt" else (n >= TH):               # :1062
                _bump(st, "over_th" if n > TH else "at_th")
                pairs.append((n, o))
                if mutant != "neighbour_not_told":
                    self.add_connection(o, name, n, mutant, st, True)      # :1065
            else:
                _bump(st, "below_th")
        if not pairs or mutant == "max_always_added":                      # :1069
            _bump(st, "max_rule")
            pairs.append((nmax, kfmax))
            if mutant != "neighbour_not_told":
                self.add_connection(kfmax, name, nmax, mutant, st, True)   # :1072
        if mutant == "weights_thresholded":
            kf.weights = {o: n for n, o in pairs}
        else:
            kf.weights = dict(c)                                           # :1088
        if mutant == "ordered_full":
            pairs = [(n, o) for o, n in c.items()]
        self._set_ordered(kf, self._sorted(pairs, mutant))                 # :1089-1090
        if not kf.first:
            _bump(st, "not_first")
        elif not allow:
            _bump(st, "first_id0")
        if (kf.first or mutant == "parent_every_time") and (allow or mutant == "parent_for_id0"):   # :1092
            _bump(st, "parent_set")
            kf.parent = kf.ordered[-1 if mutant == "parent_back" else 0]   # :1094
            self.kfs[kf.parent].children.add(name)                         # :1095
            if mutant != "first_flag_kept":
                kf.first = False                                           # :1096

    def graph(self):
        """name -> (weights in pointer order, ordered list with weights, parent, children in
        pointer order, flag)."""
        out = {}
        for n, kf in self.kfs.items():
            out[n] = ([(o, kf.weights[o]) for o in sorted(kf.weights, key=self.key)],
                      list(zip(kf.ordered, kf.oweights)), kf.parent,
                      sorted(kf.children, key=self.key), bool(kf.first))
        return out

    def run(self, op, mutant=None, st=None):
        """One script operation; the answer, or None for the map-building ones."""
        k = op[0]
        if k == "update":
            self.update_connections(op[1], op[2] if len(op) > 2 else None, mutant, st)
        elif k == "update_batch":
            allow = op[2] if len(op) > 2 else [None] * len(op[1])
            for n, a in zip(op[1], allow):
                self.update_connections(n, a, mutant, st)
        elif k == "addconn":
            self.add_connection(op[1], op[2], op[3], mutant, st)
        elif k == "eraseconn":
            self.erase_connection(op[1], op[2], mutant, st)
        elif k == "best":
            self.best(op[1], mutant, st)
        elif k == "erasekf":
            self.erase_keyframe(op[1], mutant, st)
        elif k == "setconn":
            self.kfs[op[1]].weights = dict(op[2])
        elif k == "setordered":
            self._set_ordered(self.kfs[op[1]], [(w, o) for o, w in op[2]])
        elif k == "setfirst":
            self.kfs[op[1]].first = bool(op[2])
        elif k == "byweight":
            return self.graph(), self.by_weight(op[1], op[2], mutant, st)
        elif k == "localmap":
            return self.update(op[1], op[2])
        else:
            self.apply(op)
            return None
        return self.graph()


def run_script(script, mutant=None, stats=None):
    m, out = Model(), []
    for op in script:
        a = m.run(op, mutant, stats)
        if a is not None:
            out.append(a)
    return out


# ---- the closed form of a sequential batch ----------------------------------------------------
def batch_closed_form(m, names, allows=None):
    """The graph after UpdateConnections on `names` in that order, computed without the loop from
    the model `m` (left as it is).  C_i depends on points and observations only; i tells j when
    C_i[j] >= 15, or when no count of i reaches 15 and j is i's lowest-key maximum."""
    allows = list(allows) if allows is not None else [None] * len(names)
    allows = [m.kfs[n].slot != 0 if a is None else a for n, a in zip(names, allows)]
    C = {n: m.counter(n) for n in names}
    tells = {}
    for i in names:
        told = {j: c for j, c in C[i].items() if c >= TH}
        if not told and C[i]:
            top = max(C[i].values())
            j = min((j for j, c in C[i].items() if c == top), key=m.key)
            told = {j: top}
        tells[i] = told
    pos = {n: p for p, n in enumerate(names)}

    def full(w):
        return sorted(((c, o) for o, c in w.items()), key=lambda p: (p[0], m.key(p[1])), reverse=True)

    g = m.graph()
    children = {n: set(g[n][3]) for n in g}
    out = {}
    for j, kf in m.kfs.items():
        own = j in pos and bool(C[j])
        base = dict(C[j]) if own else dict(kf.weights)
        changed = False
        for i in names:
            if i == j or (own and pos[i] < pos[j]) or j not in tells[i]:
                continue
            if base.get(i) != tells[i][j]:
                changed = True
            base[i] = tells[i][j]
        parent, first = kf.parent, bool(kf.first)
        ordered = list(zip(kf.ordered, kf.oweights))
        weights = dict(kf.weights)
        if own:
            weights = base
            th = full(tells[j])
            ordered = [(o, c) for c, o in (full(base) if changed else th)]
            if first and allows[pos[j]]:
                parent, first = th[0][1], False
                children[parent].add(j)
        elif changed:
            weights = base
            ordered = [(o, c) for c, o in full(base)]
        out[j] = (weights, ordered, parent, first)
    return {j: ([(o, w[o]) for o in sorted(w, key=m.key)], o_, p, sorted(children[j], key=m.key), f)
            for j, (w, o_, p, f) in out.items()}


# ---- the driver over native.LocalMap -----------------------------------------------------------
class LibraryRunner(L.LibraryRunner):
    """Replays a script on a ``native.LocalMap``; after every covisibility operation the complete
    graph state of every keyframe is read back through the getters.  `batch`: how an update_batch
    is run, "batch" (one call) or "single" (one call per keyframe)."""

    def __init__(self, lm, batch="batch"):
        super().__init__(lm)
        self.batch = batch

    def graph(self):
        lm, nm = self.lm, self.kf_names
        out = {}
        for s, n in enumerate(nm):
            ws, ww = lm.get_connections(s)
            os_, ow = lm.get_ordered_connections(s)
            p, f, ch = lm.get_spanning_tree(s)
            out[n] = ([(nm[a], int(b)) for a, b in zip(ws, ww)], [(nm[a], int(b)) for a, b in zip(os_, ow)],
                      None if p < 0 else nm[p], [nm[c] for c in ch], f)
        return out

    def _allow(self, names, allow):
        return [self.kf[n] != 0 if a is None else bool(a) for n, a in zip(names, allow)]

    def apply(self, op):
        k, lm = op[0], self.lm
        if k == "update":
            lm.UpdateConnections(self.kf[op[1]], self._allow([op[1]], [op[2] if len(op) > 2 else None])[0])
        elif k == "update_batch":
            allow = self._allow(op[1], op[2] if len(op) > 2 else [None] * len(op[1]))
            if self.batch == "batch":
                lm.UpdateConnections([self.kf[n] for n in op[1]], allow)
            else:
                for n, a in zip(op[1], allow):
                    lm.UpdateConnections(self.kf[n], a)
        elif k == "addconn":
            lm.AddConnection(self.kf[op[1]], self.kf[op[2]], op[3])
        elif k == "eraseconn":
            lm.EraseConnection(self.kf[op[1]], self.kf[op[2]])
        elif k == "best":
            lm.UpdateBestCovisibles(self.kf[op[1]])
        elif k == "erasekf":
            lm.erase_keyframe_connections(self.kf[op[1]])
        elif k == "setconn":
            lm.set_connections(self.kf[op[1]], [self.kf[o] for o, _ in op[2]], [w for _, w in op[2]])
        elif k == "setordered":
            lm.set_ordered_connections(self.kf[op[1]], [self.kf[o] for o, _ in op[2]], [w for _, w in op[2]])
        elif k == "setfirst":
            lm.set_first_connection(self.kf[op[1]], op[2])
        elif k == "byweight":
            return self.graph(), [self.kf_names[s] for s in lm.GetCovisiblesByWeight(self.kf[op[1]], op[2])]
        elif k == "localmap":
            return super().apply(("update",) + tuple(op[1:]))
        else:
            return super().apply(op)
        return self.graph()


# ---- built cases -------------------------------------------------------------------------------
def _kfs(s, names, v, slots=None):
    """Keyframes `names` with no points yet; keys against slot order (even v) or shuffled."""
    keys = keys_for(len(names), v)
    for n, k in zip(names, keys):
        s.append(("kf", n, k, [None] * (slots or 0)))


def _share(s, tag, holders, count, observers=None, start=None):
    """`count` new points held (appended at the end of the slots) and observed by `holders`;
    `observers` (default: the holders) are the keyframes in the points' observation sets."""
    pts = [f"{tag}{i}" for i in range(count)]
    s.append(("points", pts))
    s.append(("obs", [(p, o) for p in pts for o in (holders if observers is None else observers)]))
    return pts


def _world(v, spec, extra_obs=()):
    """spec: {tag: (holders, count[, observers])}.  Builds the keyframes (in the order of first
    mention, `Z` first so that slot 0 is a bystander) and their mvpMapPoints from the shared sets."""
    s, names, held = [], ["Z"], {}
    for tag, sp in spec.items():
        for n in list(sp[0]) + list(sp[2] if len(sp) > 2 else []):
            if n not in names:
                names.append(n)
    pts_of = {}
    for tag, sp in spec.items():
        pts = [f"{tag}{i}" for i in range(sp[1])]
        pts_of[tag] = pts
        s.append(("points", pts))
        for n in sp[0]:
            held.setdefault(n, []).extend(pts)
    keys = keys_for(len(names), v)
    for n, k in zip(names, keys):
        s.append(("kf", n, k, held.get(n, [])))
    for tag, sp in spec.items():
        obs = sp[2] if len(sp) > 2 else sp[0]
        s.append(("obs", [(p, o) for p in pts_of[tag] for o in obs]))
    return s, names


def case_threshold(v):
    """Counts 14 / 15 / 16, the max rule with one neighbour at 1, two and three keyframes tied at
    the maximum below 15, equal weights in the list, sub-threshold weights kept in the map."""
    s, names = _world(v, {"a": ("AB", 14), "b": ("AC", 15), "c": ("AD", 16), "d": ("AE", 15),
                          "e": ("FG", 1), "f": ("HI", 3 + v % 3), "g": ("HJ", 3 + v % 3),
                          "h": ("HK", 3 + v % 3 if v % 2 else 2)})
    s.append(("update", "A"))      # B 14 (out), C 15, D 16, E 15: list D, then C / E by descending key
    s.append(("update", "B"))      # only A at 14: the max rule
    s.append(("update", "F"))      # one neighbour at count 1
    s.append(("update", "H"))      # two or three tied below 15: the lowest key
    s.append(("update", "Z"))      # no points at all: nothing changes
    s.append(("byweight", "A", 15))
    s.append(("byweight", "A", 16))
    s.append(("byweight", "A", 17))
    s.append(("byweight", "Z", 1))
    s.append(("update_batch", ["C", "D", "E", "I", "J", "K", "G"]))
    s.append(("update_batch", names))
    return s


def case_points(v):
    """NULL and bad points, a point held at two indices, a keyframe among its own observers, a
    point held without being observed, observed without being held, a bad observer."""
    s, names = _world(v, {"a": ("AB", 13), "b": ("AC", 16), "n": ("A", 2, "D"), "m": ("AE", 20)})
    s.append(("kfpoints", "A", 0, ["a0", "a0"]))      # a0 at two indices: B counts 13 (a1 is gone)
    s.append(("kfpoints", "A", 13, [None]))           # b0 NULLed: C counts 15
    s.append(("mpbad", ["m0", "m1", "m2", "m3", "m4", "m5"], True))   # E counts 14
    s.append(("kfbad", "C", True))                    # observers are not tested for isBad
    s.append(("unobs", [("b1", "A")]))                # held by A, not observed by A: still counted
    s.append(("obs", [("n0", "B"), ("n1", "B")]))     # B observes without holding: B counts 15
    s.append(("update", "A"))
    s.append(("kfpoints", "A", 1, ["a1"]))
    if v % 2:
        s.append(("mpbad", ["m0"], False))            # E back to 15
    s.append(("update", "A"))
    s.append(("update_batch", ["B", "C", "D", "E"]))
    # every point NULL or bad: the counter is empty and the state stays
    s.append(("kfpoints", "B", 0, [None] * 13))
    s.append(("update", "B"))
    s.append(("mpbad", [f"m{i}" for i in range(20)], True))
    s.append(("update", "E"))
    s.append(("update_batch", ["E", "B", "A"]))
    return s


def case_tree(v):
    """The four first_connection x allow_parent combinations, the front of the list as parent with a
    tie at the top, the flag cleared, a second update that moves the front, AddChild as a union."""
    s, names = _world(v, {"a": ("AB", 20), "b": ("AC", 20), "c": ("AD", 18), "d": ("BC", 16)})
    s.append(("update", "A", False))                  # first, not allowed: no parent, flag kept
    s.append(("update", "A", True))                   # first, allowed: the higher key of B / C
    s.append(("setconn", "A", []))
    s.append(("points", ["x0", "x1", "x2"]))
    s.append(("kfpoints", "A", 0, ["x0", "x1", "x2"]))            # B drops to 17: C is the front now
    s.append(("update", "A", True))                   # not first: the parent stays
    s.append(("setfirst", "A", True))
    s.append(("update", "A", False))
    s.append(("update", "A", True))
    s.append(("children", "C" if v % 2 else "B", ["D", "Z"]))
    s.append(("update_batch", ["B", "C", "D", "Z"], [True, v % 2 == 0, True, True]))
    s.append(("setfirst", "B", True))
    s.append(("setfirst", "D", True))
    s.append(("update_batch", ["D", "B"]))
    return s


def case_addconn(v):
    """AddConnection's early return: an unchanged weight leaves a thresholded list alone, a changed
    or new one re-sorts the sub-threshold entries in; EraseConnection of a present and an absent
    key; UpdateBestCovisibles; the connection part of SetBadFlag."""
    s, names = _world(v, {"a": ("AB", 17), "b": ("AC", 15), "c": ("AD", 9), "d": ("AE", 4 + v),
                          "e": ("BC", 15), "f": ("BD", 3)})
    s.append(("update_batch", ["A", "B", "C", "D", "E"]))       # symmetric: every list thresholded
    s.append(("addconn", "A", "B", 17))               # equal weight: nothing
    s.append(("eraseconn", "A", "Z"))                 # absent: nothing
    s.append(("byweight", "A", 15))                   # every listed weight >= 15: the quirk
    s.append(("byweight", "A", 16))
    s.append(("addconn", "A", "B", 18))               # changed: D and E enter the list
    s.append(("update", "A"))                         # thresholded again; B is told 17 != its 18? no: B holds 17
    s.append(("addconn", "A", "Z", 0 if v % 2 else 30))         # absent key
    s.append(("best", "B"))
    s.append(("eraseconn", "A", "C"))                 # present
    s.append(("eraseconn", "B", "B"))
    s.append(("setordered", "D", [("A", 9)]))
    s.append(("addconn", "D", "A", 9))                # equal: the assigned list stays
    s.append(("erasekf", "C"))
    s.append(("update", "D"))                         # D: max rule (A at 9); A's entry is equal
    s.append(("erasekf", "A"))
    s.append(("erasekf", "Z"))
    s.append(("best", "Z"))
    s.append(("update_batch", ["E", "D", "C", "B", "A"]))
    return s


def case_asymmetric(v):
    """Asymmetric maps: i counts j without j counting i (or at another weight), so a tell changes a
    weight and the neighbour's list becomes the full sort; inside a batch, before and after the
    neighbour's own turn."""
    s, names = _world(v, {"a": ("A", 16, "AB"),      # A counts B at 16, B does not count A from these
                          "b": ("AB", 5), "c": ("BC", 15), "d": ("BD", 6 + v), "e": ("C", 15, "CD"),
                          "f": ("AD", 2)})
    s.append(("update", "B"))                         # B: A 5, C 15, D 6+v -> list [C]
    s.append(("update", "A"))                         # A tells B 21 != 5: B's list becomes the full sort
    s.append(("update_batch", ["B", "A"]))            # A after B: B's own list, then changed again
    s.append(("update_batch", ["A", "B"]))            # A before B: overwritten by B's own turn
    s.append(("update_batch", ["D", "C", "B", "A"]))
    s.append(("update_batch", ["C", "D"]))
    s.append(("setconn", "D", [("C", 15)]))
    s.append(("setordered", "D", [("Z", 3)]))
    s.append(("update", "C"))                         # tells D 15 == its 15: D's assigned list stays
    s.append(("kfbad", "B", True))
    s.append(("update_batch", names))
    s.append(("clear",))
    t, _ = _world(v + 1, {"a": ("AB", 15)})
    s.extend(t)
    s.append(("update_batch", ["B", "A"]))
    return s


CASES = {"threshold": case_threshold, "points": case_points, "tree": case_tree,
         "addconn": case_addconn, "asymmetric": case_asymmetric}
VARIANTS = range(6)


def built_scripts():
    for name, fn in CASES.items():
        for v in VARIANTS:
            yield f"{name}-{v}", fn(v)


def seeded_script(seed, nkf=9, npts=70, n_ops=10):
    """A random asymmetric map (a point held twice, held without being observed, observed without
    being held, a bad observer) and a random walk of edits, single updates and batches."""
    r = random.Random(seed)
    s = []
    pts = [f"p{i}" for i in range(npts)]
    s.append(("points", pts))
    kfs = [f"k{i}" for i in range(nkf)]
    keys = r.sample(range(1, 1 << 16), nkf)
    for i, n in enumerate(kfs):
        lo = r.randrange(0, npts - 30)
        window = pts[lo:lo + r.randrange(20, 45)]
        mps = [p if r.random() < 0.9 else None for p in window]
        mps += [r.choice(window)]                                   # held twice
        s.append(("kf", n, BASE + 16 * keys[i], mps))
        s.append(("obs", [(p, n) for p in mps[2:] if p is not None]))   # the first two: held, not observed
        s.append(("obs", [(r.choice(pts), n) for _ in range(3)]))       # observed, not held
    s.append(("kfbad", r.choice(kfs), True))                        # a bad observer
    s.append(("mpbad", r.sample(pts, 4), True))
    for _ in range(n_ops):
        c = r.random()
        if c < 0.2:
            s.append(("obs", [(r.choice(pts), r.choice(kfs)) for _ in range(6)]))
        elif c < 0.35:
            s.append(("unobs", [(r.choice(pts), r.choice(kfs)) for _ in range(6)]))
        elif c < 0.45:
            k = r.choice(kfs)
            s.append(("kfpoints", k, 0, [r.choice(pts + [None]) for _ in range(5)]))
        elif c < 0.5:
            s.append(("setfirst", r.choice(kfs), True))
        elif c < 0.6:
            s.append(("update", r.choice(kfs)))
        else:
            s.append(("update_batch", r.sample(kfs, r.choice((1, 2, 5, nkf)))))
    return s


# ---- the shapes at which a kernel can break (tests/test_gpu_covis.py) --------------------------
def script_observation_sets(sizes=(0, 1, 63, 64, 65, 200), v=1):
    """Keyframe Q holds one point per observation-set size, 15 times each; then all of them."""
    s = []
    nkf = max(sizes) + 1
    names = [f"K{i}" for i in range(nkf)]
    _kfs(s, names + ["Q"], v)
    tags = []
    for n in sizes:
        pts = [f"O{n}_{i}" for i in range(TH)]
        s.append(("points", pts))
        s.append(("obs", [(p, names[(7 * i) % nkf]) for p in pts for i in range(n)]))
        tags.append(pts)
    s.append(("kf", "R", BASE - 64, [p for pts in tags for p in pts]))
    for pts in tags:
        s.append(("kf", "Q" + pts[0], BASE - 128 - 64 * len(s), pts))
        s.append(("update", "Q" + pts[0]))
    s.append(("update", "R"))
    s.append(("update_batch", ["R"] + names[:70]))
    return s


def script_big_keyframe(v=0):
    """An 8,192-slot keyframe: one point in every slot, 5 observers that reach 15 at different
    slots, and a point repeated in the last 100 slots."""
    s = []
    _kfs(s, ["Z", "A", "B", "C", "D", "E"], v)
    pts = [f"q{i}" for i in range(L.MAX_KF_SLOTS)]
    s.append(("points", pts))
    s.append(("kf", "G", BASE + 0x40, pts[:-100] + [pts[-1]] * 100))
    s.append(("obs", [(p, "A") for p in pts[:14]] + [(p, "B") for p in pts[1000:1015]] +
              [(p, "C") for p in pts[::2]] + [(pts[-1], "D")] + [(pts[-1], "G")] + [(pts[5], "E")]))
    s.append(("update", "G"))
    s.append(("update_batch", ["A", "G", "D"]))
    return s


def script_many_neighbours(n, v=0):
    """Keyframe Q counts n distinct neighbours (one point each) and W, which it tells at 15."""
    s = []
    names = [f"K{i}" for i in range(n - 1)]
    _kfs(s, ["Z"] + names + ["W"], v)
    pts = [f"q{i}" for i in range(n - 1)]
    s.append(("points", pts + [f"w{i}" for i in range(TH)]))
    s.append(("obs", [(p, k) for p, k in zip(pts, names)] + [(f"w{i}", "W") for i in range(TH)]))
    s.append(("kf", "Q", BASE - 64, pts + [f"w{i}" for i in range(TH)]))
    return s


def script_children(counts=(0, 1, 64, 65), v=0):
    """Parents that already have 0, 1, 64 and 65 children get one more through UpdateConnections."""
    s = []
    total = sum(counts)
    kids = [f"c{i}" for i in range(total)]
    parents = [f"P{i}" for i in range(len(counts))]
    news = [f"N{i}" for i in range(len(counts))]
    spec = {f"s{i}": ((parents[i], news[i]), TH + i) for i in range(len(counts))}
    s, names = _world(v, spec)
    _kfs(s, kids, v + 1)
    # distinct keys for the second group
    s = [op if op[0] != "kf" or op[1] not in kids else ("kf", op[1], op[2] + 0x100000, op[3]) for op in s]
    rest = kids
    for p, c in zip(parents, counts):
        s.append(("children", p, rest[:c]))
        rest = rest[c:]
    s.append(("update_batch", news))
    s.append(("setfirst", news[-1], True))
    s.append(("update", news[-1]))              # already a child: the union changes nothing
    return s


def script_batches(nkf, order, v=0, window=6):
    """nkf keyframes in a sliding window (each shares 15 + points with its neighbours, asymmetric
    at every third, every seventh with no points), updated in one batch in `order`
    ("asc", "desc", "shuffled" by key)."""
    s = []
    names = [f"K{i}" for i in range(nkf)]
    keys = keys_for(nkf, v)
    held = {n: [] for n in names}
    obs = []
    allp = []
    for i in range(nkf):
        pts = [f"s{i}_{j}" for j in range(TH + i % 3)]
        allp += pts
        members = [names[(i + d) % nkf] for d in range(min(window, nkf))]
        for a, n in enumerate(members):
            if (i + a) % 7 == 6:
                continue
            held[n] += pts if a % 2 == 0 else pts[:10 + a]
            if not (i % 3 == 0 and a == 1):       # holds without observing
                obs += [(p, n) for p in pts]
    s.append(("points", allp))
    for i, n in enumerate(names):
        s.append(("kf", n, keys[i], [] if i % 7 == 3 else held[n]))
    s.append(("obs", [(p, n) for p, n in obs if names.index(n) % 7 != 3 or p.endswith("_0")]))
    by_key = sorted(names, key=lambda n: keys[names.index(n)])
    seq = {"asc": by_key, "desc": by_key[::-1],
           "shuffled": random.Random(nkf).sample(by_key, nkf)}[order]
    s.append(("update_batch", seq))
    return s
